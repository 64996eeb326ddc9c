/*
 * cslam.h -- C ABI of the MI355X-native EKF-SLAM / FastSLAM-2 engine (libcslam_hip.so).
 *
 * This is the drop-in boundary for the hot path of mfkiwl/conan-slam: the entry points below are what
 * a binding behind the reference's `class Slam` virtuals would call.  Each one cites the reference
 * interface it replaces (file:line relative to the reference tree).  Plain C types only: opaque handles,
 * raw pointers, sizes and status codes; no exceptions cross the boundary (the reference swallows its
 * exceptions and continues, e.g. EKF.cpp:125-128 -- a binding maps a non-zero status to that behaviour).
 *
 * Conventions (identical to the reference, which uses Eigen's defaults):
 *   - matrices are COLUMN-MAJOR; element (r,c) of a matrix with leading dimension ld is a[c*ld + r];
 *   - state X = [x, y, phi, lm1.x, lm1.y, ...], n = 3 + 2*N;  P is n x n;
 *   - feature indices `idf` are 1-BASED positions in the state (EKF.cpp:357, PF.cpp:86);
 *   - Z is 2 x m column-major: Z[2*i] = range, Z[2*i+1] = bearing (rad);
 *   - "scalar" pointers (const void*) point at elements of the dtype chosen at create time
 *     (float for CSLAM_F32 -- the reference's own precision -- or double for CSLAM_F64).
 *
 * Ownership: the handle owns the authoritative X and P in HBM (P preallocated for max_landmarks,
 * padded leading dimension).  Host copies are refreshed by get_x / get_state.  Calls on one handle are
 * stream-ordered and asynchronous unless stated otherwise; a handle is NOT thread-safe; distinct
 * handles are independent (own stream) and may be driven from distinct host threads.
 *
 * There is NO CPU fallback: every entry point fails with CSLAM_ERR_NO_DEVICE / CSLAM_ERR_HIP when no
 * gfx950 device or kernel image is available.
 */
#ifndef CSLAM_H
#define CSLAM_H

#ifdef __cplusplus
extern "C" {
#endif

#define CSLAM_VERSION 100

/* ---- status codes ---- */
#define CSLAM_OK 0
#define CSLAM_ERR_BAD_ARG 1    /* null pointer, negative size, idf out of range, wrong dtype ...      */
#define CSLAM_ERR_CAPACITY 2   /* state would exceed max_landmarks / max_features                     */
#define CSLAM_ERR_HIP 3        /* a HIP runtime call failed; see cslam_last_error()                   */
#define CSLAM_ERR_NO_DEVICE 4  /* no usable GPU                                                       */
#define CSLAM_ERR_ALLOC 5      /* host or device allocation failed                                    */
/* sticky per-handle factorisation flags (bit-or), read with cslam_ekf_factor_status() */
#define CSLAM_FACTOR_OK 0
#define CSLAM_FACTOR_FALLBACK 1 /* LLT of S failed; eigen "square root" taken (slam.h:425-429)        */
#define CSLAM_FACTOR_ZEROED 2   /* factor or its inverse non-finite -> update was a no-op (slam.h:252-255, 431-434) */
#define CSLAM_FACTOR_SKIPPED 4  /* async mode: LLT failed and the update was skipped (see set_sync_mode) */
#define CSLAM_FACTOR_INTERNAL 16 /* an internal wait of the look-ahead factor chain timed out (must never happen; results of
                                   that window are undefined) */
#define CSLAM_FACTOR_BAD_IDF 8  /* cslam_ekf_update_device: a device-resident feature index was outside 1..N; the kernels
                                   clamped it (no out-of-bounds access), the update used the clamped index           */
#define CSLAM_FACTOR_HEADING_SKIPPED 32 /* batched engine: a heading step met S = P22 + R <= 0 or non-finite (an
                                          indefinite P) and was skipped for that instance (cslam_ekf_batch_observe_heading) */
#define CSLAM_FACTOR_COUNT_CLAMPED 64 /* cslam_ekf_update_counted: *d_count was outside 0..m_cap and was clamped */

/* ---- precision ---- */
#define CSLAM_F32 0 /* the reference's precision (Eigen::MatrixXf everywhere)                          */
#define CSLAM_F64 1

/* ---- quirk flags: which of the reference's behaviours to reproduce ---- */
#define CSLAM_Q_LOWER_CHOL_GAIN 1 /* slam.h:250-260 with 423: gain built from inv(L), L lower          */
#define CSLAM_Q_PREDICT_NM4 2     /* EKF.cpp:442-443: cross-covariance stripe n-4 wide                 */
#define CSLAM_Q_REF_EXACT 3       /* both: bug-compatible with the reference (default for parity)      */
#define CSLAM_Q_TEXTBOOK 0        /* the algebra the reference meant                                   */

/* ---- profiling stages reported by cslam_ekf_get_stage_times ---- */
#define CSLAM_STAGE_GATHER 0   /* PHT = P*H^T (sparse gather form of slam.h:243)                       */
#define CSLAM_STAGE_FACTOR 1   /* S, symmetrise, chol, inverse (slam.h:244-255)                        */
#define CSLAM_STAGE_GAIN 2     /* W1 = PHT*G, X += W1*(G^T V) (slam.h:257-259)                         */
#define CSLAM_STAGE_DOWNDATE 3 /* P -= W1*W1^T (slam.h:260) -- the P-GEMM                              */
#define CSLAM_N_STAGES 4

typedef struct cslam_ekf* cslam_ekf_t;

/* ---- library-level ---- */
const char* cslam_last_error(void);       /* message of the last failing call on this thread          */
int cslam_version(void);
int cslam_device_count(int* count);

/* ================================ EKF-SLAM ================================================== */

/* Replaces: `new EKF(LM, WP)` + the caller-owned `Eigen::VectorXf X; Eigen::MatrixXf P`
 * (test/main.cpp:89,107-108).  State starts as X = 0_3, P = 0_3x3 as in the reference driver.
 * device < 0 selects the current HIP device. */
int cslam_ekf_create(int max_landmarks, int dtype, int device, int quirks, cslam_ekf_t* out);
int cslam_ekf_destroy(cslam_ekf_t h);

/* sync_mode = 1 (default): update() waits for its own completion and performs the reference's
 * eigen-decomposition fallback (slam.h:425-429) on the host when the LLT of S fails, exactly as the
 * reference would.  sync_mode = 0: fully asynchronous pipeline; a failed LLT makes that update a no-op
 * and raises CSLAM_FACTOR_SKIPPED (check cslam_ekf_factor_status). */
int cslam_ekf_set_sync_mode(cslam_ekf_t h, int sync_mode);

/* Upload / download the state.  X: n scalars; P: n x n, leading dimension ldp (>= n), both host memory.
 * These are what a binding uses where the reference passes X and P by reference into every call. */
int cslam_ekf_set_state(cslam_ekf_t h, const void* X, int n, const void* P, int ldp);
int cslam_ekf_get_state(cslam_ekf_t h, void* X, void* P, int ldp); /* synchronises */
int cslam_ekf_get_x(cslam_ekf_t h, void* X, int capacity);         /* synchronises; writes n scalars */
int cslam_ekf_get_n(cslam_ekf_t h, int* n);
/* The means and marginal covariances of landmarks first .. first+count-1 (1-based feature numbers, as idf;
 * 1 <= first, first+count-1 <= N = (n-3)/2, count >= 0), in the handle's dtype:
 *   x   [count][2]  X[fx], X[fx+1]                         (fx = 3 + 2*(f-1), 0-based)
 *   pll [count][4]  P[fx:fx+2, fx:fx+2], 2 x 2 column-major, exactly symmetric
 *   pvl [count][6]  P[0:3, fx:fx+2], 3 x 2 column-major
 * This replaces the caller reading X and P directly, which the reference allows because the driver owns them and
 * passes them by reference (test/main.cpp:107-108); the reference's data association reads exactly these blocks
 * through H*P*H^T (computeAssociation, EKF.cpp:131-144).  Unlike get_state / trace it NEVER applies the pending
 * covariance downdate, mirrors P or copies P: the 2 x 2 blocks are read from the deferred form (P = Ps - Wp Wp^T over
 * the pending columns), so a run that reads its landmarks ends bit for bit where the same run without the reads ends.
 * Queued work is launched first, exactly as get_x does: a held predict, the pose queue, and a queued look-ahead
 * update (as a window of one -- that update alone then rounds as a window of one would).  Two-stream mode
 * (CSLAM_PIPELINE=1): the read waits for the P-GEMMs in flight.  Any output may be NULL, not all three; count = 0
 * returns CSLAM_OK at once; a bad range returns CSLAM_ERR_BAD_ARG and changes nothing.  Synchronises. */
int cslam_ekf_get_landmarks(cslam_ekf_t h, int first, int count, void* x, void* pll, void* pvl);
int cslam_ekf_trace(cslam_ekf_t h, double* trace);                 /* synchronises */
/* The pose X[0:3] and the full 3 x 3 pose block P[0:3, 0:3] (column-major), in the handle's dtype: the single-handle
 * sibling of cslam_ekf_batch_get_poses (the pose test/main.cpp:136 prints; the block EKF.cpp:131-144 reads through
 * H*P*H^T; what Slam::predict, slam.h:841-847, propagates).  Queued work is launched first exactly as get_landmarks does;
 * the block is read from the pose stripe, which is always current: no covariance downdate, no P-GEMM, no copy of P, and
 * the run continues bit for bit as without the read.  Both outputs are required (NULL: CSLAM_ERR_BAD_ARG).  Synchronises. */
int cslam_ekf_get_pose(cslam_ekf_t h, void* x /* [3] */, void* pvv /* [9] */);            /* synchronises; no flush */
int cslam_ekf_synchronize(cslam_ekf_t h);
int cslam_ekf_factor_status(cslam_ekf_t h, int* flags, int clear); /* synchronises */

/* Replaces Slam::predict(X, P, v, swa, Q, wb, dt)  -- slam.h:841-847, EKF.cpp:406-455.
 * Q: 2x2 scalars. */
int cslam_ekf_predict(cslam_ekf_t h, double v, double swa, const void* Q, double wb, double dt);

/* Replaces Slam::update(X, P, Z, R, idf, batch)  -- slam.h:938-943, EKF.cpp:481-496
 * (batchUpdate EKF.cpp:93-129, singleUpdate EKF.cpp:457-479, observeModel EKF.cpp:354-404,
 *  choleskyUpdate slam.h:235-266).  Z: 2 x m scalars, R: 2x2 scalars, idf: m ints (1-based), all host
 * memory, consumed before return.  m = 0 is a no-op, as in the reference. */
int cslam_ekf_update(cslam_ekf_t h, const void* Z, int m, const void* R, const int* idf, int batch);

/* Same, with Z and idf already resident in device memory (HBM); R stays a host pointer (4 scalars).  The host cannot
 * check device-resident indices: every kernel clamps them into 1..N before it forms an address and
 * CSLAM_FACTOR_BAD_IDF is raised (cslam_ekf_factor_status) when one was out of range.
 * Lifetime: dZ / d_idf are read only by work that this call enqueues on the handle's streams (an update that a
 * look-ahead window keeps queued past the call is read from a copy the call takes on the device).  The caller must
 * keep both arrays unchanged until that work has run -- for example until cslam_ekf_synchronize returns, or until the
 * handle's streams (cslam_ekf_get_streams) or the whole device have been synchronised, which keeps a queued look-ahead
 * update queued; after that the buffers may be rewritten for the next call.  Writes the caller makes on another stream
 * must be complete (or ordered before the handle's streams) when the call is made. */
int cslam_ekf_update_device(cslam_ekf_t h, const void* dZ, int m, const void* R, const int* d_idf, int batch);

/* Replaces Slam::augment(X, P, Z, R)  -- slam.h:190-191, EKF.cpp:9-26 / addOneNewFeature EKF.cpp:28-91.
 * Z: 2 x q scalars (host). Fails with CSLAM_ERR_CAPACITY beyond max_landmarks. */
int cslam_ekf_augment(cslam_ekf_t h, const void* Z, int q, const void* R);

/* Slam::augment (test/main.cpp:188-189, slam.h:190-191, EKF.cpp:9-26 / addOneNewFeature EKF.cpp:28-91) with the new
 * features read from device memory: the result -- X, P and n, bit for bit -- is that of cslam_ekf_augment(h, Z, q, R)
 * with Z the first 2q scalars of dZ.  dZ: 2 x q scalars (r, b) in the handle's dtype, column-major, in HBM; entries
 * beyond 2q are never read.  R is a host pointer (4 scalars).  The q features are added by ONE kernel launch per 64
 * features (a call with q <= 64 is exactly one launch), where cslam_ekf_augment launches once per feature.
 * Queued work (a held predict, the pose queue, a queued look-ahead update) is launched first, as by cslam_ekf_augment;
 * pending covariance columns stay pending, their rows for the new features are zero.
 * q = 0 returns CSLAM_OK and launches no augment kernel.  q < 0, a NULL R, or a NULL dZ with q > 0 returns
 * CSLAM_ERR_BAD_ARG; more than max_landmarks features in all returns CSLAM_ERR_CAPACITY; on either error nothing changes.
 * Lifetime of dZ: as for cslam_ekf_update_device -- it is read by work this call enqueues on the chain stream, and
 * nothing is held past the call.  The dZN of cslam_ekf_association_device_ptrs and of cslam_sim_device_ptrs may be passed
 * directly, with the count the host learnt from cslam_ekf_association_wait / cslam_sim_associate_table.
 * Works in every mode in which cslam_ekf_augment works. */
int cslam_ekf_augment_device(cslam_ekf_t h, const void* dZ, int q, const void* R);

/* Augment kernel launches of this handle so far, from cslam_ekf_augment (one per feature) and cslam_ekf_augment_device
 * (one per 64 features): a host-side counter, like cslam_ekf_stage_launches. */
int cslam_ekf_augment_launches(cslam_ekf_t h, long long* launches);

/* Replaces Slam::observeHeading(X, P, phi, useHeading)  -- slam.h:788, EKF.cpp:328-352 with
 * josephUpdate slam.h:700-725.  With H = e_2^T the Joseph form equals P - p p^T / S (p = P[:,2], S = P22 + R) for a
 * symmetric P: the pose stripe is updated at once, the map block receives the rank-1 downdate as one more pending
 * column of the next P-GEMM.  O(n); a predict() issued just before it runs in the same launch. */
int cslam_ekf_observe_heading(cslam_ekf_t h, double phi, int use_heading);

/* Gated nearest-neighbour data association: Slam::dataAssociate (slam.h, implemented at EKF.cpp:235-326 with
 * EKF::computeAssociation EKF.cpp:131-144).  Z: 2 x m observations (host pointer, column-major), R: 2 x 2.
 * For observation i: kind_out[i] = 1 and idf_out[i] = the 1-based feature with the smallest normalised distance
 * among those whose normalised innovation squared is below gate1; otherwise idf_out[i] = 0 and kind_out[i] = 2 when
 * the best NIS of the remaining features exceeds gate2 (far enough to be a new feature) or 0 (ambiguous: dropped).
 * The reference's own return value carries an EMPTY new-feature list (EKF.cpp:307 re-declares ZN, :311 never
 * advances the column): a REF_EXACT caller ignores kind == 2, see conan_slam_amd/ekf.py::data_associate.
 * Synchronous (results are written to host memory). Pending deferred downdates are applied first. */
int cslam_ekf_associate(cslam_ekf_t h, const void* Z, int m, const void* R, double gate1, double gate2, int* idf_out,
                        int* kind_out);

/* The same association -- Slam::dataAssociate, EKF.cpp:235-326 with EKF::computeAssociation EKF.cpp:131-144 -- read from
 * the deferred form of the covariance (P = Ps - Wp diag(s) Wp^T over the pending columns) WITHOUT applying it: nothing is
 * flushed, the pending columns, their signs and P stay as they are, and the run continues bit for bit as without the
 * call.  Rule and measure are those of cslam_ekf_associate: kind 1 / 2 / 0, idf 1-based or 0, all four entries of R read,
 * strict comparisons, a NaN takes part in none, an empty map gives kind 2 everywhere.  Queued work is launched first
 * exactly as cslam_ekf_get_landmarks does (a held predict, the pose queue, a queued look-ahead update as a window of
 * one); two-stream mode (CSLAM_PIPELINE=1) waits for the P-GEMMs in flight.
 * Host results: idf_out[m], kind_out[m], counts_out[3] = {mf, mn, dropped}; any of the three may be NULL.  They come
 * back in one copy; the call synchronises the chain stream.  The split the reference returns (slam.h:482-487) stays on
 * the device, in observation order: ZF (2 x mf, kind 1), their features idf_f (mf), ZN (2 x mn, kind 2) and the counts,
 * see cslam_ekf_association_device_ptrs.  CSLAM_Q_REF_EXACT does not empty ZN here (EKF.cpp:307 stays a policy of the
 * callers, as for cslam_ekf_associate).
 * m = 0 returns CSLAM_OK at once with counts 0, launches nothing and leaves the device lists of the previous call as they
 * are; m < 0, a NULL R, or a NULL Z with m > 0 returns CSLAM_ERR_BAD_ARG and changes nothing.  Any m is allowed. */
int cslam_ekf_associate_deferred(cslam_ekf_t h, const void* Z, int m, const void* R, double gate1, double gate2,
                                 int* idf_out, int* kind_out, int* counts_out /* [3]: mf, mn, dropped */);

/* The device lists of the last cslam_ekf_associate_deferred call with m > 0 (the ZF / idf / ZN of Slam::dataAssociate,
 * EKF.cpp:235-326, slam.h:482-487), in the handle's dtype: dZF (2 x mf), d_idf (mf ints, 1-based), dZN (2 x mn),
 * d_counts (3 ints).  Any output may be NULL.  The pointers are valid until the next associate_deferred call on the
 * handle, which rewrites (and may move) them.  They are fit for cslam_ekf_update_device(h, dZF, mf, R, d_idf, batch)
 * under the lifetime rules stated there: the next associate_deferred call launches what is queued and is ordered behind
 * it on the handle's chain stream.  Before any such call: CSLAM_ERR_BAD_ARG. */
int cslam_ekf_association_device_ptrs(cslam_ekf_t h, const void** dZF, const int** d_idf, const void** dZN,
                                      const int** d_counts);

/* cslam_ekf_associate_deferred without the wait (Slam::dataAssociate, EKF.cpp:235-326): the same argument checks, the
 * same launch of queued work, the same kernels and the same single copy of counts / idf / kind into pinned host memory;
 * then an event is recorded on the chain stream and the call returns.  Z is consumed before it returns.  The device
 * lists (cslam_ekf_association_device_ptrs) may be handed to cslam_ekf_update_counted at once: the split the reference
 * returns (slam.h:482-487) is read there in stream order.  m = 0 launches nothing; its cslam_ekf_association_wait
 * returns counts 0.  Growing the lists for a larger m synchronises the chain stream, as the synchronous call does. */
int cslam_ekf_associate_deferred_async(cslam_ekf_t h, const void* Z, int m, const void* R, double gate1, double gate2);

/* Waits for the event of the outstanding cslam_ekf_associate_deferred_async call and hands out idf_out[m], kind_out[m],
 * counts_out[3] = {mf, mn, dropped} (any of the three may be NULL).  It waits for the association only, not for work
 * enqueued behind it.  CSLAM_ERR_BAD_ARG when no asynchronous call is outstanding: each call is waited for once, and a
 * later associate call on the handle, synchronous or asynchronous, discards the outstanding results. */
int cslam_ekf_association_wait(cslam_ekf_t h, int* idf_out, int* kind_out, int* counts_out /* [3]: mf, mn, dropped */);

/* Slam::update with batch = 1 (slam.h:938-943, batchUpdate EKF.cpp:93-129) for the first c = *d_count observations of
 * dZ / d_idf, where d_count points to ONE int in device memory that every kernel of the call reads in stream order --
 * for example d_counts of cslam_ekf_association_device_ptrs, whose first entry is the row count mf of the ZF the
 * reference splits off (slam.h:482-487).  The result is that of cslam_ekf_update_device(h, dZ, c, R, d_idf, 1); the
 * call never waits for the device and copies nothing from it, so the host need not know c.
 *   dZ: 2 x m_cap scalars, column-major; d_idf: m_cap ints; only the first c entries of each are read.  Entries
 *   c .. m_cap-1 may hold anything (NaN, 0, negative or out-of-range ids): they influence nothing and never raise
 *   CSLAM_FACTOR_BAD_IDF.  Lifetime of dZ / d_idf / d_count: as for cslam_ekf_update_device.
 *   A count outside 0..m_cap is clamped into it and CSLAM_FACTOR_COUNT_CLAMPED is raised (cslam_ekf_factor_status).
 *   c = 0 changes nothing (a held predict has still been applied).
 * Accepted: 1 <= m_cap <= 64 (f32) or 32 (f64), the ranges of the tuned factor and gain kernels; m_cap = 0 returns
 * CSLAM_OK and does nothing.  A larger m_cap, m_cap < 0, batch = 0, sync_mode = 1, two-stream mode (CSLAM_PIPELINE=1) or
 * a NULL dZ / R / d_idf / d_count returns CSLAM_ERR_BAD_ARG and changes nothing.
 * The host plans for m_cap: 2 m_cap pending columns are booked under the deferral and flush rules of
 * cslam_ekf_update_device with m = m_cap, of which the columns beyond 2c are exact zeros.  Queued work (a held predict,
 * the pose queue, a queued look-ahead update as a window of one) is launched first; the counted update itself never
 * joins a look-ahead window.  cslam_ekf_debug_last_update returns CSLAM_ERR_BAD_ARG after a counted call (its k is
 * known on the device only). */
int cslam_ekf_update_counted(cslam_ekf_t h, const void* dZ, int m_cap, const void* R, const int* d_idf, const int* d_count,
                             int batch);

/* Deferred downdates.  slam.h:260 (P = P - W1*W1^T) is linear in the W1 panels, so the engine may keep
 * P = Ps - Wp*Wp^T with up to max_pending_columns columns of not-yet-applied panels and apply them in ONE
 * P-GEMM (k = pending columns): every reader of P adds the rank-k correction for the columns it touches, so
 * results are the reference's up to rounding.  0 (default) applies each update's downdate at once.  The
 * sequential form update(batch = 0) always defers its m rank-2 downdates to one pass at the end of the call
 * (SURVEY.md 8f rank 2).  get_state / trace / associate / flush apply whatever is pending.
 * With 0 every batch update's P-GEMM is applied within its call; a window lets the P-GEMM of pending panels run
 * later, under the next updates (and, in asynchronous mode, lets batch updates pair into look-ahead windows). */
int cslam_ekf_set_deferred(cslam_ekf_t h, int max_pending_columns);
int cslam_ekf_flush(cslam_ekf_t h);

/* The two HIP streams (hipStream_t) of a handle: the chain stream carries everything except the covariance downdate,
 * the P-GEMM stream carries P -= W1*W1^T of the previous update (the same stream when the engine is not pipelined).
 * For callers that want to order their own work (event records, input copies) against the engine's. */
int cslam_ekf_get_streams(cslam_ekf_t h, void** chain_stream, void** pgemm_stream);

/* Look-ahead windows (pairs of asynchronous batch updates issued together, or a single update drained alone) that this
 * handle has launched so far: lets a caller or a test confirm which schedule ran. */
int cslam_ekf_lookahead_windows(cslam_ekf_t h, long long* windows);

/* Launches of the kernel that snapshots a queued update's device-resident inputs into the handle's staging ring.  In a
 * run of look-ahead windows only the first window after a drain needs one: from then on the previous window's wide
 * kernel carries the copy (CSLAM_LA_HOLD_WIDE=0: every window).  Lets a test confirm which of the two ran. */
int cslam_ekf_stage_launches(cslam_ekf_t h, long long* launches);

/* Launches of the kernel that gathers the rows of the pending panels for a look-ahead window's small blocks.  In a run of
 * f32 windows of two 32-observation updates the preceding window's wide kernel leaves a row-major mirror of its panels
 * and the blocks kernel reads that instead, so the count stays where it was; a window that starts from pending columns the
 * mirror does not cover (or CSLAM_LA_MIRROR=0: every window) launches the rows kernel.  Lets a test confirm which ran. */
int cslam_ekf_rows_launches(cslam_ekf_t h, long long* launches);

/* Cap on the workgroups of the persistent covariance-downdate kernel (0 = default: two per compute unit, i.e. the
 * whole chip).  For several filter instances that run side by side on one GPU (Monte-Carlo runs, one stream each): with
 * the default every instance's P-GEMM occupies all compute units for its duration and the other instances' small
 * kernels queue behind it; with e.g. 2 * CUs / instances each instance keeps to its share and their kernels interleave. */
int cslam_ekf_set_pgemm_workgroups(cslam_ekf_t h, int workgroups);

/* Whole 128 x 128 tiles and 32-row strips of the handle's last f32 covariance-downdate launch of at most 128 columns (the
 * kernel's tail phase, CSLAM_PGEMM_TAIL; strips = 0: the launch without it).  Lets a test confirm that the strip path ran. */
int cslam_ekf_pgemm_split(cslam_ekf_t h, int* whole_tiles, int* strips);

/* Monte-Carlo driver (BASELINE configs[4]; the reference's unit is one filter loop, test/main.cpp:132-200): runs
 * `steps` x { predict(v[t], swa[t], Q, wb, dt); update(Z_t, R, idf_t, batch) } on each of `count` INDEPENDENT filter
 * handles at once, one host thread and one stream pair per handle.  dZ[i] / d_idf[i]: device-resident inputs of
 * instance i, steps x (2*m scalars) and steps x (m ints), step-major.  Returns when every instance has been enqueued
 * (asynchronous mode) or has finished (sync mode); cslam_ekf_synchronize waits for an instance. */
int cslam_ekf_run_many(cslam_ekf_t* handles, int count, int steps, const double* v, const double* swa, const void* Q,
                       double wb, double dt, const void* const* dZ, const int* const* d_idf, int m, const void* R,
                       int batch);

/* Batched Monte-Carlo engine (BASELINE configs[4], test/main.cpp:132-200 x I): `instances` INDEPENDENT f32 filters of the
 * same size n = 3 + 2 * n_landmarks (common to the instances; it grows with cslam_ekf_batch_augment up to the capacity
 * given at create time) advance in lockstep, every stage of the step ONE launch for all of them
 * (conan_slam_amd/csrc/cslam_ekf_batch.hip).  The arithmetic per instance is cslam_ekf_update's (batch form with the
 * predict held back and applied inside the update, look-ahead windows of two updates): an instance's results are bitwise
 * those of a single handle that runs the same pairs of updates as look-ahead windows.
 *   run: `steps` x { predict(v[t], swa[t], Q, wb, dt); update(Z_t, R, idf_t, batch) } on every instance; the controls are
 *        common to the instances (as in cslam_ekf_run_many), dZ[i] / d_idf[i] are instance i's device-resident inputs,
 *        steps x (2*m floats) and steps x (m ints), step-major; 9 <= m <= 32 (smaller scans: update).  Asynchronous: returns when the work has
 *        been enqueued.  Feature indices are checked on the device (CSLAM_FACTOR_BAD_IDF).  Windows are formed within a
 *        call -- steps (0,1), (2,3), ...; an odd call ends with a window of one update -- so the rounding of a run depends
 *        on how its steps are cut into calls (as a single handle's does on when its updates arrive).
 *   flush applies the pending covariance panels; get_state / trace flush and synchronise; factor_status synchronises and
 *   writes one flag word per instance.  instances * (round_up(n, 128))^2 * 4 must stay below 4 GiB. */
typedef struct cslam_ekf_batch* cslam_ekf_batch_t;
int cslam_ekf_batch_create(int instances, int n_landmarks, int device, int quirks, cslam_ekf_batch_t* out);
int cslam_ekf_batch_destroy(cslam_ekf_batch_t h);
int cslam_ekf_batch_set_state(cslam_ekf_batch_t h, int instance, const float* X, int n, const float* P, int ldp);
int cslam_ekf_batch_get_state(cslam_ekf_batch_t h, int instance, float* X, float* P, int ldp);
int cslam_ekf_batch_run(cslam_ekf_batch_t h, int steps, const double* v, const double* swa, const float* Q, double wb,
                        double dt, const float* const* dZ, const int* const* d_idf, int m, const float* R);
int cslam_ekf_batch_flush(cslam_ekf_batch_t h);
int cslam_ekf_batch_synchronize(cslam_ekf_batch_t h);
int cslam_ekf_batch_trace(cslam_ekf_batch_t h, double* traces /* [instances] */);
int cslam_ekf_batch_factor_status(cslam_ekf_batch_t h, int* flags /* [instances] */);
int cslam_ekf_batch_info(cslam_ekf_batch_t h, int* instances, int* n, long long* windows);
/* HIP events around one covariance-downdate launch in `every` (0 stops; at most 256 launches are kept; synchronises);
 * get: synchronises, sum of milliseconds and number of the launches timed since profiling was switched on. */
int cslam_ekf_batch_set_profiling(cslam_ekf_batch_t h, int every);
int cslam_ekf_batch_get_pgemm_time(cslam_ekf_batch_t h, double* ms_sum, int* launches);
/* As cslam_ekf_pgemm_split, of the batch's last covariance-downdate launch (all instances together). */
int cslam_ekf_batch_pgemm_split(cslam_ekf_batch_t h, int* whole_tiles, int* strips);

/* ---- the reference's filter loop through the batch (test/main.cpp:132-200: predict + observeHeading per control step,
 *      update + augment per observation step), one call per reference call, every call one state for all instances.
 * Calls are queued as in a single handle: predict is held; observe_heading joins it into one step of a pose queue (up to
 * 8 steps per launch); update launches the queued steps, then one look-ahead window of ONE update with the held predict
 * inside it; augment launches what is queued, then the new features.  run / flush / synchronize / get_state / trace /
 * factor_status / set_state first launch whatever these calls left queued (a held predict becomes a predict-only step);
 * for a handle that never used them that is nothing.  Device inputs are read in stream order: the arrays behind dZ /
 * d_idf / dZn must stay unchanged until the work of the call has run (as for cslam_ekf_batch_run); the host arrays of
 * pointers are consumed before the call returns.  Asynchronous: the calls return when the work has been enqueued. */
/* Like cslam_ekf_batch_create, but sized for max_landmarks.  Every instance starts with n_landmarks landmarks
 * (0 = the reference driver's X = 0_3, P = 0_3x3, test/main.cpp:107-108), and the map grows with
 * cslam_ekf_batch_augment.  cslam_ekf_batch_create(I, N, ...) behaves exactly as create_capacity(I, N, N, ...).
 * cslam_ekf_batch_info reports the current n; set_state requires n equal to it. */
int cslam_ekf_batch_create_capacity(int instances, int max_landmarks, int n_landmarks, int device, int quirks,
                                    cslam_ekf_batch_t* out);
/* Slam::predict (slam.h:841-847, EKF.cpp:406-455) on every instance.  The controls are common to all instances, as in
 * cslam_ekf_batch_run. */
int cslam_ekf_batch_predict(cslam_ekf_batch_t h, double v, double swa, const float* Q, double wb, double dt);
/* Slam::predict (slam.h:841-847, EKF.cpp:406-455) with controls per instance: v / swa are host arrays of `instances`
 * values, and instance i predicts exactly as cslam_ekf_predict would with (v[i], swa[i]); Q, wb and dt are common.  This
 * is the reference's Monte-Carlo control noise: mSwitchControlNoise (on by default) draws fresh (vn, swan) for every run
 * and step (slam.h:149-159, test/main.cpp:160-165).  The values are consumed before the call returns.  Queueing rules:
 *   - observe_heading right after it joins it into one pose-queue step, as after cslam_ekf_batch_predict;
 *   - update, augment, predict, predict_each and every call that drains the queue first launch it as a predict-only
 *     pose step: a per-instance predict is NEVER carried into a look-ahead window (whose kernels take the predict by
 *     value, common to the instances).
 * Called with equal values in every instance it gives the results of cslam_ekf_batch_predict followed by the same calls,
 * bit for bit, when the next call is observe_heading. */
int cslam_ekf_batch_predict_each(cslam_ekf_batch_t h, const double* v, const double* swa, const float* Q, double wb,
                                 double dt);
/* The pose X[0:3] and the 3 x 3 pose block P[0:3, 0:3] (column-major) of every instance, after launching whatever is
 * queued (as the other reads do): 48 bytes per instance, no covariance downdate and no copy of P.  Synchronises.
 * x: [instances][3], pvv: [instances][9]; either may be NULL. */
int cslam_ekf_batch_get_poses(cslam_ekf_batch_t h, float* x, float* pvv);
/* cslam_ekf_get_landmarks for every instance (same arguments, blocks and guarantees): x [instances][count][2],
 * pll [instances][count][4], pvl [instances][count][6].  Launches what is queued (as get_poses), then reads the pending
 * region as it stands: no covariance downdate, no mirror and no copy of P -- 12 floats per instance and landmark -- and
 * the run continues bit for bit as without the read.  For Monte-Carlo scoring of the map (landmark error and NEES,
 * e^T P_jj^-1 e) in place of get_state (test/main.cpp:107-108; the blocks EKF.cpp:131-144 reads).  Synchronises. */
int cslam_ekf_batch_get_landmarks(cslam_ekf_batch_t h, int first, int count, float* x, float* pll, float* pvl);

/* ---- the score of a Monte-Carlo study, kept on the device (conan_slam_amd/csrc/ekf_score_kernels.hpp).  The reference
 *      has no scorer: these calls replace the host-side scoring a study does with get_poses and get_landmarks after every
 *      observation step -- the pose test/main.cpp:136 prints against the true pose, and the blocks EKF.cpp:131-144 reads
 *      against a true position per state feature.  All error and NEES arithmetic is f64 on the device from the f32
 *      state; the sums are formed in a fixed order without atomics, so the totals of a run are reproducible bit for
 *      bit.  The single handle (f32 and f64) has the same scorer, cslam_ekf_score* below, and the particle filter its
 *      own, cslam_pf_score* further down: the same rules and the same total indices.
 * Indices into one instance's totals (doubles): */
enum { CSLAM_SCORE_POSE_N, CSLAM_SCORE_POSE_BAD, CSLAM_SCORE_POSE_IN, CSLAM_SCORE_POSE_ERR2 /* sum ex^2+ey^2 */,
       CSLAM_SCORE_POSE_EPHI2 /* sum wrapped heading error^2 */, CSLAM_SCORE_POSE_NEES /* sum e^T Pvv^-1 e */,
       CSLAM_SCORE_LM_N, CSLAM_SCORE_LM_BAD, CSLAM_SCORE_LM_IN, CSLAM_SCORE_LM_ERR2, CSLAM_SCORE_LM_NEES,
       CSLAM_SCORE_FIELDS };
/* Zeroes the totals, the series and the call count (replaces scoring state kept on the host beside test/main.cpp:136).
 * series_capacity >= 0 records of [instances][4] floats (0: totals only).  A gate <= 0 selects the 95 % chi-square
 * point: 7.8147 for the pose (3 degrees of freedom), 5.9915 for a landmark (2).  The truth rows are kept.  A score call
 * without a prior reset behaves as after score_reset(h, 0, 0, 0).  A handle that never calls a score function allocates
 * nothing for it. */
int cslam_ekf_batch_score_reset(cslam_ekf_batch_t h, int series_capacity, double gate_pose, double gate_lm);
/* The true position of state feature j + 1 is row j of lm_true (host, [count][2]; the features of EKF.cpp:131-144),
 * copied into a device buffer sized for max_landmarks before the call returns.  Features beyond `count` are not scored.
 * count > max_landmarks: CSLAM_ERR_BAD_ARG, nothing changed. */
int cslam_ekf_batch_score_set_truth(cslam_ekf_batch_t h, const float* lm_true /* host [count][2] */, int count);
/* One score step against the true pose xv_true (host [3], consumed before the call returns; the pose of
 * test/main.cpp:136 and the blocks of EKF.cpp:131-144).  Launches what is queued exactly as get_landmarks does (no
 * covariance downdate: the pending columns stay pending and the run continues bit for bit as without the call), then
 * the score kernels on the main stream, and returns when the work is enqueued: no synchronise, no device-to-host copy.
 *   pose      e = (x - xt, y - yt, wrap(phi - phit)) with the heading error wrapped to (-pi, pi]; NEES = e^T Pvv^-1 e by
 *             a 3 x 3 Cholesky.  A pivot <= 0 or anything non-finite: POSE_BAD += 1, nothing enters the sums.  Otherwise
 *             POSE_N, ERR2, EPHI2, NEES accumulate and POSE_IN += (NEES <= gate_pose).
 *   landmark  e = x_j - truth_j, NEES = (p11 e0^2 - 2 p10 e0 e1 + p00 e1^2) / det over the 2 x 2 marginal get_landmarks
 *             would return.  p00 <= 0, det <= 0 or anything non-finite (a truth row included): LM_BAD += 1.  Otherwise
 *             as the pose, with gate_lm.
 *   series    while there is room, one record per call and instance: pose err^2, pose NEES, mean landmark err^2, mean
 *             landmark NEES over this call's valid landmarks; NaN where there is none. */
int cslam_ekf_batch_score(cslam_ekf_batch_t h, const float* xv_true /* host [3] */);
/* Launches what is queued, synchronises, and copies the totals [instances][CSLAM_SCORE_FIELDS] and up to
 * capacity_records series records [records][instances][4] (the read-out that replaces a get_poses / get_landmarks pair
 * per step: test/main.cpp:136, EKF.cpp:131-144).  *records = min(calls, series_capacity) is the number of records held
 * (at most capacity_records of them are copied), *calls counts every score call since the reset (calls beyond the
 * series capacity still enter the totals).  Any output pointer may be NULL. */
int cslam_ekf_batch_get_scores(cslam_ekf_batch_t h, double* totals /* [I][CSLAM_SCORE_FIELDS] */,
                               float* series /* [records][I][4] */, int capacity_records, int* records, long long* calls);

/* ---- the same score for the single handle, f32 and f64 (ekf_score_landmarks / ekf_score_finish in
 *      conan_slam_amd/csrc/ekf_score_kernels.hpp), with a trajectory log.  A consistency study of one filter otherwise
 *      reads cslam_ekf_get_landmarks and cslam_ekf_get_pose after every step (a synchronise each) or cslam_ekf_trace /
 *      cslam_ekf_get_state (which apply the pending columns early and so change the rounding of every later step).  These
 *      calls read X, the pose stripe and the deferred form P = Ps - Wp diag(s) Wp^T as they stand -- the sign words of
 *      heading columns stored with S < 0 included -- and never write the filter's state.  The rules, the gates, the f64
 *      arithmetic, the fixed summation order and the CSLAM_SCORE_* indices are those of cslam_ekf_batch_score with one
 *      instance; the truth rows and the true pose are doubles for both dtypes, as for cslam_pf_score. */
/* Zeroes the totals, the series, the track and the call count (scoring state a study keeps on the host beside
 * test/main.cpp:136; the blocks of EKF.cpp:131-144; per step of slam.h:841-847).  series_capacity >= 0 records of 4
 * floats and 5 doubles (0: totals only).  A gate <= 0 selects the 95 % chi-square point: 7.8147 for the pose, 5.9915 for a
 * landmark.  The truth rows are kept.  A score call without a prior reset behaves as after score_reset(h, 0, 0, 0).  A
 * negative capacity: CSLAM_ERR_BAD_ARG, nothing changed.  A handle that never calls a score function allocates nothing
 * for it; cslam_ekf_set_state leaves the score state alone. */
int cslam_ekf_score_reset(cslam_ekf_t h, int series_capacity, double gate_pose, double gate_lm);
/* The true position of state feature j + 1 is row j of lm_true (host [count][2] doubles; the features of
 * EKF.cpp:131-144, scored beside the pose of test/main.cpp:136 after a step of slam.h:841-847), copied into a device
 * buffer sized for max_landmarks before the call returns.  Features beyond `count` are not scored.  count < 0 or
 * count > max_landmarks: CSLAM_ERR_BAD_ARG, nothing changed. */
int cslam_ekf_score_set_truth(cslam_ekf_t h, const double* lm_true /* host [count][2] */, int count);
/* One score step against the true pose xv_true (host [3], finite; it travels as kernel arguments; the pose of
 * test/main.cpp:136, the blocks of EKF.cpp:131-144, after the step of slam.h:841-847).  Launches what is queued exactly as
 * cslam_ekf_get_landmarks does -- a held predict, the pose queue, a queued look-ahead update as a window of one; a call
 * at a window boundary finds nothing queued -- waits on the stream (not the host) for a P-GEMM in flight, then queues the
 * two score kernels on the main stream and returns: no covariance downdate, no synchronise, no copy, and after the first
 * call no allocation.  The run continues bit for bit as without the call.
 *   totals    the pose and c = min(N, truth count) landmarks, by the pose, landmark and series rules written at
 *             cslam_ekf_batch_score above.  with_map == 0: the landmark kernel is not launched, the landmark totals are
 *             untouched and series fields 2 and 3 are NaN.
 *   track     while there is room, one record of 5 doubles per call: X[0], X[1], X[2] widened bit for bit, trace(P) --
 *             the pose diagonal from the stripe plus p00 + p11 of EVERY landmark of the state from the deferred form,
 *             summed in f64 in a fixed order; NaN when with_map == 0 -- and n.
 * A NULL or non-finite xv_true: CSLAM_ERR_BAD_ARG, nothing changed. */
int cslam_ekf_score(cslam_ekf_t h, const double* xv_true /* host [3] */, int with_map);
/* The one synchronising call of the score: copies the totals [CSLAM_SCORE_FIELDS], up to capacity_records series records
 * [records][4] and track records [records][5] on the main stream and waits for it (the read-out that replaces a get_pose
 * / get_landmarks pair per step: test/main.cpp:136, EKF.cpp:131-144, slam.h:841-847).  It applies no pending column and
 * launches nothing that is queued -- a held predict and a queued look-ahead update stay queued -- so the rest of the run
 * does not depend on where the scores are read.  *records = min(calls, series_capacity) is the number of records held (at
 * most capacity_records of them are copied), *calls counts every score call since the reset.  Any output pointer may be
 * NULL; a negative capacity_records: CSLAM_ERR_BAD_ARG. */
int cslam_ekf_get_scores(cslam_ekf_t h, double* totals /* [CSLAM_SCORE_FIELDS] */, float* series /* [records][4] */,
                         double* track /* [records][5] */, int capacity_records, int* records, long long* calls);
/* Slam::observeHeading (slam.h:788, EKF.cpp:328-352, josephUpdate slam.h:700-725) on every instance.  phi is common,
 * as in the reference driver, which observes the true heading.  Deliberate difference from the single handle: an
 * instance whose S = P22 + R is <= 0 or non-finite (an indefinite P; a healthy filter never has one) skips the heading
 * half of the step -- a predict in the same step still applies, X and P are otherwise unchanged -- and raises
 * CSLAM_FACTOR_HEADING_SKIPPED in its flag word (sticky).  The other instances are unaffected. */
int cslam_ekf_batch_observe_heading(cslam_ekf_batch_t h, double phi, int use_heading);
/* Slam::update(..., batch = true) (slam.h:938-943, EKF.cpp:93-129) on every instance.  dZ[i] / d_idf[i] are instance
 * i's device-resident 2 x m observations and m feature indices; 1 <= m <= 32 (m = 0 is a no-op; m <= 8, k = 2m <= 16,
 * runs the factor chain's k <= 16 form).  A held predict_each is launched first as a predict-only step (see below). */
int cslam_ekf_batch_update(cslam_ekf_batch_t h, const float* const* dZ, const int* const* d_idf, int m, const float* R);
/* Slam::augment (slam.h:190-191, EKF.cpp:9-91) on every instance.  dZn[i] holds instance i's 2 x q new-feature
 * observations (device).  q is common to all instances, so n stays common.  CSLAM_ERR_CAPACITY beyond max_landmarks,
 * with nothing changed. */
int cslam_ekf_batch_augment(cslam_ekf_batch_t h, const float* const* dZn, int q, const float* R);

/* Per-stage device times of update() measured with HIP events on the handle's streams.
 * on = 1 starts recording (events around every stage of every update), on = 2 brackets the covariance downdate
 * (P-GEMM) launches only, on = 3 one downdate launch in sixteen, on = 4 one in four (an event pair costs ~11 us of
 * stream time), on = 0 stops.
 * get: synchronises, writes the SUM of milliseconds per stage since profiling was switched on and the
 * number of launches per stage. */
int cslam_ekf_set_profiling(cslam_ekf_t h, int on);
int cslam_ekf_get_stage_times(cslam_ekf_t h, double* ms_sum, int* launches);

/* Introspection for tests: copy the update intermediates of the LAST batch update to the host.
 * PHT and W1 are n x k (leading dimension n on output), S and G are k x k, V and t have k entries.
 * Any pointer may be NULL. Synchronises. */
int cslam_ekf_debug_last_update(cslam_ekf_t h, void* PHT, void* S, void* G, void* W1, void* V, int* k);

/* ================================ FastSLAM-2 particle set ==================================== */
typedef struct cslam_pf* cslam_pf_t;

/* Replaces PF::initializeParticles(numParticles)  -- slam.h:688, PF.cpp:319-341, for the
 * n_particles this process owns (one shard of the global set; see INTEGRATION.md for the sharding).
 * Layout is structure-of-arrays in HBM. */
int cslam_pf_create(int n_particles, int max_features, int dtype, int device, int quirks, cslam_pf_t* out);
int cslam_pf_destroy(cslam_pf_t h);
int cslam_pf_synchronize(cslam_pf_t h);
int cslam_pf_get_counts(cslam_pf_t h, int* n_particles, int* n_features);
/* The stream every call of this handle is ordered on (a hipStream_t).  The handle owns it and destroys it with
 * cslam_pf_destroy.  A caller MAY record events on it (timing around calls), make other streams wait for such events,
 * and synchronise it.  A caller MUST NOT enqueue kernels or copies on it that touch the handle's buffers, capture it
 * into a graph, or destroy it. */
int cslam_pf_get_stream(cslam_pf_t h, void** stream);

/* set every particle's weight to w0 (PF.cpp:327 uses 1/N of the GLOBAL particle count) */
int cslam_pf_set_uniform_weight(cslam_pf_t h, double w0);

/* Replaces PF::predict(particle, v, swa, Q, wb, dt) for every owned particle -- slam.h:858-863,
 * PF.cpp:419-471. */
int cslam_pf_predict(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt);

/* Replaces PF::observeHeading(particle, phi, use) for every owned particle -- PF.cpp:382-417. */
int cslam_pf_observe_heading(cslam_pf_t h, double phi, int use_heading);

/* Replaces PF::sampleProposal(particle, Z, idf, R) for every owned particle -- slam.h:881-884,
 * PF.cpp:502-544 (computeJacobians PF.cpp:70-135, likelihood 343-359, gaussEvaluate 279-317).
 * normals: 3 * n_particles scalars (host), the N(0,1) draws slam.h:753-764 would make, COMPONENT-major:
 * normals[e * n_particles + p] is draw e (0..2) of particle p (i.e. an n_particles x 3 column-major matrix).
 * Like every per-particle call of this section, it consumes its host arrays before it returns but does
 * not wait for the device: the work is ordered on the handle's stream, and cslam_pf_synchronize() (or
 * any call that returns data to the host) waits for it. */
int cslam_pf_sample_proposal(cslam_pf_t h, const void* Z, int m, const int* idf, const void* R,
                             const void* normals);

/* Replaces PF::featureUpdate(particle, Z, idf, R) for every owned particle -- slam.h:549-552,
 * PF.cpp:222-277. */
int cslam_pf_feature_update(cslam_pf_t h, const void* Z, int m, const int* idf, const void* R);

/* Replaces PF::addOneNewFeature(particle, Z, R) for every owned particle -- slam.h:134, PF.cpp:9-60. */
int cslam_pf_add_features(cslam_pf_t h, const void* Z, int q, const void* R);

/* ---- observations whose correspondence is unknown: every particle carries its own association hypothesis ----
 * Gated nearest-neighbour association of m observations against the map of EVERY owned particle: the measure of
 * EKF::computeAssociation and the rule of dataAssociate (EKF.cpp:131-144, 235-326) on the particle's own state, whose
 * covariance is blockdiag(Pv, PF_f): S = HV Pv HV^T + HF PF_f HF^T + R (all four entries of R are read),
 * nis = v^T S^-1 v, nd = nis + log det S.  For particle p and observation j: kind 1 and idf = the lowest-index feature
 * with the smallest nd among those with nis < gate1; else idf 0 and kind 2 when the smallest nis exceeds gate2 (a new
 * feature), kind 0 otherwise (ambiguous).  Comparisons are strict; a NaN takes part in none; an empty map gives kind 2.
 * Afterwards no two observations of one particle hold the same feature: the smallest nd keeps it (the lower observation
 * index on equal nd), the others become idf 0 / kind 0.  Fills the handle's device tables idf[m][np], kind[m][np]
 * (particle index fastest) and summary[m][4] = (sum of w over the particles of kind 1, of kind 2, of kind 0, number of
 * particles of kind 1), sums in double over THIS handle's particles (a sharded caller adds the shards' summaries).
 * Asynchronous like the other per-particle calls; returns nothing to the host. */
int cslam_pf_associate(cslam_pf_t h, const void* Z, int m, const void* R, double gate1, double gate2);
/* The tables of the last cslam_pf_associate (EKF.cpp:131-144, 235-326): idf_host and kind_host m * n_particles ints,
 * summary_host m * 4 doubles; any of the three may be NULL.  Synchronises. */
int cslam_pf_get_association(cslam_pf_t h, int* idf_host, int* kind_host, double* summary_host);
/* PF::sampleProposal with PF::featureUpdate at the sampled pose (PF.cpp:502-544, 222-277) where particle p takes the
 * correspondence of observation j from the table of the last cslam_pf_associate (EKF.cpp:131-144, 235-326).  Z and m
 * must be those of that call, and the particles must not have changed slots in between (resample, gather, unpack,
 * set_particle, observation_step): the table is indexed by particle slot.  Either violation is CSLAM_ERR_BAD_ARG.
 * use: m ints (host), 0 or 1.  use[j] = 0: no particle sees observation j (the caller adds it as a new feature).
 * use[j] = 1 and idf != 0: the arithmetic of cslam_pf_sample_proposal + cslam_pf_feature_update in their order.
 * use[j] = 1 and idf == 0: no pose or feature update; the particle's likelihood product takes the factor
 * miss_likelihood (FastSLAM's new-feature likelihood) at observation j's place. */
int cslam_pf_sample_proposal_assoc(cslam_pf_t h, const void* Z, int m, const void* R, const void* normals, const int* use,
                                   double miss_likelihood);
/* PF::featureUpdate alone (PF.cpp:222-277) from the table of the last cslam_pf_associate (EKF.cpp:131-144, 235-326) and
 * the same mask: the unfused form, for a caller that has moved the poses with cslam_pf_sample_proposal itself. */
int cslam_pf_feature_update_assoc(cslam_pf_t h, const void* Z, int m, const void* R, const int* use);

/* ---- the resample step (PF.cpp:473-500, 546-577), split so that a multi-GPU driver can put its
 *      collectives between the pieces; see INTEGRATION.md ---- */
/* local partial sums: sums[0] = sum w, sums[1] = sum w^2 (doubles, host). Synchronises. */
int cslam_pf_weight_sums(cslam_pf_t h, double* sums);
/* w *= scale (the 1/ws of PF.cpp:482-487 with ws the GLOBAL sum) */
int cslam_pf_scale_weights(cslam_pf_t h, double scale);
/* w = w / ws, each quotient rounded once to the particle dtype.  The normalisation at the ends of the range: a driver
 * scales by 1/ws as long as that scale, rounded to the particle dtype, is a NORMAL number (ws in (2^-128, 2^126] for
 * f32, (2^-1024, 2^1022] for f64) and divides otherwise -- below, the scale overflows; above, it is subnormal and
 * short of bits.  cslam_pf_resample_local and cslam_pf_resample_sharded apply this rule themselves. */
int cslam_pf_divide_weights(cslam_pf_t h, double ws);
/* What the resample calls of this handle do with a weight sum that is not a positive finite number (DEGENERATE SUMS at
 * cslam_pf_resample_local).  CSLAM_PF_REPORT: the rule.  CSLAM_PF_REPAIR: what the engine did before the rule existed and
 * a KNOWN DEFECT -- Neff comes out as 0, the call resamples, no stratum lies below a NaN running sum, so every slot becomes
 * a copy of particle 0 and the weights are reset to 1/N: the degeneracy is erased.  REPAIR is still what a new handle
 * starts with, because a filter that runs two observation steps in a row without anything that restores Pv between them
 * (PF.cpp:537 zeroes it, the next predict leaves it singular) has NaN weights from its second step and runs on only
 * through that repair; the default becomes REPORT once such drivers are gone.  Every rank of a sharded set must use the
 * same policy. */
#define CSLAM_PF_REPAIR 0
#define CSLAM_PF_REPORT 1
int cslam_pf_set_degenerate_policy(cslam_pf_t h, int policy);
/* device pointer to the owned weights (n_particles scalars) for an all-gather */
int cslam_pf_weights_device_ptr(cslam_pf_t h, void** dptr);
int cslam_pf_get_weights(cslam_pf_t h, void* w_host); /* synchronises */
int cslam_pf_set_weights(cslam_pf_t h, const void* w_host);
/* size in bytes of one packed particle record (w, Xv, Pv, XF, PF for max_features) */
int cslam_pf_record_bytes(cslam_pf_t h, long long* bytes);
/* pack the particles src_idx[0..count) (local 0-based indices, host array) into the device buffer
 * d_records (count * record_bytes), e.g. a send buffer of the all-to-all-v */
int cslam_pf_pack(cslam_pf_t h, const int* src_idx, int count, void* d_records);
/* overwrite local slots dst_idx[0..count) from packed records in device memory */
int cslam_pf_unpack(cslam_pf_t h, const int* dst_idx, int count, const void* d_records);
/* purely local resample: slot i <- copy of local particle keep[i] (0-based), all weights = w_new */
/* PF::resampleParticles (PF.cpp:473-500) with stratifiedResample (PF.cpp:546-574) when ONE handle holds the whole
 * particle set: weight sums, normalisation, Neff, the decision (Neff < n_effective && resample_status), keep[] and
 * the particle moves all run on the device; `select` are the N strata positions (PF.cpp:557, host pointer).
 * neff / resampled may be NULL (then nothing returns to the host). Same results as weight_sums + scale_weights +
 * host keep[] + gather_local.  Any particle count (the running sum is sequential, as in the reference: 8192 weights
 * are staged in LDS at a time).
 * THE RANGE OF THE SUM: sum w is formed in double, and every positive finite sum normalises correctly, subnormal sums
 * and sums beyond the particle dtype's largest number included (see cslam_pf_divide_weights); in f64, where the squares
 * of the weights leave the range of double, Neff is formed from the normalised weights.  The same holds for
 * cslam_pf_observation_step, cslam_pf_resample_sharded and the drawn forms.
 * DEGENERATE SUMS: when sum w is NOT a positive finite number -- 0 after total underflow, a NaN or +inf weight in the
 * set -- the rule is the reference's arithmetic (PF.cpp:482-490): the weights become the IEEE quotients w / sum w (NaN,
 * or 0 under an infinite sum), Neff is NaN, NOTHING is resampled whatever n_effective is, *resampled = 0, and every pose,
 * covariance and feature is left as it was.  The degeneracy is reported, not repaired: cslam_pf_resample_stats counts
 * the call and no resample with a NaN last Neff, cslam_pf_estimate returns NaN moments afterwards and cslam_pf_score
 * counts POSE_BAD.  A handle follows the rule after cslam_pf_set_degenerate_policy(h, CSLAM_PF_REPORT). */
int cslam_pf_resample_local(cslam_pf_t h, const void* select, double n_effective, int resample_status, double* neff,
                            int* resampled);
int cslam_pf_gather_local(cslam_pf_t h, const int* keep, double w_new);
/* One whole observation step of the reference's FastSLAM-2 loop (test/main.cpp:279-311) for a handle that holds every
 * particle: PF::predict (PF.cpp:419-471), PF::sampleProposal (PF.cpp:502-544), PF::featureUpdate (PF.cpp:222-277) and
 * PF::resampleParticles (PF.cpp:473-500), same arguments as the individual calls, with ONE staged host-to-device copy
 * for all the small inputs and nothing returned to the host (cslam_pf_resample_stats reports what happened). */
int cslam_pf_observation_step(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt, const void* Z, int m,
                              const int* idf, const void* R, const void* normals, const void* select, double n_effective,
                              int resample_status);
/* resample calls / resamples performed since the handle was created and the last Neff (device-side counters of
 * cslam_pf_resample_local and cslam_pf_observation_step; any pointer may be NULL).  Synchronises. */
int cslam_pf_resample_stats(cslam_pf_t h, double* calls, double* resamples, double* last_neff);

/* ---- the resample step over a particle set SHARDED across GPUs, one process (rank) per GPU:
 * PF::resampleParticles (slam.h:871-872, PF.cpp:473-500) with stratifiedResample (PF.cpp:546-574) where every rank
 * holds n_particles of the world * n_particles particles (block partition: global slot g lives on rank g / n_particles).
 * The collectives run over RCCL (xGMI inside a node) on the handle's stream:
 *     1. all-gather of the weights; every rank forms [sum w, sum w^2] over the whole set with the reduction of the
 *        one-shard call -> normalisation and Neff, identical on every rank AND bit for bit those of
 *        cslam_pf_resample_local on the whole set, whatever the number of ranks
 *     2. only when it resamples: every rank derives the identical keep[] on its own device from the gathered weights
 *        and the shared strata positions
 *     3. one grouped send/recv of the packed particle records whose source rank differs from the destination rank
 * `select`: the world * n_particles strata positions of PF.cpp:557 (host pointer), identical on every rank.
 * neff / resampled may be NULL.  The range of the sum and DEGENERATE SUMS: as stated at cslam_pf_resample_local (every
 * rank sees the same sum and, under one policy, decides alike: Neff = NaN and no rank resamples under CSLAM_PF_REPORT).  The librccl of the process is bound at run time (dlopen): there is no link-time
 * dependency, and a process that never shards never loads it.
 * A communicator is made the RCCL way: rank 0 calls cslam_comm_unique_id, distributes the CSLAM_COMM_ID_BYTES bytes by
 * whatever means the application has (MPI_Bcast, a file, torch.distributed), every rank calls cslam_comm_create. */
typedef struct cslam_comm* cslam_comm_t;
#define CSLAM_COMM_ID_BYTES 128
int cslam_comm_unique_id(void* id_bytes);
int cslam_comm_create(const void* id_bytes, int rank, int world, int device, cslam_comm_t* out);
int cslam_comm_destroy(cslam_comm_t c);
int cslam_comm_info(cslam_comm_t c, int* rank, int* world); /* either pointer may be NULL */
/* A LOOPBACK communicator: `world` (<= 16) ranks inside ONE process on ONE device, out[0..world) their handles.  RCCL
 * refuses the same device twice in one communicator, so this is how the multi-rank paths of cslam_pf_resample_sharded
 * (ranks > 0, the exchange plan, the receive ordering by source rank) run on a one-GPU box: all-reduce, all-gather and
 * the grouped send/recv become device-to-device copies ordered by a host barrier.  Every rank's
 * cslam_pf_resample_sharded must be called from its OWN host thread (the ranks meet inside the call, as processes do
 * over RCCL); a rank that fails or does not arrive within 60 s breaks the communicator for all.  For tests and for
 * sharding one GPU's particle set by hand -- not a fast path. */
int cslam_comm_create_loopback(int world, int device, cslam_comm_t* out);
int cslam_pf_resample_sharded(cslam_pf_t h, cslam_comm_t comm, const void* select, double n_effective,
                              int resample_status, double* neff, int* resampled);
/* Introspection for tests: the exchange plan of the LAST cslam_pf_resample_sharded on this handle.  counts: 2 * world
 * ints -- records sent to each destination rank, then records received from each source rank (all 0 when it did not
 * resample); send_idx: the local source indices in send order (capacity >= *n_send).  Any pointer may be NULL. */
int cslam_pf_debug_last_exchange(cslam_pf_t h, int* counts, int* send_idx, int capacity, int* n_send);

/* ---- the random inputs drawn on the device.  The reference draws them on the host from generators it seeds from the
 * clock (slam.h:587-594): the three standard normals per particle of multivariateGauss (slam.h:753-764) that
 * PF::sampleProposal consumes, and the strata positions of stratifiedRandom (PF.cpp:557, PF.cpp:579-596) that
 * PF::resampleParticles consumes.  The calls above take them as host arrays (`normals`, `select`); the _drawn calls below
 * take a step number instead and draw them on the device from the counter-based generator of conan_slam_amd/synth.py:
 *     key(step, e, g) = ((step * 4 + e) << 32) | g   (uint64, wrapping; g = GLOBAL particle slot, e = stream)
 *     normals[e][p]   = T(normal(seed, key(step, e, first_global + p)))                e = 0, 1, 2
 *     select          = stratified_random(n_global, u),  u[i] = uniform01(seed, 2 * key(step, 3, i))
 * (synth.pf_draw_normals / synth.pf_draw_select; select comes out bit for bit, the normals to the device's log / cos).
 * A draw depends on (seed, step, global slot) only: ranks that hold 8 x 64 particles and one handle that holds 512 see
 * the same noise, and nobody distributes select.  One producer kernel writes the draws where the staged copy of the
 * host-array call would have put them, and the same consumer kernels follow with the same arguments; with m <= 32 the
 * observations travel as that kernel's arguments and the call enqueues no copy command at all.
 *
 * cslam_pf_seed_draws   the seed (slam.h:587-594), the global slot of this handle's particle 0 and the size of the whole
 *                       set: 0 <= first_global, first_global + n_particles <= n_global < 2^32.  May be called again.
 *                       The strata (select) exist for n_global <= 2^31 - 1, which is all a resample can hold; a larger
 *                       set draws normals only, and cslam_pf_get_draws refuses its select.
 *                       Seeding changes nothing about any call that takes host arrays.
 * cslam_pf_get_draws    what the _drawn calls of `step` consume: normals 3 * n_particles (component-major, as
 *                       cslam_pf_sample_proposal takes them; slam.h:753-764) and select n_global (PF.cpp:557); either may
 *                       be NULL.  Synchronises; touches neither the particles nor the staging area.
 * Every _drawn call returns CSLAM_ERR_BAD_ARG on an unseeded handle and changes nothing; otherwise it validates and
 * behaves as its host-array twin (cslam_pf_sample_proposal: PF.cpp:502-544, cslam_pf_sample_proposal_assoc,
 * cslam_pf_resample_local / _sharded: PF.cpp:473-500, cslam_pf_observation_step).  The proposal uses streams 0..2 of
 * `step`, the resample stream 3: cslam_pf_sample_proposal_drawn(step) + cslam_pf_feature_update +
 * cslam_pf_resample_local_drawn(step) behind cslam_pf_predict is cslam_pf_observation_step_drawn(step).
 * cslam_pf_resample_local_drawn and cslam_pf_observation_step_drawn need first_global = 0 and n_global = n_particles;
 * cslam_pf_resample_sharded_drawn needs n_global = world * n_particles and first_global = rank * n_particles.
 * cslam_pf_stage_copies  introspection: host-to-device copy commands this handle has enqueued for per-step inputs (the
 *                       staged copies of Z / idf / normals / select), so that a test can hold "no copy". */
int cslam_pf_seed_draws(cslam_pf_t h, long long seed, long long first_global, long long n_global);
int cslam_pf_get_draws(cslam_pf_t h, long long step, void* normals /* 3*np or NULL */, void* select /* n_global or NULL */);
int cslam_pf_sample_proposal_drawn(cslam_pf_t h, const void* Z, int m, const int* idf, const void* R, long long step);
int cslam_pf_sample_proposal_assoc_drawn(cslam_pf_t h, const void* Z, int m, const void* R, const int* use,
                                         double miss_likelihood, long long step);
int cslam_pf_resample_local_drawn(cslam_pf_t h, long long step, double n_effective, int resample_status, double* neff,
                                  int* resampled);
int cslam_pf_resample_sharded_drawn(cslam_pf_t h, cslam_comm_t comm, long long step, double n_effective,
                                    int resample_status, double* neff, int* resampled);
int cslam_pf_observation_step_drawn(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt, const void* Z,
                                    int m, const int* idf, const void* R, long long step, double n_effective,
                                    int resample_status);
int cslam_pf_stage_copies(cslam_pf_t h, long long* copies);

/* ---- the scan that observes ONLY new features (test/main.cpp:314-328; from X = 0, P = 0 the first scan of every run).
 * The reference then draws every particle's pose from its own Gaussian, X <- X + chol(P) z
 * (multivariateNormalGaussianDistribution, slam.h:753-764, with choleskyDecomposition, slam.h:413-436: the Jacobi
 * factor V sqrt(lambda) where the LLT fails, a zero factor where that is not finite -- such a particle keeps its pose),
 * sets P <- 0 and initialises the new features at the SAMPLED pose (PF::addOneNewFeature, PF.cpp:9-60).  The weights
 * are not touched.
 *
 * cslam_pf_sample_pose        replaces test/main.cpp:321-324 for every owned particle (slam.h:753-764, slam.h:413-436).
 *                             normals: 3 * n_particles scalars (host), component-major as cslam_pf_sample_proposal
 *                             takes them.
 * cslam_pf_new_feature_step   replaces the whole branch test/main.cpp:314-328 in ONE launch: PF::predict
 *                             (PF.cpp:419-471) when Q is not NULL, the pose sample (slam.h:753-764, slam.h:413-436),
 *                             P <- 0, and PF::addOneNewFeature (PF.cpp:9-60) of the q observations Z (2 x q) at the
 *                             sampled pose.  Q = NULL: no predict (v, swa, wb, dt are ignored); the poses and Pv then
 *                             come out bit for bit as cslam_pf_sample_pose leaves them, and the features as
 *                             cslam_pf_add_features computes them behind it (to rounding: another kernel).
 *                             q = 0 does exactly what [cslam_pf_predict +] cslam_pf_sample_pose does.
 * The _drawn forms take the normals of `step` from the device-side draws (streams e = 0..2, see above; a scan takes
 * either the proposal or this branch, so the two never both draw at one step): they need cslam_pf_seed_draws, work on
 * ANY shard (first_global arbitrary: there is no collective in this branch), enqueue no copy command up to 32 new
 * observations, and cslam_pf_get_draws(step) returns exactly the normals they consume.
 * All four are asynchronous on the handle's stream and consume their host arrays before they return.
 * q < 0, NULL normals, or q > 0 with a NULL Z or R: CSLAM_ERR_BAD_ARG; an unseeded handle in a _drawn form:
 * CSLAM_ERR_BAD_ARG; nf + q > max_features: CSLAM_ERR_CAPACITY.  A refused call changes nothing: not the store, not the
 * feature count, not the staging area, not the association tables.  On success the feature count grows by q.
 * The tables of cslam_pf_associate are treated as cslam_pf_predict and cslam_pf_add_features treat them: poses and the
 * feature count change, particles keep their slots, so the tables stay valid for their consumers. */
int cslam_pf_sample_pose(cslam_pf_t h, const void* normals /* 3*np, component-major */);
int cslam_pf_sample_pose_drawn(cslam_pf_t h, long long step);
int cslam_pf_new_feature_step(cslam_pf_t h, double v, double swa, const void* Q /* NULL: no predict */, double wb, double dt,
                              const void* Z, int q, const void* R, const void* normals);
int cslam_pf_new_feature_step_drawn(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt, const void* Z,
                                    int q, const void* R, long long step);

/* ---- the vote on new features, on the device: the scan with unknown correspondences without a host decision ----
 * cslam_pf_associate gives every particle its own correspondences (EKF.cpp:131-144, 235-326); WHICH observations become
 * new features is one decision for the whole set, because the feature index space is shared (the split that
 * test/main.cpp:279-328 takes from its table).  Observation j is NEW when, with summary[j] = (s0, s1, s2, .) of the last
 * associate and total = (s0 + s1) + s2 in double, in this order:  total > 0, s1 > 0 and s1 >= new_fraction * total.
 *
 * cslam_pf_associate_vote          cslam_pf_associate (EKF.cpp:131-144, 235-326), then the vote on this handle's summary:
 *                                  in HBM use[j] = new ? 0 : 1, the new observations compacted in observation order
 *                                  (new_idx[k] = j, ZN column k = Z column j) and their count q; one device-to-host copy
 *                                  of [q, m, use[m]] into a pinned block and an event behind it.  Asynchronous.  A
 *                                  non-finite new_fraction: CSLAM_ERR_BAD_ARG, nothing changes.  m = 0 launches nothing
 *                                  and is a vote with q = 0.
 * cslam_pf_associate_vote_sharded  the same (EKF.cpp:131-144, 235-326 on every rank's shard) with the vote read from the
 *                                  SUM over the ranks of the shards' summaries (one all-reduce of 4 m doubles; the
 *                                  loopback communicator adds in rank order): every rank ends with identical use, ZN and
 *                                  q.  cslam_pf_get_association still returns the shard's own summary.  Everything that
 *                                  can fail locally comes before the collective, as in cslam_pf_resample_sharded.
 * A vote belongs to the last associate: a later cslam_pf_associate drops it, a later cslam_pf_associate_vote replaces it.
 * cslam_pf_vote_wait               waits for the vote's event only -- not for work queued behind it -- and returns q and
 *                                  (use != NULL) the m flags from the pinned block.  May be called more than once per
 *                                  vote.  No live vote: CSLAM_ERR_BAD_ARG.
 * cslam_pf_get_vote                for tests and reporting; synchronises.  use m ints, new_idx q ints, ZN 2 * q scalars of
 *                                  the handle's dtype (room for m / m / 2 * m serves any vote), any output may be NULL.
 *                                  Entries from q on are not written.
 * cslam_pf_sample_proposal_voted, _voted_drawn (PF.cpp:502-544 + 222-277), cslam_pf_feature_update_voted (PF.cpp:222-277)
 *                                  cslam_pf_sample_proposal_assoc, _assoc_drawn and cslam_pf_feature_update_assoc with the
 *                                  mask read from the vote's use[] on the device: the same kernels, no mask staged.  They
 *                                  need a live vote and what the _assoc calls need: Z and m of that associate, particles
 *                                  in the slots they had then (a resample since: CSLAM_ERR_BAD_ARG, "moved"), a map that
 *                                  has not shrunk.
 * cslam_pf_add_features_voted      PF::addOneNewFeature (PF.cpp:9-60) of the q voted observations, read from the vote's
 *                                  ZN: waits for the vote's event if nobody has, then one launch, and the feature count
 *                                  grows by q (*q_out = q, may be NULL).  Allowed after a resample (ZN is per observation,
 *                                  not per slot).  q = 0 launches nothing.  A vote is added at most once: a second call
 *                                  is CSLAM_ERR_BAD_ARG.  nf + q > max_features: CSLAM_ERR_CAPACITY with *q_out = q,
 *                                  nothing changes and the vote stays as it was.
 * cslam_pf_assoc_scan_step_drawn   one scan of test/main.cpp:279-328 with unknown correspondences in ONE call, for a
 *                                  handle that holds the whole set (the preconditions of cslam_pf_resample_local_drawn):
 *                                  cslam_pf_predict (PF.cpp:419-471), cslam_pf_associate_vote,
 *                                  cslam_pf_sample_proposal_voted_drawn(step), cslam_pf_resample_local_drawn(step) with
 *                                  nothing returned (PF.cpp:473-500), and only then the wait for the vote and
 *                                  cslam_pf_add_features_voted: the host blocks on the vote's event alone, with the
 *                                  proposal and the resample already queued.  m = 0 is the predict alone (*q_out = 0, a
 *                                  live vote is left as it is).  On CSLAM_ERR_CAPACITY the predict, the proposal and the
 *                                  resample HAVE been applied and no feature was added -- the state the separate calls
 *                                  leave; the vote can still be added after room has been made.  A scan in which every
 *                                  observation is new takes this path too (the poses are not sampled as
 *                                  cslam_pf_new_feature_step samples them: q is not known when the proposal is queued). */
int cslam_pf_associate_vote(cslam_pf_t h, const void* Z, int m, const void* R, double gate1, double gate2,
                            double new_fraction);
int cslam_pf_associate_vote_sharded(cslam_pf_t h, cslam_comm_t comm, const void* Z, int m, const void* R, double gate1,
                                    double gate2, double new_fraction);
int cslam_pf_vote_wait(cslam_pf_t h, int* q, int* use /* m or NULL */);
int cslam_pf_get_vote(cslam_pf_t h, int* use, int* new_idx, void* ZN, int* q);
int cslam_pf_sample_proposal_voted(cslam_pf_t h, const void* Z, int m, const void* R, const void* normals,
                                   double miss_likelihood);
int cslam_pf_sample_proposal_voted_drawn(cslam_pf_t h, const void* Z, int m, const void* R, double miss_likelihood,
                                         long long step);
int cslam_pf_feature_update_voted(cslam_pf_t h, const void* Z, int m, const void* R);
int cslam_pf_add_features_voted(cslam_pf_t h, const void* R, int* q_out);
int cslam_pf_assoc_scan_step_drawn(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt, const void* Z,
                                   int m, const void* R, double gate1, double gate2, double new_fraction,
                                   double miss_likelihood, long long step, double n_effective, int resample_status,
                                   int* q_out);

/* ---- a run of control steps in one launch, and whole-cycle calls ----
 * Between two scans the reference's particle loop (test/main.cpp:249-334) runs about six control steps
 * (mDtObserve = 5.058 mDtControls, slam.h:69-77), each of them PF::predict then PF::observeHeading for every particle
 * (test/main.cpp:279-286); mSwitchHeadingKnown is true by default (slam.h:99).
 *
 * cslam_pf_control_run       replaces k iterations of test/main.cpp:279-286 for every owned particle: bit for bit the
 *                            result of k x (cslam_pf_predict(v[j], swa[j], Q, wb, dt) -- PF.cpp:419-471;
 *                            cslam_pf_observe_heading(phi[j], use_heading) -- PF.cpp:382-417, slam.h:700-725), with ONE
 *                            launch per 16 steps (the chunks of a longer run are queued back to back) and the pose state
 *                            loaded and stored once per launch.  v, swa, phi: k host doubles each, cast to the handle's
 *                            dtype as the single calls cast theirs; phi may be NULL when use_heading = 0.  Works on any
 *                            shard, needs no draws, is asynchronous as cslam_pf_predict is, and leaves the staging area,
 *                            the association tables and the vote exactly as cslam_pf_predict leaves them.  k = 0 returns
 *                            CSLAM_OK and launches nothing.  k < 0, a NULL v, swa or Q with k > 0, or a NULL phi with
 *                            k > 0 and use_heading != 0: CSLAM_ERR_BAD_ARG, nothing changes.
 * cslam_pf_control_launches  introspection: control-run kernel launches of this handle so far (a host-side counter), so
 *                            that a test can hold "one launch per 16 steps".
 * cslam_pf_cycle_drawn       one whole iteration block of test/main.cpp:249-334 with known correspondences, for a handle
 *                            that holds the whole seeded set (the preconditions of cslam_pf_resample_local_drawn): the
 *                            control run of ALL k steps (test/main.cpp:279-286), then the scan of test/main.cpp:294-328
 *                            without a predict of its own.  mf > 0: bit for bit cslam_pf_sample_proposal_drawn(ZF, mf,
 *                            idf, R, step) (PF.cpp:502-544), cslam_pf_feature_update(ZF, mf, idf, R) (PF.cpp:222-277),
 *                            cslam_pf_resample_local_drawn(step) with nothing returned (PF.cpp:473-500), then
 *                            cslam_pf_add_features(ZN, mn, R) (PF.cpp:9-60).  mf = 0 and mn > 0:
 *                            cslam_pf_new_feature_step_drawn(ZN, mn, R, step) with Q = NULL (test/main.cpp:314-328; any
 *                            shard of a seeded set will do).  mf = mn = 0: the control run alone.  With mf <= 32 and
 *                            mn <= 32 the call enqueues no copy command (cslam_pf_stage_copies does not move).
 *                            Everything that can refuse is checked BEFORE the control run is launched -- what
 *                            cslam_pf_control_run refuses, an unseeded handle or a shard of a larger set, idf outside
 *                            1..nf, NULL arrays: CSLAM_ERR_BAD_ARG; nf + mn > max_features: CSLAM_ERR_CAPACITY -- and a
 *                            refused cycle changes nothing.
 * cslam_pf_assoc_cycle_drawn the same with unknown correspondences: the control run (test/main.cpp:279-286), then the body
 *                            of cslam_pf_assoc_scan_step_drawn behind its predict -- cslam_pf_associate_vote
 *                            (EKF.cpp:131-144, 235-326), cslam_pf_sample_proposal_voted_drawn(step) (PF.cpp:502-544 +
 *                            222-277), cslam_pf_resample_local_drawn(step) (PF.cpp:473-500), cslam_pf_add_features_voted
 *                            (PF.cpp:9-60) -- with its return values, its *q, and its rule that a capacity overflow
 *                            leaves the run, the proposal and the resample applied and the vote live.  m = 0 is the
 *                            control run alone (*q = 0). */
int cslam_pf_control_run(cslam_pf_t h, int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                         const double* phi /* k or NULL */, int use_heading);
int cslam_pf_control_launches(cslam_pf_t h, long long* launches);
int cslam_pf_cycle_drawn(cslam_pf_t h, int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                         const double* phi, int use_heading, const void* ZF, int mf, const int* idf, const void* ZN, int mn,
                         const void* R, long long step, double n_effective, int resample_status);
int cslam_pf_assoc_cycle_drawn(cslam_pf_t h, int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                               const double* phi, int use_heading, const void* Z, int m, const void* R, double gate1,
                               double gate2, double new_fraction, double miss_likelihood, long long step,
                               double n_effective, int resample_status, int* q);

/* ---- the FastSLAM-1.0 step ----
 * The reference declares the switch between its two particle loops, mSwitchSampleProposal (slam.h:102), and runs only
 * the FastSLAM-2 one (test/main.cpp:249-334).  The pieces of the other lie next to it: addControlNoise (slam.h:149-159),
 * PF::likelihood (PF.cpp:343-359 over PF.cpp:279-317), PF::featureUpdate (PF.cpp:222-277), PF::resampleParticles
 * (PF.cpp:473-500) and PF::addOneNewFeature (PF.cpp:9-60).  The calls below make that loop: sample the motion per
 * particle, weight by the observation likelihood at the particle's own pose, update the features, resample.  Nothing in
 * them inverts Pv, so two scans may follow each other with Pv = 0 in between.
 *
 * The control draws are a stream of their own, a pure function of (seed of cslam_pf_seed_draws, control step, component,
 * GLOBAL particle slot): normal = T(counter_normal(splitmix64(seed, 0x4354524C), key(ctl_step, c, g))) with the key of
 * the proposal draws, c = 0 for the velocity and c = 1 for the steering.  A shard sees the noise of the unsharded set.
 *
 * cslam_pf_control_run_sampled  cslam_pf_control_run (test/main.cpp:277-286) with every particle's own noisy controls
 *                               (slam.h:149-159, Q taken as diagonal): step j of the run uses
 *                               vn = T(v[j]) + n0 * sqrt(T(Q[0,0])), swan = T(swa[j]) + n1 * sqrt(T(Q[1,1])), every
 *                               operation rounded in T, with the normals of control step ctl_step + j; then PF.cpp:419-471
 *                               with (vn, swan) and PF.cpp:382-417.  One launch per 16 steps, counted by
 *                               cslam_pf_control_launches.  Bit for bit cslam_pf_control_run of one particle with its
 *                               (vn, swan); Q = 0 is cslam_pf_control_run.  Any shard of a seeded set.  k = 0 returns
 *                               CSLAM_OK and launches nothing.  What cslam_pf_control_run refuses, ctl_step < 0, a negative
 *                               Q[0,0] or Q[1,1], an unseeded handle: CSLAM_ERR_BAD_ARG, nothing changes.
 * cslam_pf_get_control_draws    the normals of control steps ctl_step .. ctl_step + k - 1 for the owned particles,
 *                               [k][2][np] in the handle's dtype (for tests and for host restatements).  Synchronises.
 * cslam_pf_likelihood_update    PF.cpp:343-359 in one launch: for every owned particle and every observation i the
 *                               Jacobians at the particle's pose (PF.cpp:70-135), V = Z - ZP with the bearing wrapped, the
 *                               factor of PF.cpp:279-317, like = ((1 l_0) l_1) ... l_{m-1}, w <- w like.  update_features:
 *                               PF.cpp:222-277 rides along, bit for bit cslam_pf_feature_update(Z, m, idf, R) with the
 *                               handle's gain quirk (a list that names a feature twice gets that call behind the weights
 *                               instead).  zero_pv: Pv = 0 afterwards, the state PF.cpp:537 leaves, so FastSLAM-2 calls may
 *                               follow.  xv is never written.  m = 0 returns CSLAM_OK and touches nothing (nothing is read:
 *                               R may be NULL then).  Any shard; needs no draws.  NULL arrays with m > 0, m < 0, idf outside
 *                               1..nf: CSLAM_ERR_BAD_ARG before any launch.
 * cslam_pf_fs1_cycle_drawn      one iteration block for a handle that holds the whole seeded set: bit for bit
 *                               cslam_pf_control_run_sampled(.., ctl_step); mf > 0: cslam_pf_likelihood_update(ZF, mf, idf,
 *                               R, 1, 1) and cslam_pf_resample_local_drawn(step) with nothing returned (PF.cpp:473-500);
 *                               then cslam_pf_add_features(ZN, mn, R) at every particle's own pose (PF.cpp:9-60) -- no pose
 *                               is sampled: the particle is the sample.  With mf <= 32 and mn <= 32 no copy command is
 *                               enqueued.  Everything that can refuse does so before the first launch -- the refusals of
 *                               cslam_pf_control_run_sampled, a shard of a larger set, NULL arrays, idf outside 1..nf:
 *                               CSLAM_ERR_BAD_ARG; nf + mn > max_features: CSLAM_ERR_CAPACITY -- and a refused cycle
 *                               changes nothing. */
int cslam_pf_control_run_sampled(cslam_pf_t h, int k, const double* v, const double* swa, const void* Q, double wb,
                                 double dt, const double* phi /* k or NULL */, int use_heading, long long ctl_step);
int cslam_pf_get_control_draws(cslam_pf_t h, long long ctl_step, int k, void* normals /* [k][2][np], T */);
int cslam_pf_likelihood_update(cslam_pf_t h, const void* Z, int m, const int* idf, const void* R, int update_features,
                               int zero_pv);
int cslam_pf_fs1_cycle_drawn(cslam_pf_t h, int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                             const double* phi, int use_heading, long long ctl_step, const void* ZF, int mf, const int* idf,
                             const void* ZN, int mn, const void* R, long long step, double n_effective, int resample_status);
/* download one particle (host buffers; any may be NULL): w (1), Xv (3), Pv (9), XF (2*nf), PF (4*nf) */
int cslam_pf_get_particle(cslam_pf_t h, int index, void* w, void* Xv, void* Pv, void* XF, void* PF);
/* upload one particle with nf features (nf must equal the current feature count, or set it when the
 * store is empty of features) */
int cslam_pf_set_particle(cslam_pf_t h, int index, const void* w, const void* Xv, const void* Pv,
                          const void* XF, const void* PF, int nf);

/* ---- reading the estimate out of the particle set held in HBM.  Every call below is ordered on the handle's stream
 * behind whatever is queued, runs a few kernels, brings its results to the host with ONE copy, synchronises, and never
 * modifies the store.  Outputs are scalars of the handle's dtype (as for cslam_pf_get_particle): Xv 3, Pv 9
 * (column-major), XF 2*nf, PF 4*nf; any output pointer may be NULL, and with XF and PF both NULL (or nf = 0, which
 * leaves them untouched) the map kernels are skipped.
 *
 * cslam_pf_best_particle replaces Slam::extractStatesFromParticles(particles)  -- slam.h:493-511, called once per
 * iteration by the PF loop (test/main.cpp:330) -- and returns the chosen particle's whole record, not only its pose.
 * pick = CSLAM_PF_PICK_MAX chooses the particle of maximum weight, which is what the reference meant;
 * CSLAM_PF_PICK_MIN the one of minimum weight, which is what slam.h:505-506 does (`result.first` of
 * std::minmax_element is the minimum).  Ties go to the lowest index (minmax_element's "first"), a
 * NaN weight is never chosen, and if every weight is NaN the index is 0.
 *
 * cslam_pf_estimate has no counterpart in the reference: the moments of the mixture that the weighted particles form.
 *   *w_sum = W = sum w, *neff = W^2 / sum w^2,
 *   Xv = (sum w x / W, sum w y / W, atan2(sum w sin phi, sum w cos phi))           -- the heading mean is circular
 *   Pv = sum w (Pv_p + d d^T) / W,  d = (x - xbar, y - ybar, pi2pi(phi - phibar))  -- pi2pi: slam.h:816-829
 *   XF[f] = sum w XF_pf / W,  PF[f] = sum w (PF_pf + d d^T) / W,  d = XF_pf - XF[f],   for every feature f < nf
 * accumulated in double in a fixed order (the same store gives the same bits) with centred second moments.  If W is
 * zero, negative or not finite the call still returns CSLAM_OK: *w_sum is W as computed, *neff and every moment are NaN.
 *
 * cslam_pf_get_all_features replaces Slam::extractFeaturesFromParticles(particles)  -- slam.h:513-539: XF_all is the
 * 2 x (n_particles * nf) column-major matrix that slam.h:531-536 assembles, particle p's 2 x nf block at column p * nf. */
#define CSLAM_PF_PICK_MAX 0 /* what the reference meant        */
#define CSLAM_PF_PICK_MIN 1 /* what slam.h:505-506 does        */
int cslam_pf_best_particle(cslam_pf_t h, int pick, int* index, void* w, void* Xv, void* Pv, void* XF, void* PF);
int cslam_pf_estimate(cslam_pf_t h, double* w_sum, double* neff, void* Xv, void* Pv, void* XF, void* PF);
int cslam_pf_get_all_features(cslam_pf_t h, void* XF_all);
/* The same two reads (slam.h:493-511 and the mixture moments) over a set SHARDED as for cslam_pf_resample_sharded: rank r
 * owns the global indices [r * n_particles, (r + 1) * n_particles).  Every rank makes the same call with the same pick
 * and the same choice of NULL map pointers (from its own host thread on a loopback communicator).  Each rank reduces
 * its particles to a summary -- per moment group W, the mean and the second moment centred on that mean; its best
 * weight, global index and record --, one all-gather carries the summaries as doubles (one more, in the handle's dtype,
 * the best records), and every rank merges them in rank order (a pairwise Chan update; the lowest global index wins
 * ties), so that all ranks return identical bits.  A communicator of one rank gives the unsharded call's bits. */
int cslam_pf_best_particle_sharded(cslam_pf_t h, cslam_comm_t comm, int pick, long long* global_index, void* w, void* Xv,
                                   void* Pv, void* XF, void* PF);
int cslam_pf_estimate_sharded(cslam_pf_t h, cslam_comm_t comm, double* w_sum, double* neff, void* Xv, void* Pv, void* XF,
                              void* PF);

/* ---- the score and the trajectory log of the estimate, kept on the device (conan_slam_amd/csrc/pf_score_kernels.hpp).
 * The reference's PF loop prints its estimate on every iteration (test/main.cpp:330, from slam.h:493-511; the map:
 * slam.h:513-539), and a Monte-Carlo study scores that estimate against the truth after every step.  These calls do both
 * without draining the stream once per step: a score call queues the kernels of cslam_pf_estimate (or
 * cslam_pf_best_particle) up to, but without, the fetch, and two score kernels behind them that read the estimate as it
 * lies in HBM, i.e. the values those calls would have returned, rounded to the handle's dtype.  Totals, series and track
 * are read once, at the end.  All error and NEES arithmetic is f64 on the device; the sums are formed in a fixed order
 * without atomics, so two identical runs give identical bits.  The rules, the gates and the CSLAM_SCORE_* indices are
 * those of cslam_ekf_batch_score with one instance.  The particle store is never written. */
#define CSLAM_PF_SCORE_MEAN 0 /* the mixture moments of cslam_pf_estimate */
#define CSLAM_PF_SCORE_BEST 1 /* the maximum-weight particle, cslam_pf_best_particle(CSLAM_PF_PICK_MAX) */
/* Zeroes the totals, the series, the track and the call count, and chooses which estimate the following calls score
 * (replaces scoring state kept on the host beside test/main.cpp:330; slam.h:493-511).  series_capacity >= 0 records of
 * series and track alike (0: totals only).  A gate <= 0 selects the 95 % chi-square point: 7.8147 for the pose, 5.9915
 * for a landmark.  The truth rows are kept.  A score call without a prior reset behaves as after
 * score_reset(h, CSLAM_PF_SCORE_MEAN, 0, 0, 0).  A bad estimator or a negative capacity: CSLAM_ERR_BAD_ARG, nothing
 * changed.  A handle that never calls a score function allocates nothing for it. */
int cslam_pf_score_reset(cslam_pf_t h, int estimator, int series_capacity, double gate_pose, double gate_lm);
/* The truth the map part of the estimate (test/main.cpp:330, slam.h:493-511) is scored against: the true position of
 * state feature j + 1 is row j of lm_true (host, [count][2] doubles; the features slam.h:513-539 assembles), copied into
 * a device buffer sized for max_features before the call returns.  Features beyond `count` are not scored.  count < 0 or
 * count > max_features: CSLAM_ERR_BAD_ARG, nothing changed. */
int cslam_pf_score_set_truth(cslam_pf_t h, const double* lm_true /* host [count][2] */, int count);
/* One score step against the true pose xv_true (host [3], finite; it travels as kernel arguments): the estimate
 * test/main.cpp:330 prints (slam.h:493-511) -- Xv, Pv and, when with_map != 0, XF, PF of the first
 * c = min(n_features, truth count) features (slam.h:513-539) -- scored by the pose, landmark and series rules written at
 * cslam_ekf_batch_score above.  with_map == 0 scores no feature: the landmark totals are untouched and series fields 2
 * and 3 are NaN.  A degenerate weight sum makes the estimate NaN, which counts POSE_BAD += 1 and LM_BAD += c.
 *   track     while there is room, one record of five doubles per call: (Xv[0], Xv[1], Xv[2], W, Neff) for
 *             CSLAM_PF_SCORE_MEAN, (Xv[0], Xv[1], Xv[2], w_best, index) for CSLAM_PF_SCORE_BEST -- bit for bit what
 *             cslam_pf_estimate / cslam_pf_best_particle would have returned at that point, widened to double.
 * Returns when its kernels are enqueued on the handle's stream: no synchronise, no device-to-host copy, no staged
 * host-to-device copy (cslam_pf_stage_copies does not move).  A NULL or non-finite xv_true: CSLAM_ERR_BAD_ARG, nothing
 * changed. */
int cslam_pf_score(cslam_pf_t h, const double* xv_true /* host [3] */, int with_map);
/* cslam_pf_score (test/main.cpp:330, slam.h:493-511, slam.h:513-539) over a set SHARDED as for cslam_pf_estimate_sharded:
 * summaries, all-gather and combine as there, then the same score kernels on the merged block.  Every rank makes the
 * same call (same reset, same truth) and ends with identical totals, series and track; CSLAM_PF_SCORE_BEST records the
 * GLOBAL index.  A communicator of one rank gives the unsharded call's bits.  Everything that can fail is allocated
 * before the first collective. */
int cslam_pf_score_sharded(cslam_pf_t h, cslam_comm_t comm, const double* xv_true /* host [3] */, int with_map);
/* The one synchronising call of the score: copies the totals [CSLAM_SCORE_FIELDS], up to capacity_records series records
 * [records][4] and track records [records][5] (the read-out that replaces one cslam_pf_estimate per step:
 * test/main.cpp:330, slam.h:493-511).  *records = min(calls, series_capacity) is the number of records held (at most
 * capacity_records of them are copied), *calls counts every score call since the reset (calls beyond the series
 * capacity still enter the totals).  Any output pointer may be NULL. */
int cslam_pf_get_scores(cslam_pf_t h, double* totals /* [CSLAM_SCORE_FIELDS] */, float* series /* [records][4] */,
                        double* track /* [records][5] */, int capacity_records, int* records, long long* calls);

/* ------------------------------------------------------------------------------------------------
 * Device-side observation generator and known-association table: the per-step host work of
 * the reference's driver (test/main.cpp:139-165) -- a visibility filter over all landmarks and a table lookup per
 * observation -- with the map, the table, the scan and its split resident in HBM.
 *   cslam_sim_get_observations      Slam::getObservations, slam.h:575-683 with computeRangeBearing slam.h:339-368:
 *                                   landmarks with |dx|,|dy| < rmax, in front of the vehicle and inside the range
 *                                   circle, ascending tag order; Z (2 x m) and tags (1-based) are copied to the host
 *                                   pointers when these are not NULL.
 *   cslam_sim_add_observation_noise slam.h:168-178: Z[r][i] += normals[2i+r] * sqrt(R[r][r]) on the device-resident
 *                                   scan (the N(0,1) draws are an input, as for the particle filter).
 *   cslam_sim_associate_table       EKF::dataAssociateTable, EKF.cpp:146-233, on the device-resident scan: known tags
 *                                   -> (ZF, idf = their state position), unknown tags -> ZN, and the table assigns
 *                                   them the positions n_features+1, n_features+2, ... in scan order.
 *   cslam_sim_device_ptrs           the device-resident ZF / idf / ZN / Z / tags, e.g. for cslam_ekf_update_device.
 * All calls are synchronous with respect to their host outputs. */
typedef struct cslam_sim* cslam_sim_t;
int cslam_sim_create(const void* LM, int n_landmarks, int dtype, int device, cslam_sim_t* out);
int cslam_sim_destroy(cslam_sim_t h);
int cslam_sim_get_observations(cslam_sim_t h, const void* xv_true, double rmax, void* Z, int* tags, int* m);
int cslam_sim_add_observation_noise(cslam_sim_t h, const void* R, const void* normals);
int cslam_sim_associate_table(cslam_sim_t h, int n_features, void* ZF, int* idf, int* mf, void* ZN, int* mn);
int cslam_sim_device_ptrs(cslam_sim_t h, const void** dZF, const int** dIdf, const void** dZN, const void** dZ,
                          const int** dTags);
int cslam_sim_get_table(cslam_sim_t h, int* table);
int cslam_sim_set_table(cslam_sim_t h, const int* table);

/* ------------------------------------------------------------------------------------------------
 * Batched scan generator for Monte-Carlo studies through cslam_ekf_batch_* (f32): the sensor side of the reference's
 * demo loop (test/main.cpp:139-165, 188-189) for `instances` runs that share the true trajectory and the map, hence the
 * visible tags, the table association, idf, mf and mn; only the sensor noise differs.  One scan = one observation step
 * for all instances, in two launches on a stream of the generator's own:
 *   1. Slam::getObservations (slam.h:575-683, computeRangeBearing slam.h:339-368) and EKF::dataAssociateTable
 *      (EKF.cpp:146-233) ONCE, with the arithmetic and ordering of cslam_sim_get_observations / _associate_table;
 *   2. the sensor noise of slam.h:168-178 per instance i, scan position c (before the split) and component r (0 range,
 *      1 bearing), every operation in f32:  Z_i[r][c] = Z0[r][c] + float(g) * float(sqrt(R[r][r])),  g = the counter-based
 *      standard normal of conan_slam_amd/synth.py normal(seed, idx), evaluated in f64 on the device, with
 *      seed = seeds[i] + 1 and idx = (10000000 + step) * 64 + 2 c + r; the value goes to instance i's ZF or ZN column
 *      by the common split.  R == NULL: noise off (mSwitchSensorNoise = false), every instance gets Z0.
 * A scan holds at most 32 observations (the batched update's limit; the stride 64 of the noise key holds exactly their
 * draws): a pose that sees more returns CSLAM_ERR_CAPACITY and leaves the table and the current scan unchanged.
 * The generator keeps nf, the number of state features its table has assigned, and a small ring of scan slots in HBM;
 * a slot is rewritten only after the last kernel that consumed it has finished.  scan() waits only for its own two
 * kernels (the three counts come back through pinned memory), never for filter work in flight, and may be called as soon
 * as the previous scan has been consumed (there is one current scan: a new one replaces it, consumed or not, and the
 * table has then advanced past it).  `step` is the control-step number, counted from 1.
 *   create     LM: 2 x n_landmarks floats (host, column-major); seeds: one per instance; 1 <= instances <= 255.
 *   get_scan   host copies of the current scan (tests): ZF 2 x mf, idf mf, ZN 2 x mn of `instance`, tags m; any may be NULL.
 *   get_table / set_table  as cslam_sim_get_table / _set_table; set_table also sets nf to the highest position in it. */
typedef struct cslam_sim_batch* cslam_sim_batch_t;
int cslam_sim_batch_create(const float* LM, int n_landmarks, int instances, const long long* seeds, int device,
                           cslam_sim_batch_t* out);
int cslam_sim_batch_destroy(cslam_sim_batch_t h);
int cslam_sim_batch_scan(cslam_sim_batch_t h, const float* xv_true, double rmax, const float* R, long long step, int* m,
                         int* mf, int* mn);
int cslam_sim_batch_get_scan(cslam_sim_batch_t h, int instance, float* ZF, int* idf, float* ZN, int* tags);
int cslam_sim_batch_get_table(cslam_sim_batch_t h, int* table);
int cslam_sim_batch_set_table(cslam_sim_batch_t h, const int* table);
/* Slam::update(..., batch = true) (slam.h:938-943, EKF.cpp:93-129, test/main.cpp:188) on every instance with the
 * generator's CURRENT scan: the queueing rules, kernels and rounding of cslam_ekf_batch_update with that scan's ZF / idf,
 * without copying pointer tables (they are resident in the scan slot).  mf == 0 is a no-op.
 * Slam::augment (slam.h:190-191, EKF.cpp:9-91, test/main.cpp:189) likewise, as cslam_ekf_batch_augment with the scan's
 * ZN; mn == 0 is a no-op; CSLAM_ERR_CAPACITY beyond max_landmarks, with nothing changed.
 * Each may be called at most once per scan, and when mf > 0 the update comes before the augment.  CSLAM_ERR_BAD_ARG, with
 * nothing changed (state, queue, table, scan): different instance counts or devices, a batch whose feature count
 * (n - 3) / 2 is not the nf the scan was split against, a scan consumed twice, the wrong order, no current scan. */
int cslam_ekf_batch_update_scan(cslam_ekf_batch_t b, cslam_sim_batch_t s, const float* R);
int cslam_ekf_batch_augment_scan(cslam_ekf_batch_t b, cslam_sim_batch_t s, const float* R);
/* cslam_ekf_batch_score with the truth taken from the generator (the map and the table of test/main.cpp:139-165, the
 * blocks of EKF.cpp:131-144): for every tag t with table[t - 1] = p, 1 <= p <= (n - 3) / 2 of the batch, feature p's true
 * position is LM[:, t - 1].  A position is assigned once and never changes, so a gather kernel fills the rows of the
 * truth buffer not filled yet, and every feature of the batch is scored (a feature the table does not hold has no truth
 * and counts in LM_BAD).  Positions beyond the batch's feature count are ignored: the table may run a scan ahead.
 * cslam_sim_batch_scan has waited for its kernels when it returns, so the table is ordered by the host.  Replaces rows
 * given with score_set_truth.  CSLAM_ERR_BAD_ARG with nothing changed: different instance counts or devices, no current
 * scan. */
int cslam_ekf_batch_score_scan(cslam_ekf_batch_t b, cslam_sim_batch_t s, const float* xv_true /* host [3] */);

#ifdef __cplusplus
}
#endif
#endif /* CSLAM_H */
