// cslam_pf.hip -- host side of the FastSLAM-2 particle store behind the C ABI of include/cslam.h.
//
// One handle owns np particles (one shard of the global particle set) in structure-of-arrays form in HBM
// and launches one lane per particle (or per particle x observation).  The only step of the reference that
// couples particles -- resampleParticles, PF.cpp:473-500 -- is exposed in pieces (weight sums, scaling,
// pack / unpack of particle records, local gather) so that a multi-GPU driver can put its collectives
// between them (conan_slam_amd/pf.py does that with torch.distributed over RCCL).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "cslam_common.hpp"
#include "device_owners.hpp"
#include "pf_assoc_kernels.hpp"
#include "pf_buffers.hpp"
#include "pf_comm.hpp"
#include "pf_control_kernels.hpp"
#include "pf_draw_kernels.hpp"
#include "pf_estimate_kernels.hpp"
#include "pf_fs1_kernels.hpp"
#include "pf_kernels.hpp"
#include "pf_new_feature_kernels.hpp"
#include "pf_score_kernels.hpp"
#include "pf_staging.hpp"
#include "pf_vote_kernels.hpp"

using namespace cslam;

namespace
{

struct PfBase
{
    virtual ~PfBase() {}
    int         dtype  = CSLAM_F32;
    int         device = 0;
    int         quirks = CSLAM_Q_REF_EXACT;
    int         report_degenerate = 0; // cslam_pf_set_degenerate_policy
    int         np     = 0;
    int         nfcap  = 0;
    int         nf     = 0;
    Stream      stream_own;       // (in the base: destroyed after the buffers and events of Pf<T>)
    hipStream_t stream = nullptr; // = stream_own.get()
    long long   control_launches = 0; // pf_control_run_kernel launches (cslam_pf_control_launches)

    virtual int init()                                                                       = 0;
    virtual int set_uniform_weight(double w0)                                                 = 0;
    virtual int predict(double v, double swa, const void* Q, double wb, double dt)            = 0;
    virtual int observe_heading(double phi, int use)                                          = 0;
    virtual int sample_proposal(const void* Z, int m, const int* idf, const void* R, const void* normals) = 0;
    virtual int feature_update(const void* Z, int m, const int* idf, const void* R)           = 0;
    virtual int add_features(const void* Z, int q, const void* R)                             = 0;
    virtual int weight_sums(double* sums)                                                     = 0;
    virtual int scale_weights(double scale)                                                   = 0;
    virtual int set_degenerate_policy(int report)                                             = 0;
    virtual int divide_weights(double ws)                                                     = 0;
    virtual int weights_ptr(void** p)                                                         = 0;
    virtual int get_weights(void* w)                                                          = 0;
    virtual int set_weights(const void* w)                                                    = 0;
    virtual int record_bytes(long long* b)                                                    = 0;
    virtual int pack(const int* idx, int count, void* drec)                                   = 0;
    virtual int unpack(const int* idx, int count, const void* drec)                           = 0;
    virtual int gather_local(const int* keep, double w_new)                                   = 0;
    virtual int resample_local(const void* select, double n_eff, int status, double* neff, int* did) = 0;
    virtual int resample_sharded(Comm* c, const void* select, double n_eff, int status, double* neff, int* did) = 0;
    virtual int debug_last_exchange(int* counts, int* send_idx, int cap, int* n_send)                = 0;
    virtual int observation_step(double v, double swa, const void* Q, double wb, double dt, const void* Z, int m,
                                 const int* idf, const void* R, const void* normals, const void* select, double n_eff,
                                 int status) = 0;
    virtual int resample_stats(double* calls, double* resamples, double* last_neff) = 0;
    virtual int get_particle(int i, void* w, void* Xv, void* Pv, void* XF, void* PF)          = 0;
    virtual int set_particle(int i, const void* w, const void* Xv, const void* Pv, const void* XF, const void* PF,
                             int nf)                                                          = 0;
    // the read path (pf_estimate_kernels.hpp); c == nullptr: this handle alone
    virtual int best_particle(Comm* c, int pick, long long* index, void* w, void* Xv, void* Pv, void* XF, void* PF) = 0;
    virtual int estimate(Comm* c, double* w_sum, double* neff, void* Xv, void* Pv, void* XF, void* PF)              = 0;
    virtual int get_all_features(void* XF_all)                                                                      = 0;
    // the score of the estimate, kept on the device (pf_score_kernels.hpp); c == nullptr: this handle alone
    virtual int score_reset(int estimator, int series_capacity, double gate_pose, double gate_lm)                    = 0;
    virtual int score_set_truth(const double* lm_true, int count)                                                   = 0;
    virtual int score(Comm* c, const double* xv_true, int with_map)                                                 = 0;
    virtual int get_scores(double* totals, float* series, double* track, int capacity_records, int* records,
                           long long* calls)                                                                        = 0;
    // per-particle data association (pf_assoc_kernels.hpp) and the consumers of its table
    virtual int associate(const void* Z, int m, const void* R, double gate1, double gate2)                          = 0;
    virtual int get_association(int* idf, int* kind, double* summary)                                               = 0;
    virtual int sample_proposal_assoc(const void* Z, int m, const void* R, const void* normals, const int* use,
                                      double miss_likelihood)                                                       = 0;
    virtual int feature_update_assoc(const void* Z, int m, const void* R, const int* use)                           = 0;
    // the random inputs drawn on the device (pf_draw_kernels.hpp) and the calls that consume them
    virtual int seed_draws(long long seed, long long first_global, long long n_global)                              = 0;
    virtual int get_draws(long long step, void* normals, void* select)                                              = 0;
    virtual int sample_proposal_drawn(const void* Z, int m, const int* idf, const void* R, long long step)          = 0;
    virtual int sample_proposal_assoc_drawn(const void* Z, int m, const void* R, const int* use, double miss_likelihood,
                                            long long step)                                                         = 0;
    virtual int resample_local_drawn(long long step, double n_eff, int status, double* neff, int* did)              = 0;
    virtual int resample_sharded_drawn(Comm* c, long long step, double n_eff, int status, double* neff, int* did)   = 0;
    virtual int observation_step_drawn(double v, double swa, const void* Q, double wb, double dt, const void* Z, int m,
                                       const int* idf, const void* R, long long step, double n_eff, int status)     = 0;
    virtual int get_stage_copies(long long* copies)                                                                 = 0;
    // the scan that observes only new features (pf_new_feature_kernels.hpp); Q == nullptr: no predict
    virtual int sample_pose(const void* normals)                                                                    = 0;
    virtual int sample_pose_drawn(long long step)                                                                   = 0;
    virtual int new_feature_step(double v, double swa, const void* Q, double wb, double dt, const void* Z, int q,
                                 const void* R, const void* normals)                                                = 0;
    virtual int new_feature_step_drawn(double v, double swa, const void* Q, double wb, double dt, const void* Z, int q,
                                       const void* R, long long step)                                               = 0;
    // the vote on new features kept on the device (pf_vote_kernels.hpp) and the calls that consume it; c == nullptr: this
    // handle alone
    virtual int associate_vote(Comm* c, const void* Z, int m, const void* R, double gate1, double gate2,
                               double new_fraction)                                                                 = 0;
    virtual int vote_wait(int* q, int* use)                                                                         = 0;
    virtual int get_vote(int* use, int* new_idx, void* ZN, int* q)                                                  = 0;
    virtual int sample_proposal_voted(const void* Z, int m, const void* R, const void* normals, double miss_likelihood) = 0;
    virtual int sample_proposal_voted_drawn(const void* Z, int m, const void* R, double miss_likelihood, long long step) = 0;
    virtual int feature_update_voted(const void* Z, int m, const void* R)                                           = 0;
    virtual int add_features_voted(const void* R, int* q_out)                                                       = 0;
    virtual int assoc_scan_step_drawn(double v, double swa, const void* Q, double wb, double dt, const void* Z, int m,
                                      const void* R, double gate1, double gate2, double new_fraction,
                                      double miss_likelihood, long long step, double n_eff, int status, int* q_out) = 0;
    // a run of control steps in one launch per kPfControlMax (pf_control_kernels.hpp) and the whole-cycle calls behind it
    virtual int control_run(int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                            const double* phi, int use)                                                             = 0;
    virtual int cycle_drawn(int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                            const double* phi, int use, const void* ZF, int mf, const int* idf, const void* ZN, int mn,
                            const void* R, long long step, double n_eff, int status)                                = 0;
    virtual int assoc_cycle_drawn(int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                                  const double* phi, int use, const void* Z, int m, const void* R, double gate1,
                                  double gate2, double new_fraction, double miss_likelihood, long long step, double n_eff,
                                  int status, int* q_out)                                                           = 0;
    // the FastSLAM-1 step (pf_fs1_kernels.hpp): per-particle control noise, likelihood weights, the whole block
    virtual int control_run_sampled(int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                                    const double* phi, int use, long long ctl_step)                                 = 0;
    virtual int get_control_draws(long long ctl_step, int k, void* normals)                                         = 0;
    virtual int likelihood_update(const void* Z, int m, const int* idf, const void* R, int update_features, int zero_pv) = 0;
    virtual int fs1_cycle_drawn(int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                                const double* phi, int use, long long ctl_step, const void* ZF, int mf, const int* idf,
                                const void* ZN, int mn, const void* R, long long step, double n_eff, int status)    = 0;
};

// Pf<T> sequences the runtime calls of every entry point; what it sequences them over lives in parts with one job each
// (pf_staging.hpp, pf_buffers.hpp, pf_host_parts.hpp).  The parts are members, so they die before PfBase's stream.
template <typename T>
struct Pf : PfBase
{
    DevBuf<T>          dW;
    PfArrays<T>        cur, twin; // the store, and the set the single-pass resample gathers into; swapped by every resample
    PfObsArea<T>       obs;
    DevBuf<double>     dSums;
    DevBuf<T>          dRec; // scratch for gather_local
    PfStageRing        ring;
    PfResampleBufs<T>  rs;
    PfShardedBufs<T>   sh;
    PfEstimateBufs<T>  est;
    PfScoreBufs        sc;
    PfAssocTables<T>   assoc;
    PfVote<T>          vote;
    PfDraws<T>         draws;

    ~Pf() override
    {
        (void)hipSetDevice(device);
        if (stream)
        {
            (void)hipStreamSynchronize(stream);
        }
    }

    int use_device()
    {
        CSLAM_HIP_TRY(hipSetDevice(device));
        return CSLAM_OK;
    }

    PfStore<T> store_of(const PfArrays<T>& a) const
    {
        return PfStore<T>{dW.get(), a.xv.get(), a.pv.get(), a.xf.get(), a.pf.get(), np, nf};
    }
    PfStore<T> store() const { return store_of(cur); }

    int ensure_m(int m) { return obs.ensure(m, stream); }

    int init() override
    {
        CSLAM_TRY(use_device());
        CSLAM_TRY(stream_own.create(hipStreamNonBlocking));
        stream    = stream_own.get();
        size_t n1 = (size_t)np;
        size_t cf = (size_t)std::max(nfcap, 1);
        obs.set_particles(np);
        // w = 1/np until the driver sets the global value
        CSLAM_TRY(dW.alloc(n1));
        CSLAM_TRY(cur.alloc_zeroed(n1, cf, stream));
        CSLAM_TRY(dSums.alloc(2));
        CSLAM_TRY(dRec.alloc(n1 * (13 + 6 * cf)));
        CSLAM_TRY(twin.alloc_zeroed(n1, cf, stream));
        CSLAM_TRY(ensure_m(64));
        CSLAM_TRY(set_uniform_weight(1.0 / (double)np));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // One launch helper per kernel that more than one entry point launches.  Z | idf | normals are those of the staging
    // area.  The quirk decides the gain of the feature update: a flag of the update kernels, another of the fused forms.
    // ------------------------------------------------------------------------------------------------
    int update_gain() const { return (quirks & CSLAM_Q_LOWER_CHOL_GAIN) ? 0 : 1; }
    int fused_update_gain() const { return (quirks & CSLAM_Q_LOWER_CHOL_GAIN) ? 1 : 2; }
    static PfPredict<T> no_predict() { return PfPredict<T>{0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0}; }

    int launch_predict(double v, double swa, const T* Q, double wb, double dt)
    {
        hipLaunchKernelGGL(pf_predict_kernel<T>, dim3((np + 63) / 64), dim3(64), 0, stream, store(), (T)v, (T)swa, Q[0],
                           Q[1], Q[2], Q[3], (T)wb, (T)dt);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    // fu: 0 = proposal alone, else fused_update_gain()
    int launch_proposal(int m, const T* R, const PfPredict<T>& pr, int fu)
    {
        hipLaunchKernelGGL(pf_sample_proposal_kernel<T>, dim3((np * kPfSubLanes + 63) / 64), dim3(64), 0, stream,
                           store(), obs.z(), obs.dIdf(), m, R[0], R[1], R[2], R[3], obs.dNormals(), pr, fu);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    // use: the mask on the device -- the staging area's idf slot (a caller's mask travels there) or the vote's
    int launch_proposal_assoc(int m, const T* R, double miss_likelihood, const int* use)
    {
        hipLaunchKernelGGL(pf_sample_proposal_assoc_kernel<T>, dim3((np * kPfSubLanes + 63) / 64), dim3(64), 0, stream,
                           store(), obs.z(), assoc.tab.idf.get(), use, m, R[0], R[1], R[2], R[3], obs.dNormals(),
                           (T)miss_likelihood, fused_update_gain());
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    int launch_feature_update(int m, const T* R)
    {
        hipLaunchKernelGGL(pf_feature_update_kernel<T>, dim3((np + 63) / 64, m), dim3(64), 0, stream, store(), obs.z(),
                           obs.dIdf(), m, R[0], R[1], R[2], R[3], update_gain());
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    int launch_feature_update_assoc(int m, const T* R, const int* use)
    {
        hipLaunchKernelGGL(pf_feature_update_assoc_kernel<T>, dim3((np + 63) / 64, m), dim3(64), 0, stream, store(),
                           obs.z(), assoc.tab.idf.get(), use, m, R[0], R[1], R[2], R[3], update_gain());
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    int launch_weight_sums()
    {
        hipLaunchKernelGGL(pf_weight_sums_kernel<T>, dim3(1), dim3(256), 0, stream, dW.get(), np, dSums.get());
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    // w = value (set) or w *= value
    int launch_scale_weights(double value, int set)
    {
        hipLaunchKernelGGL(pf_scale_weights_kernel<T>, dim3((np + 255) / 256), dim3(256), 0, stream, dW.get(), np,
                           (T)value, set);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    // wv[0..n) /= ws
    int launch_divide_weights(T* wv, int n, double ws)
    {
        hipLaunchKernelGGL(pf_divide_weights_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, stream, wv, n, ws);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    // wv[0..n) normalised by the weight sum ws as the plan kernel does it (PF.cpp:482-487): by the scale (T)(1 / ws)
    // where that is a normal number of T, else by division (pf_kernels.hpp, at pf_scale_is_normal)
    int launch_normalize(T* wv, int n, double ws)
    {
        if (!pf_use_scale<T>(ws, report_degenerate))
        {
            return launch_divide_weights(wv, n, ws);
        }
        hipLaunchKernelGGL(pf_scale_weights_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, stream, wv, n, (T)(1.0 / ws), 0);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    int launch_pack(const int* d_idx, int count, T* d_rec)
    {
        hipLaunchKernelGGL(pf_pack_kernel<T>, dim3(count), dim3(256), 0, stream, store(), d_idx, count, d_rec);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    // d_idx == nullptr: record i into slot i
    int launch_unpack(const int* d_idx, int count, const T* d_rec)
    {
        hipLaunchKernelGGL(pf_unpack_kernel<T>, dim3(count), dim3(256), 0, stream, store(), d_idx, count, d_rec);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    int set_uniform_weight(double w0) override
    {
        CSLAM_TRY(use_device());
        return launch_scale_weights(w0, 1);
    }

    int predict(double v, double swa, const void* Qv, double wb, double dt) override
    {
        if (!Qv)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_predict: Q is null");
        }
        CSLAM_TRY(use_device());
        return launch_predict(v, swa, static_cast<const T*>(Qv), wb, dt);
    }

    int observe_heading(double phi, int use) override
    {
        if (!use)
        {
            return CSLAM_OK;
        }
        CSLAM_TRY(use_device());
        T sigma = (T)(((double)0.01f * kPi) / 180.0); // PF.cpp:391
        hipLaunchKernelGGL(pf_heading_kernel<T>, dim3((np + 63) / 64), dim3(64), 0, stream, store(), (T)phi,
                           sigma * sigma);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    int check_idf(const int* idf, int m, const char* who)
    {
        for (int i = 0; i < m; i++)
        {
            if (idf[i] < 1 || idf[i] > nf)
            {
                return fail(CSLAM_ERR_BAD_ARG, "%s: idf[%d]=%d outside 1..%d", who, i, idf[i], nf);
            }
        }
        return CSLAM_OK;
    }

    // stage Z (2*m) and idf (m, or the use[] mask, or nullptr) of one call, plus the 3*np normals when given; inputs are
    // consumed before return.  Without normals, a call whose Z / idf the staging area already holds sends nothing.
    int stage(const void* Z, int m, const int* idf, const void* normals = nullptr)
    {
        CSLAM_TRY(ensure_m(m));
        if (!normals && obs.holds(Z, m, idf))
        {
            return CSLAM_OK;
        }
        const PfObsLayout<T>& lay = obs.layout();
        const size_t zb = lay.bytes_z(m), ib = idf ? (size_t)m * sizeof(int) : 0, nb = (size_t)3 * np * sizeof(T);
        const size_t bytes = normals ? lay.bytes_z_idf_normals() : (idf ? lay.bytes_z_idf(m) : zb);
        CSLAM_TRY(obs.receive(ring, bytes, stream, [&](char* slot) {
            if (zb)
            {
                std::memcpy(slot, Z, zb);
            }
            if (ib)
            {
                std::memcpy(slot + lay.off_idf(), idf, ib);
            }
            if (normals)
            {
                std::memcpy(slot + lay.off_normals(), normals, nb);
            }
        }));
        obs.remember(Z, m, idf);
        return CSLAM_OK;
    }

    int sample_proposal(const void* Z, int m, const int* idf, const void* Rv, const void* normals) override
    {
        if (m < 0 || !Rv || !normals || (m > 0 && (!Z || !idf)))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_sample_proposal: bad arguments");
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(check_idf(idf, m, "pf_sample_proposal"));
        CSLAM_TRY(stage(Z, m, idf, normals));
        return launch_proposal(m, static_cast<const T*>(Rv), no_predict(), 0);
    }

    int feature_update(const void* Z, int m, const int* idf, const void* Rv) override
    {
        if (m < 0 || !Rv || (m > 0 && (!Z || !idf)))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_feature_update: bad arguments");
        }
        if (m == 0)
        {
            return CSLAM_OK;
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(check_idf(idf, m, "pf_feature_update"));
        CSLAM_TRY(stage(Z, m, idf));
        return launch_feature_update(m, static_cast<const T*>(Rv));
    }

    int add_features(const void* Z, int q, const void* Rv) override
    {
        if (q < 0 || !Rv || (q > 0 && !Z))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_add_features: bad arguments");
        }
        if (q == 0)
        {
            return CSLAM_OK;
        }
        if (nf + q > nfcap)
        {
            return fail(CSLAM_ERR_CAPACITY, "pf_add_features: %d features would exceed max_features=%d", nf + q, nfcap);
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(stage(Z, q, nullptr));
        const T* R = static_cast<const T*>(Rv);
        hipLaunchKernelGGL(pf_add_features_kernel<T>, dim3((np + 63) / 64, q), dim3(64), 0, stream, store(), obs.z(), q,
                           R[0], R[1], R[2], R[3]);
        CSLAM_HIP_TRY(hipGetLastError());
        nf += q;
        return CSLAM_OK;
    }

    int weight_sums(double* sums) override
    {
        if (!sums)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_weight_sums: null");
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(launch_weight_sums());
        CSLAM_HIP_TRY(hipMemcpyAsync(sums, dSums.get(), 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int scale_weights(double scale) override
    {
        CSLAM_TRY(use_device());
        return launch_scale_weights(scale, 0);
    }

    int set_degenerate_policy(int report) override
    {
        if (report != 0 && report != 1)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_set_degenerate_policy: %d is neither CSLAM_PF_REPAIR nor CSLAM_PF_REPORT", report);
        }
        report_degenerate = report;
        return CSLAM_OK;
    }

    int divide_weights(double ws) override
    {
        CSLAM_TRY(use_device());
        return launch_divide_weights(dW.get(), np, ws);
    }

    int weights_ptr(void** p) override
    {
        if (!p)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_weights_device_ptr: null");
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // the caller will read it from another stream
        *p = dW.get();
        return CSLAM_OK;
    }

    int get_weights(void* w) override
    {
        if (!w)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_get_weights: null");
        }
        CSLAM_TRY(use_device());
        CSLAM_HIP_TRY(hipMemcpyAsync(w, dW.get(), (size_t)np * sizeof(T), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int set_weights(const void* w) override
    {
        if (!w)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_set_weights: null");
        }
        CSLAM_TRY(use_device());
        CSLAM_HIP_TRY(hipMemcpyAsync(dW.get(), w, (size_t)np * sizeof(T), hipMemcpyHostToDevice, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int record_bytes(long long* b) override
    {
        if (!b)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_record_bytes: null");
        }
        *b = (long long)(13 + 6 * nf) * (long long)sizeof(T);
        return CSLAM_OK;
    }

    int stage_idx(const int* idx, int count, const char* who)
    {
        if (count < 0 || (count > 0 && !idx))
        {
            return fail(CSLAM_ERR_BAD_ARG, "%s: bad index list", who);
        }
        for (int i = 0; i < count; i++)
        {
            if (idx[i] < 0 || idx[i] >= np)
            {
                return fail(CSLAM_ERR_BAD_ARG, "%s: index %d outside 0..%d", who, idx[i], np - 1);
            }
        }
        CSLAM_TRY(ensure_m(count));
        CSLAM_HIP_TRY(hipMemcpyAsync(obs.dIdx(), idx, (size_t)count * sizeof(int), hipMemcpyHostToDevice, stream));
        return CSLAM_OK;
    }

    int pack(const int* idx, int count, void* drec) override
    {
        if (count == 0)
        {
            return CSLAM_OK;
        }
        if (!drec)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_pack: null buffer");
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(stage_idx(idx, count, "pf_pack"));
        CSLAM_TRY(launch_pack(obs.dIdx(), count, static_cast<T*>(drec)));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // the buffer is handed to a collective on another stream
        return CSLAM_OK;
    }

    int unpack(const int* idx, int count, const void* drec) override
    {
        if (count == 0)
        {
            return CSLAM_OK;
        }
        if (!drec)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_unpack: null buffer");
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(stage_idx(idx, count, "pf_unpack"));
        assoc.memo.moved();
        CSLAM_TRY(launch_unpack(obs.dIdx(), count, static_cast<const T*>(drec)));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    // PF.cpp:490-499 for a single shard: slot i <- particle keep[i], weights = w_new
    int gather_local(const int* keep, double w_new) override
    {
        CSLAM_TRY(use_device());
        CSLAM_TRY(stage_idx(keep, np, "pf_gather_local"));
        assoc.memo.moved();
        CSLAM_TRY(launch_pack(obs.dIdx(), np, dRec.get()));
        std::vector<int> ident((size_t)np);
        for (int i = 0; i < np; i++)
        {
            ident[i] = i;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        CSLAM_HIP_TRY(hipMemcpyAsync(obs.dIdx(), ident.data(), (size_t)np * sizeof(int), hipMemcpyHostToDevice, stream));
        CSLAM_TRY(launch_unpack(obs.dIdx(), np, dRec.get()));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return set_uniform_weight(w_new);
    }

    // PF.cpp:473-500 for a single shard that holds the whole particle set, without leaving the device: plan
    // (sums, normalise, Neff, decision, keep[]) -> gather into the twin set -> w = 1/N, the last two gated by a device
    // flag.  One D2H of {Neff, flag} at the end, and only if the caller asks for them.
    int resample_local(const void* select, double n_eff, int status, double* neff, int* did) override
    {
        if (!select)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_resample_local: null select");
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(rs.ensure(np, stream));
        const size_t bytes = (size_t)np * sizeof(T);
        CSLAM_TRY(ring.send(rs.sel.get(), bytes, stream, [&](char* slot) { std::memcpy(slot, select, bytes); }));
        CSLAM_TRY(launch_resample(rs.sel.get(), n_eff, status));
        return resample_result(neff, did);
    }

    // {Neff, resampled} of the resample just launched, when the caller asks for either
    int resample_result(double* neff, int* did)
    {
        if (neff || did)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(rs.hInfo.get(), rs.info.get(), 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            if (neff)
            {
                *neff = rs.hInfo[0];
            }
            if (did)
            {
                *did = rs.hInfo[1] != 0.0 ? 1 : 0;
            }
        }
        return CSLAM_OK;
    }

    int resample_sharded(Comm* c, const void* select, double n_eff, int status, double* neff, int* did) override
    {
        if (!c || !select)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_resample_sharded: null communicator or select");
        }
        return resample_sharded_from(c, select, 0, n_eff, status, neff, did);
    }

    int resample_sharded_drawn(Comm* c, long long step, double n_eff, int status, double* neff, int* did) override
    {
        if (!c)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_resample_sharded_drawn: null communicator");
        }
        CSLAM_TRY(need_draws("pf_resample_sharded_drawn"));
        if (draws.nglobal != (long long)c->world * np || draws.first != (long long)c->rank * np)
        {
            return fail(CSLAM_ERR_BAD_ARG,
                        "pf_resample_sharded_drawn: the draws were seeded for slots %lld.. of %lld, rank %d of %d holds %lld.. of %lld",
                        draws.first, draws.nglobal, c->rank, c->world, (long long)c->rank * np, (long long)c->world * np);
        }
        return resample_sharded_from(c, nullptr, step, n_eff, status, neff, did);
    }

    // PF.cpp:473-500 over a particle set sharded across ranks (one rank per GPU): see cslam_pf_resample_sharded in
    // include/cslam.h.  Everything is ordered on the handle's stream; the host reads back the two global sums (the
    // decision must be the same on every rank and drives which collectives run) and, when it resamples, the
    // 2 x world record counts of the exchange.
    // select != nullptr: the caller's strata positions (one staged copy); nullptr: those of `step`, drawn on the device
    int resample_sharded_from(Comm* c, const void* select, long long step, double n_eff, int status, double* neff, int* did)
    {
        if (!c->loop && !rccl())
        {
            return fail(CSLAM_ERR_HIP, "pf_resample_sharded: librccl could not be loaded");
        }
        const int world = c->world, rank = c->rank, L = np, N = np * world;
        assoc.memo.moved();
        CSLAM_TRY(use_device());
        CSLAM_TRY(sh.ensure(world, nf, np, stream));
        const ncclDataType_t dt = (sizeof(T) == 4) ? ncclFloat : ncclDouble;
        // the strata positions go to the device up front as well (staging can fail; the copy is cheap when unused)
        if (select)
        {
            const size_t bytes = (size_t)N * sizeof(T);
            CSLAM_TRY(ring.send(sh.plan.selG.get(), bytes, stream, [&](char* slot) { std::memcpy(slot, select, bytes); }));
        }
        else
        {
            CSLAM_TRY(launch_draw(step, nullptr, sh.plan.selG.get(), N, 0, nullptr, nullptr));
        }
        // 1. global weight sums, formed by every rank from the gathered weights with the reduction of the one-shard plan
        // kernel: an all-reduce of per-rank sums would add the same f64 terms in an order that depends on the partition,
        // and the normalised weights of a set would then depend, in their last bits, on how many ranks hold it
        T* wall = sh.plan.wall.get();
        CSLAM_TRY(c->all_gather(dW.get(), wall, (size_t)L, dt, sizeof(T), stream));
        hipLaunchKernelGGL(pf_weight_sums_kernel<T>, dim3(1), dim3(256), 0, stream, wall, N, sh.plan.sumsG.get());
        CSLAM_HIP_TRY(hipGetLastError());
        double* hs = sh.h_sums(); // (pinned; the counts use it later)
        CSLAM_HIP_TRY(hipMemcpyAsync(hs, sh.plan.sumsG.get(), 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        const double ws = hs[0], ws2 = hs[1];
        // 2. w /= ws (PF.cpp:482-487), Neff = 1 / sum (w/ws)^2 (PF.cpp:549-554), the decision (PF.cpp:490); as the plan
        // kernel does at the ends of the range: Neff from the sums of the normalised weights where the raw squares have
        // left the range of double (f64 only)
        CSLAM_TRY(launch_normalize(dW.get(), np, ws));
        double ne = pf_neff_raw(ws, ws2, report_degenerate);
        bool   wall_normalised = false;
        if (sizeof(T) == 8 && pf_sum_usable(ws) && !pf_neff_from_raw_sums(ws, ws2))
        {
            CSLAM_TRY(launch_normalize(wall, N, ws));
            wall_normalised = true;
            hipLaunchKernelGGL(pf_weight_sums_kernel<T>, dim3(1), dim3(256), 0, stream, wall, N, sh.plan.sumsG.get());
            CSLAM_HIP_TRY(hipGetLastError());
            CSLAM_HIP_TRY(hipMemcpyAsync(hs, sh.plan.sumsG.get(), 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            ne = (hs[0] * hs[0]) / hs[1];
        }
        const bool go = (ne < n_eff) && status;
        if (neff)
        {
            *neff = ne;
        }
        if (did)
        {
            *did = go ? 1 : 0;
        }
        sh.last_counts.assign((size_t)2 * world, 0);
        sh.last_n_send = 0;
        if (!go)
        {
            return CSLAM_OK;
        }
        // 3. every rank plans the same keep[] from the gathered weights, normalised as its own were, and the shared strata
        if (!wall_normalised)
        {
            CSLAM_TRY(launch_normalize(wall, N, ws));
        }
        hipLaunchKernelGGL(pf_keep_kernel<T>, dim3(1), dim3(256), 0, stream, wall, N, sh.plan.selG.get(),
                           sh.plan.keepG.get(), sh.plan.cumG.get());
        CSLAM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pf_exchange_plan_kernel<0>, dim3(1), dim3(256), 0, stream, sh.plan.keepG.get(), N, L, rank, world,
                           sh.plan.sendIdx.get(), sh.plan.counts.get());
        CSLAM_HIP_TRY(hipGetLastError());
        int* hc = sh.h_counts();
        CSLAM_HIP_TRY(hipMemcpyAsync(hc, sh.plan.counts.get(), (size_t)2 * world * sizeof(int), hipMemcpyDeviceToHost,
                                     stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        int        n_send = 0, n_recv = 0;
        const bool plan_ok = pf_exchange_plan_ok(hc, world, rank, L, &n_send, &n_recv);
        sh.last_counts.assign(hc, hc + 2 * world);
        sh.last_n_send = n_send;
        // (every rank derives the plan from the same gathered weights, so these checks fail on all ranks or on none)
        if (!plan_ok)
        {
            return fail(CSLAM_ERR_HIP, "pf_resample_sharded: inconsistent exchange plan (%d of %d slots filled, self %d / %d)",
                        n_recv, L, hc[rank], hc[world + rank]);
        }
        const size_t rec = (size_t)(13 + 6 * nf);
        T *          sbuf = sh.rec.send.get(), *rbuf = sh.rec.recv.get();
        // 4. records out of the store (before any slot is overwritten), exchange, records into the slots in order
        if (n_send > 0)
        {
            CSLAM_TRY(launch_pack(sh.plan.sendIdx.get(), n_send, sbuf));
        }
        size_t soff = 0, roff = 0;
        // the records that stay on this rank: a device copy, outside the group
        pf_exchange_offsets(hc, world, rank, &soff, &roff);
        if (hc[rank] > 0)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(rbuf + roff * rec, sbuf + soff * rec, (size_t)hc[rank] * rec * sizeof(T),
                                         hipMemcpyDeviceToDevice, stream));
        }
        int rc = c->group_start();
        if (rc)
        {
            return rc;
        }
        for (int r = 0; r < world && rc == CSLAM_OK; r++)
        {
            const size_t sc = (size_t)hc[r], rcv = (size_t)hc[world + r];
            pf_exchange_offsets(hc, world, r, &soff, &roff);
            if (r != rank && sc > 0)
            {
                rc = c->send(sbuf + soff * rec, sc * rec, dt, sizeof(T), r, stream);
            }
            if (r != rank && rcv > 0 && rc == CSLAM_OK)
            {
                rc = c->recv(rbuf + roff * rec, rcv * rec, dt, sizeof(T), r, stream);
            }
        }
        const int rc_end = c->group_end(stream); // (closed on the failure path too)
        if (rc || rc_end)
        {
            return rc ? rc : rc_end;
        }
        CSLAM_TRY(launch_unpack(nullptr, L, rbuf));
        return set_uniform_weight(1.0 / (double)N); // PF.cpp:495-499
    }

    // test introspection: the record counts (2 * world) and the send list of the last sharded resample
    int debug_last_exchange(int* counts, int* send_idx, int cap, int* n_send) override
    {
        if (n_send)
        {
            *n_send = sh.last_n_send;
        }
        if (counts)
        {
            std::copy(sh.last_counts.begin(), sh.last_counts.end(), counts);
        }
        if (send_idx && sh.last_n_send > 0)
        {
            if (cap < sh.last_n_send)
            {
                return fail(CSLAM_ERR_BAD_ARG, "debug_last_exchange: capacity %d < %d", cap, sh.last_n_send);
            }
            CSLAM_TRY(use_device());
            CSLAM_HIP_TRY(hipMemcpyAsync(send_idx, sh.plan.sendIdx.get(), (size_t)sh.last_n_send * sizeof(int),
                                         hipMemcpyDeviceToHost, stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        }
        return CSLAM_OK;
    }

    // plan (sums, normalise, Neff, decision, keep[]) -> gather -> copy back + w = 1/N, the last two gated by a device flag
    int launch_resample(const T* d_select, double n_eff, int status)
    {
        assoc.memo.moved(); // (whether it resamples is decided on the device)
        hipLaunchKernelGGL(pf_resample_plan_kernel<T>, dim3(1), dim3(256), 0, stream, dW.get(), np, d_select, n_eff,
                           status, rs.cum.get(), rs.keep.get(), rs.info.get(), rs.enable.get(), report_degenerate);
        CSLAM_HIP_TRY(hipGetLastError());
        const dim3 ggrid(13 + 6 * nf, (np + 255) / 256);
        const T    w_new = (T)(1.0 / (double)np);
        hipLaunchKernelGGL(pf_gather_move_kernel<T>, ggrid, dim3(256), 0, stream, store(), store_of(twin), rs.keep.get(),
                           rs.enable.get(), w_new);
        CSLAM_HIP_TRY(hipGetLastError());
        std::swap(cur, twin); // the twin set is the store now (whether particles moved or were copied in place)
        return CSLAM_OK;
    }

    // One whole FastSLAM-2 observation step for a shard that holds every particle -- predict, sampleProposal,
    // featureUpdate, resampleParticles (PF.cpp:419-471, 502-544, 222-277, 473-500) -- with ONE staged host-to-device
    // copy for all its small inputs (Z | idf | normals | select) and nothing returned to the host.
    int observation_step(double v, double swa, const void* Qv, double wb, double dt, const void* Z, int m, const int* idf,
                         const void* Rv, const void* normals, const void* select, double n_eff, int status) override
    {
        if (!Qv || !Rv || m < 0 || (m > 0 && (!Z || !idf || !normals)) || !select)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_observation_step: bad arguments");
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(check_idf(idf, m, "pf_observation_step"));
        CSLAM_TRY(ensure_m(std::max(m, 1)));
        CSLAM_TRY(rs.ensure(np, stream));
        const PfObsLayout<T>& lay = obs.layout();
        // (zero-copy -- the kernels reading the pinned slot over the host link -- was tried instead of this staged copy:
        // 13.7 k instead of 15.0 k steps/s)
        // (a small kernel reading the pinned slot in place of this copy command: 19.6 k instead of 19.9 k steps/s)
        // (a second stream for this copy, double-buffered inputs and event hand-overs so that it runs under the previous
        // step's kernels was tried: 14.8 k instead of 16.7 k steps/s -- four more runtime calls per step cost more host
        // time than the 10 us of stream time they free)
        CSLAM_TRY(obs.receive(ring, lay.bytes_step(), stream, [&](char* slot) {
            if (m > 0)
            {
                std::memcpy(slot, Z, lay.bytes_z(m));
                std::memcpy(slot + lay.off_idf(), idf, (size_t)m * sizeof(int));
                std::memcpy(slot + lay.off_normals(), normals, (size_t)3 * np * sizeof(T));
            }
            std::memcpy(slot + lay.off_select(), select, (size_t)np * sizeof(T));
        }));
        return launch_observation_step(v, swa, Qv, wb, dt, m, idf, Rv, n_eff, status);
    }

    // the launches of one observation step behind its inputs in the staging area (Z | idf | normals | select); idf: the
    // host copy
    int launch_observation_step(double v, double swa, const void* Qv, double wb, double dt, int m, const int* idf,
                                const void* Rv, double n_eff, int status)
    {
        const T* Q = static_cast<const T*>(Qv);
        const T* R = static_cast<const T*>(Rv);
        if (m > 0) // predict rides inside the proposal kernel (which overwrites xv / Pv anyway)
        {
            const PfPredict<T> pr{1, (T)v, (T)swa, Q[0], Q[1], Q[2], Q[3], (T)wb, (T)dt};
            // ... and so does the feature update, unless an observation list names a feature twice (the separate kernel
            // then updates it twice from the same old value, last writer wins: kept as it was)
            const int fu = pf_has_duplicate(idf, m) ? 0 : fused_update_gain();
            CSLAM_TRY(launch_proposal(m, R, pr, fu));
            if (fu == 0)
            {
                CSLAM_TRY(launch_feature_update(m, R));
            }
        }
        else
        {
            CSLAM_TRY(launch_predict(v, swa, Q, wb, dt));
        }
        return launch_resample(obs.dSelect(), n_eff, status);
    }

    int resample_stats(double* calls, double* resamples, double* last_neff) override
    {
        CSLAM_TRY(use_device());
        CSLAM_TRY(rs.ensure(np, stream));
        CSLAM_HIP_TRY(hipMemcpyAsync(rs.hInfo.get(), rs.info.get(), 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        if (last_neff)
        {
            *last_neff = rs.hInfo[0];
        }
        if (calls)
        {
            *calls = rs.hInfo[2];
        }
        if (resamples)
        {
            *resamples = rs.hInfo[3];
        }
        return CSLAM_OK;
    }

    // column i of an np-column array <-> a contiguous host vector of `rows` scalars (nothing for a null vector or no rows)
    int copy_column(void* host, T* dev, int i, size_t rows, bool to_device)
    {
        const size_t s = sizeof(T), pitch = (size_t)np * s;
        if (host && rows > 0 && to_device)
        {
            CSLAM_HIP_TRY(hipMemcpy2DAsync(dev + i, pitch, host, s, s, rows, hipMemcpyHostToDevice, stream));
        }
        else if (host && rows > 0)
        {
            CSLAM_HIP_TRY(hipMemcpy2DAsync(host, s, dev + i, pitch, s, rows, hipMemcpyDeviceToHost, stream));
        }
        return CSLAM_OK;
    }
    int copy_particle(int i, void* Xv, void* Pv, void* XF, void* PF, int nfeat, bool to_device)
    {
        CSLAM_TRY(copy_column(Xv, cur.xv.get(), i, 3, to_device));
        CSLAM_TRY(copy_column(Pv, cur.pv.get(), i, 9, to_device));
        CSLAM_TRY(copy_column(XF, cur.xf.get(), i, (size_t)2 * nfeat, to_device));
        CSLAM_TRY(copy_column(PF, cur.pf.get(), i, (size_t)4 * nfeat, to_device));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int get_particle(int i, void* w, void* Xv, void* Pv, void* XF, void* PF) override
    {
        if (i < 0 || i >= np)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_get_particle: index %d", i);
        }
        CSLAM_TRY(use_device());
        if (w)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(w, dW.get() + i, sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        return copy_particle(i, Xv, Pv, XF, PF, nf, false);
    }

    int set_particle(int i, const void* w, const void* Xv, const void* Pv, const void* XF, const void* PF,
                     int nfeat) override
    {
        if (i < 0 || i >= np || nfeat < 0 || nfeat > nfcap)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_set_particle: index %d / nf %d", i, nfeat);
        }
        CSLAM_TRY(use_device());
        assoc.memo.moved();
        if (w)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(dW.get() + i, w, sizeof(T), hipMemcpyHostToDevice, stream));
        }
        CSLAM_TRY(copy_particle(i, const_cast<void*>(Xv), const_cast<void*>(Pv), const_cast<void*>(XF),
                                const_cast<void*>(PF), nfeat, true)); // (read only in this direction)
        nf = nfeat; // every particle of the store carries the same number of features
        return CSLAM_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // The read path: best particle, mixture moments, all features.  Every call queues its launches behind whatever is
    // on the stream, brings ONE block back through est.hEst (pinned) and synchronises; the store is only read.
    // ------------------------------------------------------------------------------------------------
    int est_grow_common(size_t part_count, size_t od)
    {
        CSLAM_TRY(est.grow(est.part, part_count, stream));
        CSLAM_TRY(est.grow(est.out, od, stream));
        return est.grow(est.hEst, od * sizeof(double), stream);
    }
    int    est_chunks() const { return (np + kEstChunk - 1) / kEstChunk; }
    size_t est_out_doubles() const { return (size_t)kEstOutHdr + ((size_t)(13 + 6 * nf) * sizeof(T) + 7) / 8; }
    int est_comm_ok(Comm* c, const char* who)
    {
        if (c && !c->loop && !rccl())
        {
            return fail(CSLAM_ERR_HIP, "%s: librccl could not be loaded", who);
        }
        return CSLAM_OK;
    }

    // the launches of the best-particle read: the block [hdr | rec] of the pick in est.out, nothing fetched
    int launch_best(Comm* c, int pick)
    {
        const int    nch = est_chunks(), len = 13 + 6 * nf, world = c ? c->world : 1;
        const size_t od  = est_out_doubles();
        // (everything that can fail is allocated before the first collective)
        CSLAM_TRY(est_grow_common((size_t)nch * kEstP1, od));
        if (c)
        {
            CSLAM_TRY(est.grow(est.local, od, stream));
            CSLAM_TRY(est.grow(est.bestHdrAll, (size_t)world * kEstOutHdr, stream));
            CSLAM_TRY(est.grow(est.bestRecAll, (size_t)world * len, stream));
        }
        double* local = c ? est.local.get() : est.out.get();
        hipLaunchKernelGGL(pf_est_pass1_kernel<T>, dim3(nch), dim3(256), 0, stream, store(), est.part.get());
        CSLAM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pf_best_finish_kernel<T>, dim3(1), dim3(256), 0, stream, store(), est.part.get(), nch, pick,
                           c ? (long long)c->rank * np : 0LL, local, est.rec(local));
        CSLAM_HIP_TRY(hipGetLastError());
        if (c)
        {
            const ncclDataType_t dt = (sizeof(T) == 4) ? ncclFloat : ncclDouble;
            CSLAM_TRY(c->all_gather(local, est.bestHdrAll.get(), (size_t)kEstOutHdr, ncclDouble, sizeof(double), stream));
            CSLAM_TRY(c->all_gather(est.rec(local), est.bestRecAll.get(), (size_t)len, dt, sizeof(T), stream));
            hipLaunchKernelGGL(pf_best_combine_kernel<T>, dim3(1), dim3(256), 0, stream, est.bestHdrAll.get(),
                               est.bestRecAll.get(), world, len, pick, est.out.get(), est.rec(est.out.get()));
            CSLAM_HIP_TRY(hipGetLastError());
        }
        return CSLAM_OK;
    }

    int best_particle(Comm* c, int pick, long long* index, void* w, void* Xv, void* Pv, void* XF, void* PF) override
    {
        if (pick != kEstPickMax && pick != kEstPickMin)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_best_particle: pick %d is neither CSLAM_PF_PICK_MAX nor _MIN", pick);
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(est_comm_ok(c, "pf_best_particle_sharded"));
        CSLAM_TRY(launch_best(c, pick));
        const int  len = 13 + 6 * nf;
        const bool map = nf > 0 && (XF || PF);
        CSLAM_TRY(est.fetch(est.out.get(), map ? (size_t)len : 13, stream));
        if (index)
        {
            *index = (long long)est.h_hdr()[2];
        }
        est.scatter(map, nf, w, Xv, Pv, XF, PF);
        return CSLAM_OK;
    }

    // the launches of the mixture moments (map: with every feature's): the block [hdr | rec] in est.out, nothing fetched
    int launch_estimate(Comm* c, bool map)
    {
        const int    nch = est_chunks(), world = c ? c->world : 1;
        const int    stride = kEstSumHdr + (map ? kEstSumFeat * nf : 0);
        CSLAM_TRY(est_grow_common((size_t)nch * (kEstP1 + kEstP2Pose + (map ? (size_t)kEstP2Feat * nf : 0)),
                                  est_out_doubles()));
        if (c)
        {
            CSLAM_TRY(est.grow(est.sum, (size_t)stride, stream));
            CSLAM_TRY(est.grow(est.sumAll, (size_t)world * stride, stream));
        }
        double* p1 = est.part.get();
        double* p2 = p1 + (size_t)nch * kEstP1;
        double* pm = map ? p2 + (size_t)nch * kEstP2Pose : nullptr;
        double* out = est.out.get();
        const int fgroups = map ? (nf + kEstFeatPerWg - 1) / kEstFeatPerWg : 0;
        const int fblocks = map ? (nf + 255) / 256 : 0;
        hipLaunchKernelGGL(pf_est_pass1_kernel<T>, dim3(nch), dim3(256), 0, stream, store(), p1);
        CSLAM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pf_est_pass2_kernel<T>, dim3(nch, 1 + fgroups), dim3(256), 0, stream, store(), p1, nch, p2, pm);
        CSLAM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pf_est_finish_kernel<T>, dim3(1 + fblocks), dim3(256), 0, stream, store(), p1, p2, pm, nch,
                           c ? est.sum.get() : nullptr, out, est.rec(out));
        CSLAM_HIP_TRY(hipGetLastError());
        if (c)
        {
            CSLAM_TRY(c->all_gather(est.sum.get(), est.sumAll.get(), (size_t)stride, ncclDouble, sizeof(double), stream));
            hipLaunchKernelGGL(pf_est_combine_kernel<T>, dim3(1 + fblocks), dim3(256), 0, stream, est.sumAll.get(), world,
                               stride, nf, map ? 1 : 0, out, est.rec(out));
            CSLAM_HIP_TRY(hipGetLastError());
        }
        return CSLAM_OK;
    }

    int estimate(Comm* c, double* w_sum, double* neff, void* Xv, void* Pv, void* XF, void* PF) override
    {
        CSLAM_TRY(use_device());
        CSLAM_TRY(est_comm_ok(c, "pf_estimate_sharded"));
        const bool map = nf > 0 && (XF || PF);
        CSLAM_TRY(launch_estimate(c, map));
        CSLAM_TRY(est.fetch(est.out.get(), map ? (size_t)(13 + 6 * nf) : 13, stream));
        if (w_sum)
        {
            *w_sum = est.h_hdr()[0];
        }
        if (neff)
        {
            *neff = est.h_hdr()[1];
        }
        est.scatter(map, nf, nullptr, Xv, Pv, XF, PF);
        return CSLAM_OK;
    }

    int get_all_features(void* XF_all) override
    {
        int rc = use_device();
        if (rc || nf == 0 || !XF_all)
        {
            return rc;
        }
        const size_t count = (size_t)2 * nf * np;
        CSLAM_TRY(est.grow(est.feat, count, stream));
        CSLAM_TRY(est.grow(est.hEst, count * sizeof(T), stream));
        hipLaunchKernelGGL(pf_all_features_kernel<T>, dim3((np + 63) / 64, (2 * nf + 63) / 64), dim3(256), 0, stream,
                           store(), est.feat.get());
        CSLAM_HIP_TRY(hipGetLastError());
        CSLAM_HIP_TRY(hipMemcpyAsync(est.hEst.get(), est.feat.get(), count * sizeof(T), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        std::memcpy(XF_all, est.hEst.get(), count * sizeof(T));
        return CSLAM_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // The score of the estimate and its trajectory log, kept in HBM (pf_score_kernels.hpp).  A score call queues the
    // launches of the read path above -- up to, but without, the fetch -- and the two score kernels behind them on the
    // estimate block; only get_scores synchronises and copies.
    // ------------------------------------------------------------------------------------------------
    int score_reset(int estimator, int series_capacity, double gate_pose, double gate_lm) override
    {
        if (!PfScoreBook::reset_args_ok(estimator, series_capacity))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_score_reset: estimator %d (CSLAM_PF_SCORE_MEAN or _BEST), series_capacity %d (>= 0)",
                        estimator, series_capacity);
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(sc.ensure_base(CSLAM_SCORE_FIELDS, nfcap, stream));
        CSLAM_TRY(sc.ensure_log(series_capacity, stream));
        CSLAM_HIP_TRY(hipMemsetAsync(sc.base.totals.get(), 0, CSLAM_SCORE_FIELDS * sizeof(double), stream));
        if (sc.log.series)
        {
            CSLAM_HIP_TRY(hipMemsetAsync(sc.log.series.get(), 0, sc.log.series.count() * sizeof(float), stream));
            CSLAM_HIP_TRY(hipMemsetAsync(sc.log.track.get(), 0, sc.log.track.count() * sizeof(double), stream));
        }
        sc.book.reset(estimator, series_capacity, gate_pose, gate_lm);
        return CSLAM_OK;
    }

    int score_set_truth(const double* lm_true, int count) override
    {
        if (!PfScoreBook::truth_args_ok(count, nfcap) || (count > 0 && !lm_true))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_score_set_truth: count %d outside 0..max_features=%d, or null rows", count, nfcap);
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(sc.ensure_base(CSLAM_SCORE_FIELDS, nfcap, stream));
        if (count > 0)
        {
            // (behind whatever score call still reads the old rows; the host array is consumed before the return)
            CSLAM_HIP_TRY(hipMemcpyAsync(sc.base.truth.get(), lm_true, (size_t)2 * count * sizeof(double),
                                         hipMemcpyHostToDevice, stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        }
        sc.book.set_truth_count(count);
        return CSLAM_OK;
    }

    int score(Comm* c, const double* xv_true, int with_map) override
    {
        const char* who = c ? "pf_score_sharded" : "pf_score";
        if (!xv_true || !std::isfinite(xv_true[0]) || !std::isfinite(xv_true[1]) || !std::isfinite(xv_true[2]))
        {
            return fail(CSLAM_ERR_BAD_ARG, "%s: xv_true is null or not finite", who);
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(est_comm_ok(c, who));
        // (everything that can fail is allocated before the first collective: the score's here, the read path's in its
        // launch helpers)
        CSLAM_TRY(sc.ensure_base(CSLAM_SCORE_FIELDS, nfcap, stream));
        const PfScoreBook& bk    = sc.book;
        const int          count = bk.scored(nf, with_map);
        if (bk.estimator() == CSLAM_PF_SCORE_BEST)
        {
            CSLAM_TRY(launch_best(c, kEstPickMax));
        }
        else
        {
            CSLAM_TRY(launch_estimate(c, count > 0));
        }
        const double* hdr    = est.out.get();
        const T*      rec    = est.rec(est.out.get());
        const int     blocks = PfScoreBook::blocks(count);
        if (count > 0)
        {
            hipLaunchKernelGGL(pf_score_landmarks_kernel<T>, dim3(blocks), dim3(256), 0, stream, rec, nf, count,
                               sc.base.truth.get(), bk.gate_lm(), sc.base.parts.get());
            CSLAM_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(pf_score_finish_kernel<T>, dim3(1), dim3(64), 0, stream, hdr, rec, sc.base.parts.get(), blocks,
                           xv_true[0], xv_true[1], xv_true[2], bk.gate_pose(), bk.estimator(), sc.base.totals.get(),
                           sc.log.series.get(), sc.log.track.get(), (double)bk.next_record());
        CSLAM_HIP_TRY(hipGetLastError());
        sc.book.called();
        return CSLAM_OK;
    }

    int get_scores(double* totals, float* series, double* track, int capacity_records, int* records, long long* calls) override
    {
        if (capacity_records < 0)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_get_scores: capacity_records %d", capacity_records);
        }
        CSLAM_TRY(use_device());
        const PfScoreBook& bk = sc.book;
        const size_t       n  = (size_t)bk.records_to_copy(capacity_records);
        if (totals && !sc.allocated())
        {
            std::fill(totals, totals + CSLAM_SCORE_FIELDS, 0.0);
        }
        else if (totals)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(totals, sc.base.totals.get(), CSLAM_SCORE_FIELDS * sizeof(double),
                                         hipMemcpyDeviceToHost, stream));
        }
        if (series && n > 0)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(series, sc.log.series.get(), n * 4 * sizeof(float), hipMemcpyDeviceToHost, stream));
        }
        if (track && n > 0)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(track, sc.log.track.get(), n * kPfScoreTrack * sizeof(double), hipMemcpyDeviceToHost,
                                         stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        if (records)
        {
            *records = bk.records();
        }
        if (calls)
        {
            *calls = bk.calls();
        }
        return CSLAM_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // Per-particle gated nearest-neighbour association (EKF.cpp:131-144, 235-326 on each particle's own state) and the
    // consumers that read its table.  The tables belong to the handle and describe the LAST associate call
    // (assoc.memo): its observations, the particle order and the map size of that moment.
    // ------------------------------------------------------------------------------------------------
    int associate(const void* Z, int m, const void* Rv, double gate1, double gate2) override
    {
        if (m < 0 || m > 65535 || !Rv || (m > 0 && !Z)) // (one grid row per observation)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_associate: bad arguments (m=%d)", m);
        }
        if (!std::isfinite(gate1) || !std::isfinite(gate2))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_associate: gates must be finite (gate1=%g, gate2=%g)", gate1, gate2);
        }
        CSLAM_TRY(use_device());
        const int nchunks = (nf + kPfAssocFeatChunk - 1) / kPfAssocFeatChunk;
        if (m > 0)
        {
            CSLAM_TRY(assoc.ensure(m, nchunks, np, stream));
            CSLAM_TRY(stage(Z, m, nullptr));
            const T*   R  = static_cast<const T*>(Rv);
            const int  pb = (np + 63) / 64;
            const auto& p = assoc.part;
            const auto& t = assoc.tab;
            if (nchunks > 0)
            {
                hipLaunchKernelGGL(pf_assoc_scan_kernel<T>, dim3(pb, nchunks, (m + kPfAssocObsChunk - 1) / kPfAssocObsChunk),
                                   dim3(64), 0, stream, store(), obs.z(), m, R[0], R[1], R[2], R[3], (T)gate1,
                                   p.nd.get(), p.j.get(), p.nis.get());
                CSLAM_HIP_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(pf_assoc_merge_kernel<T>, dim3(pb, m), dim3(64), 0, stream, np, m, nchunks, p.nd.get(),
                               p.j.get(), p.nis.get(), (T)gate2, t.rawIdf.get(), t.rawKind.get(), t.rawNd.get());
            CSLAM_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(pf_assoc_resolve_kernel<T>, dim3(pb, m), dim3(64), 0, stream, np, m, t.rawIdf.get(),
                               t.rawKind.get(), t.rawNd.get(), t.idf.get(), t.kind.get());
            CSLAM_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(pf_assoc_summary_kernel<T>, dim3(m), dim3(256), 0, stream, dW.get(), np, t.kind.get(),
                               t.summary.get());
            CSLAM_HIP_TRY(hipGetLastError());
        }
        assoc.memo.associated(Z, m, nf);
        vote.memo.forget(); // a vote belongs to the associate it was taken on
        return CSLAM_OK;
    }

    int get_association(int* idf, int* kind, double* summary) override
    {
        const int am = assoc.memo.m();
        if (am < 0)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_get_association: cslam_pf_associate has not been called");
        }
        CSLAM_TRY(use_device());
        const size_t cnt = (size_t)am * np;
        if (idf && cnt)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(idf, assoc.tab.idf.get(), cnt * sizeof(int), hipMemcpyDeviceToHost, stream));
        }
        if (kind && cnt)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(kind, assoc.tab.kind.get(), cnt * sizeof(int), hipMemcpyDeviceToHost, stream));
        }
        if (summary && am)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(summary, assoc.tab.summary.get(), (size_t)am * 4 * sizeof(double),
                                         hipMemcpyDeviceToHost, stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    // the texts of PfAssocMemo's refusals
    int check_assoc_inputs(const void* Z, int m, const int* use, const char* who)
    {
        int i = 0;
        switch (assoc.memo.check(Z, m, nf, use, &i))
        {
        case PfAssocRefusal::none:
            return CSLAM_OK;
        case PfAssocRefusal::never_associated:
            return fail(CSLAM_ERR_BAD_ARG, "%s: cslam_pf_associate has not been called", who);
        case PfAssocRefusal::moved:
            return fail(CSLAM_ERR_BAD_ARG,
                        "%s: particles were resampled, unpacked or set since cslam_pf_associate (its table is per slot)", who);
        case PfAssocRefusal::other_scan:
            return fail(CSLAM_ERR_BAD_ARG, "%s: Z / m (%d) are not those of the last cslam_pf_associate (m=%d)", who, m,
                        assoc.memo.m());
        case PfAssocRefusal::map_shrank:
            return fail(CSLAM_ERR_BAD_ARG, "%s: the map shrank (%d features) since cslam_pf_associate (%d)", who, nf,
                        assoc.memo.nf());
        case PfAssocRefusal::bad_use:
            break;
        }
        return fail(CSLAM_ERR_BAD_ARG, "%s: use[%d]=%d is neither 0 nor 1", who, i, use[i]);
    }

    int sample_proposal_assoc(const void* Z, int m, const void* Rv, const void* normals, const int* use,
                              double miss_likelihood) override
    {
        if (m < 0 || !Rv || !normals || (m > 0 && (!Z || !use)) || !std::isfinite(miss_likelihood))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_sample_proposal_assoc: bad arguments");
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(check_assoc_inputs(Z, m, use, "pf_sample_proposal_assoc"));
        CSLAM_TRY(stage(Z, m, use, normals));
        return launch_proposal_assoc(m, static_cast<const T*>(Rv), miss_likelihood, obs.dIdf());
    }

    int feature_update_assoc(const void* Z, int m, const void* Rv, const int* use) override
    {
        if (m < 0 || !Rv || (m > 0 && (!Z || !use)))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_feature_update_assoc: bad arguments");
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(check_assoc_inputs(Z, m, use, "pf_feature_update_assoc"));
        if (m == 0)
        {
            return CSLAM_OK;
        }
        CSLAM_TRY(stage(Z, m, use));
        return launch_feature_update_assoc(m, static_cast<const T*>(Rv), obs.dIdf());
    }

    // ------------------------------------------------------------------------------------------------
    // The random inputs drawn on the device (pf_draw_kernels.hpp).  A _drawn call is its host-array twin with ONE
    // producer launch in place of the caller's normals / select: pf_stage_draw_kernel fills the staging area in the
    // layout the consumers read, and these are launched behind it with the arguments they always get.  Up to
    // kPfDrawObsMax observations Z / idf ride along as kernel arguments (no copy command at all); more take the staged copy.
    // ------------------------------------------------------------------------------------------------
    int seed_draws(long long seed, long long first_global, long long n_global) override
    {
        long long n_strata = 0;
        if (!pf_seed_args_ok(first_global, n_global, np, &n_strata))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_seed_draws: need 0 <= first_global, first_global + %d <= n_global < 2^32 (got %lld, %lld)",
                        np, first_global, n_global);
        }
        CSLAM_TRY(use_device());
        return draws.reseed(seed, first_global, n_global, n_strata, np, stream);
    }

    int need_draws(const char* who)
    {
        if (!draws.seeded)
        {
            return fail(CSLAM_ERR_BAD_ARG, "%s: cslam_pf_seed_draws has not been called", who);
        }
        return CSLAM_OK;
    }
    int need_whole_set(const char* who)
    {
        int rc = need_draws(who);
        if (rc == CSLAM_OK && (draws.first != 0 || draws.nglobal != np))
        {
            rc = fail(CSLAM_ERR_BAD_ARG, "%s: the draws were seeded for slots %lld.. of %lld, this handle resamples its own %d",
                      who, draws.first, draws.nglobal, np);
        }
        return rc;
    }

    // normals (3 np, or nullptr), select (n_sel strata, or nullptr with n_sel = 0) of `step`, and -- m > 0 -- Z | idf into
    // the staging area from the kernel's own arguments
    int launch_draw(long long step, T* normals, T* select, int n_sel, int m, const void* Z, const int* idf)
    {
        PfDrawObs<T> o;
        std::memset(&o, 0, sizeof(o));
        if (m > 0)
        {
            std::memcpy(o.z, Z, (size_t)2 * m * sizeof(T));
            if (idf) // (none: the new-feature scan has no correspondences; the idf slots get zeros)
            {
                std::memcpy(o.idf, idf, (size_t)m * sizeof(int));
            }
        }
        const int nn = normals ? np : 0;
        const int lanes = std::max(std::max(nn, n_sel), std::max(2 * m, 1));
        hipLaunchKernelGGL(pf_stage_draw_kernel<T>, dim3((lanes + 255) / 256), dim3(256), 0, stream, draws.seed,
                           (unsigned long long)step, (unsigned long long)draws.first, normals, nn, select, draws.di.get(),
                           n_sel, draws.k, obs.z(), obs.dIdf(), m, o);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    // Z | idf (or the use[] mask) of a proposal call and the normals of `step` into the staging area
    int stage_drawn(const void* Z, int m, const int* idf, long long step)
    {
        CSLAM_TRY(ensure_m(m));
        if (m > kPfDrawObsMax)
        {
            CSLAM_TRY(stage(Z, m, idf));
            return launch_draw(step, obs.dNormals(), nullptr, 0, 0, nullptr, nullptr);
        }
        obs.forget();
        CSLAM_TRY(launch_draw(step, obs.dNormals(), nullptr, 0, m, Z, idf));
        if (m > 0) // (what stage() remembers: a feature update right behind sends nothing)
        {
            obs.remember(Z, m, idf);
        }
        return CSLAM_OK;
    }

    int get_draws(long long step, void* normals, void* select) override
    {
        CSLAM_TRY(need_draws("pf_get_draws"));
        CSLAM_TRY(use_device());
        if (select && draws.nglobal > 0x7fffffffLL)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_get_draws: a set of %lld has no strata (at most 2^31 - 1), only normals", draws.nglobal);
        }
        T* dn = draws.out.get();
        T* ds = dn + (size_t)3 * np;
        CSLAM_TRY(launch_draw(step, normals ? dn : nullptr, select ? ds : nullptr, select ? (int)draws.nglobal : 0, 0, nullptr,
                              nullptr));
        if (normals)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(normals, dn, (size_t)3 * np * sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        if (select)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(select, ds, (size_t)draws.nglobal * sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int sample_proposal_drawn(const void* Z, int m, const int* idf, const void* Rv, long long step) override
    {
        if (m < 0 || !Rv || (m > 0 && (!Z || !idf)))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_sample_proposal_drawn: bad arguments");
        }
        CSLAM_TRY(need_draws("pf_sample_proposal_drawn"));
        CSLAM_TRY(use_device());
        CSLAM_TRY(check_idf(idf, m, "pf_sample_proposal_drawn"));
        CSLAM_TRY(stage_drawn(Z, m, idf, step));
        return launch_proposal(m, static_cast<const T*>(Rv), no_predict(), 0);
    }

    int sample_proposal_assoc_drawn(const void* Z, int m, const void* Rv, const int* use, double miss_likelihood,
                                    long long step) override
    {
        if (m < 0 || !Rv || (m > 0 && (!Z || !use)) || !std::isfinite(miss_likelihood))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_sample_proposal_assoc_drawn: bad arguments");
        }
        CSLAM_TRY(need_draws("pf_sample_proposal_assoc_drawn"));
        CSLAM_TRY(use_device());
        CSLAM_TRY(check_assoc_inputs(Z, m, use, "pf_sample_proposal_assoc_drawn"));
        CSLAM_TRY(stage_drawn(Z, m, use, step));
        return launch_proposal_assoc(m, static_cast<const T*>(Rv), miss_likelihood, obs.dIdf());
    }

    int resample_local_drawn(long long step, double n_eff, int status, double* neff, int* did) override
    {
        CSLAM_TRY(need_whole_set("pf_resample_local_drawn"));
        CSLAM_TRY(use_device());
        CSLAM_TRY(rs.ensure(np, stream));
        CSLAM_TRY(launch_draw(step, nullptr, rs.sel.get(), np, 0, nullptr, nullptr));
        CSLAM_TRY(launch_resample(rs.sel.get(), n_eff, status));
        return resample_result(neff, did);
    }

    // cslam_pf_observation_step with launches only: the producer writes normals | select (and Z | idf up to
    // kPfDrawObsMax observations) where the staged copy of the host-array form puts them
    int observation_step_drawn(double v, double swa, const void* Qv, double wb, double dt, const void* Z, int m,
                               const int* idf, const void* Rv, long long step, double n_eff, int status) override
    {
        if (!Qv || !Rv || m < 0 || (m > 0 && (!Z || !idf)))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_observation_step_drawn: bad arguments");
        }
        CSLAM_TRY(need_whole_set("pf_observation_step_drawn"));
        CSLAM_TRY(use_device());
        CSLAM_TRY(check_idf(idf, m, "pf_observation_step_drawn"));
        CSLAM_TRY(ensure_m(std::max(m, 1)));
        CSLAM_TRY(rs.ensure(np, stream));
        obs.forget();
        const bool by_copy = m > kPfDrawObsMax;
        if (by_copy)
        {
            CSLAM_TRY(stage(Z, m, idf));
        }
        CSLAM_TRY(launch_draw(step, m > 0 ? obs.dNormals() : nullptr, obs.dSelect(), np, by_copy ? 0 : m, Z, idf));
        return launch_observation_step(v, swa, Qv, wb, dt, m, idf, Rv, n_eff, status);
    }

    int get_stage_copies(long long* copies) override
    {
        if (!copies)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_stage_copies: null");
        }
        *copies = ring.copies();
        return CSLAM_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // The scan that observes only new features (test/main.cpp:314-328, pf_new_feature_kernels.hpp): sample every pose
    // from its own Gaussian, zero Pv, add the features at the sampled pose.  The normals sit where the proposal's sit in
    // the staging area; Z travels as add_features' does.  Poses and nf change, slots do not: the association memo is
    // left as cslam_pf_add_features and cslam_pf_predict leave it.
    // ------------------------------------------------------------------------------------------------
    int check_new_features(const void* Z, int q, const void* Rv, bool has_normals, const char* who)
    {
        switch (pf_new_feature_check(q, Z != nullptr, Rv != nullptr, has_normals, nf, nfcap))
        {
        case PfNewFeatureRefusal::none:
            return CSLAM_OK;
        case PfNewFeatureRefusal::capacity:
            return fail(CSLAM_ERR_CAPACITY, "%s: %d features would exceed max_features=%d", who, nf + q, nfcap);
        case PfNewFeatureRefusal::bad_arg:
            break;
        }
        return fail(CSLAM_ERR_BAD_ARG, "%s: bad arguments (q=%d)", who, q);
    }
    int launch_sample_pose()
    {
        hipLaunchKernelGGL(pf_sample_pose_kernel<T>, dim3((np + 63) / 64), dim3(64), 0, stream, store(), obs.dNormals());
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    // [predict +] sample + q new features behind Z | normals in the staging area; counts the features
    int launch_new_feature_step(double v, double swa, const void* Qv, double wb, double dt, int q, const void* Rv)
    {
        const T*     Q = static_cast<const T*>(Qv);
        const T*     R = static_cast<const T*>(Rv);
        const T      zero[4] = {(T)0, (T)0, (T)0, (T)0};
        PfPredict<T> pr = no_predict();
        if (Q)
        {
            pr = PfPredict<T>{1, (T)v, (T)swa, Q[0], Q[1], Q[2], Q[3], (T)wb, (T)dt};
        }
        if (!R) // (q == 0: nothing reads it)
        {
            R = zero;
        }
        hipLaunchKernelGGL(pf_new_feature_step_kernel<T>, dim3((np + 63) / 64), dim3(64), 0, stream, store(), obs.z(), q,
                           R[0], R[1], R[2], R[3], obs.dNormals(), pr);
        CSLAM_HIP_TRY(hipGetLastError());
        nf += q;
        return CSLAM_OK;
    }

    int sample_pose(const void* normals) override
    {
        CSLAM_TRY(check_new_features(nullptr, 0, nullptr, normals != nullptr, "pf_sample_pose"));
        CSLAM_TRY(use_device());
        CSLAM_TRY(stage(nullptr, 0, nullptr, normals));
        return launch_sample_pose();
    }

    int sample_pose_drawn(long long step) override
    {
        CSLAM_TRY(need_draws("pf_sample_pose_drawn"));
        CSLAM_TRY(use_device());
        CSLAM_TRY(stage_drawn(nullptr, 0, nullptr, step));
        return launch_sample_pose();
    }

    int new_feature_step(double v, double swa, const void* Qv, double wb, double dt, const void* Z, int q, const void* Rv,
                         const void* normals) override
    {
        CSLAM_TRY(check_new_features(Z, q, Rv, normals != nullptr, "pf_new_feature_step"));
        CSLAM_TRY(use_device());
        CSLAM_TRY(stage(Z, q, nullptr, normals));
        return launch_new_feature_step(v, swa, Qv, wb, dt, q, Rv);
    }

    // launches only up to kPfDrawObsMax new observations: the producer writes Z and the normals of `step`
    int new_feature_step_drawn(double v, double swa, const void* Qv, double wb, double dt, const void* Z, int q,
                               const void* Rv, long long step) override
    {
        CSLAM_TRY(check_new_features(Z, q, Rv, true, "pf_new_feature_step_drawn"));
        CSLAM_TRY(need_draws("pf_new_feature_step_drawn"));
        CSLAM_TRY(use_device());
        CSLAM_TRY(stage_drawn(Z, q, nullptr, step));
        return launch_new_feature_step(v, swa, Qv, wb, dt, q, Rv);
    }

    // ------------------------------------------------------------------------------------------------
    // The vote on new features, kept on the device (pf_vote_kernels.hpp): which observations of the last associate become
    // features of every particle.  The vote kernel runs behind the association's summary kernel and leaves use[], the
    // compacted new observations and their count in HBM; one device-to-host copy of [q, m, use[m]] and an event follow.
    // The _voted consumers launch the kernels of the _assoc consumers with the vote's use[] in the mask's place;
    // add_features_voted waits for the event alone (the host owns nf, and q sizes the grid) and launches
    // pf_add_features_kernel on the vote's ZN.  What the buffers describe: vote.memo (PfVoteMemo).
    // ------------------------------------------------------------------------------------------------
    int associate_vote(Comm* c, const void* Z, int m, const void* Rv, double gate1, double gate2,
                       double new_fraction) override
    {
        const char* who = c ? "pf_associate_vote_sharded" : "pf_associate_vote";
        if (!std::isfinite(new_fraction))
        {
            return fail(CSLAM_ERR_BAD_ARG, "%s: new_fraction must be finite (got %g)", who, new_fraction);
        }
        if (m < 0 || m > 65535 || !Rv || (m > 0 && !Z) || !std::isfinite(gate1) || !std::isfinite(gate2))
        {
            return associate(Z, m, Rv, gate1, gate2); // (refuses with its own text, changes nothing)
        }
        CSLAM_TRY(use_device());
        // everything that can fail comes before the collective: a rank never leaves its peers waiting inside one
        CSLAM_TRY(est_comm_ok(c, who));
        CSLAM_TRY(vote.ensure(m, c != nullptr, stream));
        CSLAM_TRY(associate(Z, m, Rv, gate1, gate2));
        if (m == 0) // nothing to vote on: q = 0, known at once, nothing launched
        {
            vote.memo.voted(0);
            vote.memo.arrived(0);
            return CSLAM_OK;
        }
        const double* summary = assoc.tab.summary.get();
        if (c)
        {
            // the sum over the ranks of the shards' summaries, identical on every rank (the loopback adds in rank order)
            CSLAM_TRY(c->all_reduce_sum_f64(summary, vote.summary_all.get(), 4 * m, stream));
            summary = vote.summary_all.get();
        }
        hipLaunchKernelGGL(pf_assoc_vote_kernel<T>, dim3(1), dim3(kPfVoteLanes), 0, stream, summary, obs.z(), m,
                           new_fraction, vote.use(), vote.b.new_idx.get(), vote.b.ZN.get(), vote.count());
        CSLAM_HIP_TRY(hipGetLastError());
        CSLAM_HIP_TRY(hipMemcpyAsync(vote.b.host.get(), vote.count(), PfVote<T>::copy_ints(m) * sizeof(int),
                                     hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipEventRecord(vote.ev.get(), stream));
        vote.memo.voted(m);
        return CSLAM_OK;
    }

    // the texts of PfVoteMemo's refusals
    int vote_refused(PfVoteRefusal r, const char* who)
    {
        switch (r)
        {
        case PfVoteRefusal::none:
            return CSLAM_OK;
        case PfVoteRefusal::already_added:
            return fail(CSLAM_ERR_BAD_ARG, "%s: the features of this vote have been added already", who);
        case PfVoteRefusal::no_vote:
            break;
        }
        return fail(CSLAM_ERR_BAD_ARG, "%s: no vote: cslam_pf_associate_vote has not been called since the last cslam_pf_associate",
                    who);
    }

    // q of the live vote on the host: waits for the vote's event, and for nothing queued behind it
    int vote_arrive(const char* who)
    {
        if (!vote.memo.waited())
        {
            CSLAM_HIP_TRY(hipEventSynchronize(vote.ev.get()));
            const int q = vote.h_count()[0], m = vote.h_count()[1];
            if (m != vote.memo.m() || q < 0 || q > m)
            {
                return fail(CSLAM_ERR_HIP, "%s: the vote came back as q=%d of m=%d, expected m=%d", who, q, m, vote.memo.m());
            }
            vote.memo.arrived(q);
        }
        return CSLAM_OK;
    }

    int vote_wait(int* q, int* use) override
    {
        CSLAM_TRY(vote_refused(vote.memo.check_read(), "pf_vote_wait"));
        CSLAM_TRY(use_device());
        CSLAM_TRY(vote_arrive("pf_vote_wait"));
        if (q)
        {
            *q = vote.memo.q();
        }
        if (use && vote.memo.m() > 0)
        {
            std::memcpy(use, vote.h_use(), (size_t)vote.memo.m() * sizeof(int));
        }
        return CSLAM_OK;
    }

    int get_vote(int* use, int* new_idx, void* ZN, int* q) override
    {
        CSLAM_TRY(vote_refused(vote.memo.check_read(), "pf_get_vote"));
        CSLAM_TRY(use_device());
        CSLAM_TRY(vote_arrive("pf_get_vote"));
        const int m = vote.memo.m(), nq = vote.memo.q();
        if (use && m > 0)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(use, vote.use(), (size_t)m * sizeof(int), hipMemcpyDeviceToHost, stream));
        }
        if (new_idx && nq > 0) // (entries from q on were never written)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(new_idx, vote.b.new_idx.get(), (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, stream));
        }
        if (ZN && nq > 0)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(ZN, vote.b.ZN.get(), (size_t)2 * nq * sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        if (q)
        {
            *q = nq;
        }
        return CSLAM_OK;
    }

    // a _voted consumer reads use[] next to the association table: a live vote, and the scan and slots of its associate
    int check_voted_inputs(const void* Z, int m, const char* who)
    {
        CSLAM_TRY(vote_refused(vote.memo.check_read(), who));
        switch (assoc.memo.check_scan(Z, m, nf))
        {
        case PfAssocRefusal::never_associated:
            return fail(CSLAM_ERR_BAD_ARG, "%s: cslam_pf_associate has not been called", who);
        case PfAssocRefusal::moved:
            return fail(CSLAM_ERR_BAD_ARG,
                        "%s: particles were resampled, unpacked or set (moved) since cslam_pf_associate_vote (its table is per slot)",
                        who);
        case PfAssocRefusal::other_scan:
            return fail(CSLAM_ERR_BAD_ARG, "%s: Z / m (%d) are not those of the last cslam_pf_associate_vote (m=%d)", who, m,
                        assoc.memo.m());
        case PfAssocRefusal::map_shrank:
            return fail(CSLAM_ERR_BAD_ARG, "%s: the map shrank (%d features) since cslam_pf_associate_vote (%d)", who, nf,
                        assoc.memo.nf());
        default:
            break;
        }
        return CSLAM_OK;
    }

    int sample_proposal_voted(const void* Z, int m, const void* Rv, const void* normals, double miss_likelihood) override
    {
        if (m < 0 || !Rv || !normals || (m > 0 && !Z) || !std::isfinite(miss_likelihood))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_sample_proposal_voted: bad arguments");
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(check_voted_inputs(Z, m, "pf_sample_proposal_voted"));
        CSLAM_TRY(stage(Z, m, nullptr, normals));
        return launch_proposal_assoc(m, static_cast<const T*>(Rv), miss_likelihood, vote.use());
    }

    int sample_proposal_voted_drawn(const void* Z, int m, const void* Rv, double miss_likelihood, long long step) override
    {
        if (m < 0 || !Rv || (m > 0 && !Z) || !std::isfinite(miss_likelihood))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_sample_proposal_voted_drawn: bad arguments");
        }
        CSLAM_TRY(need_draws("pf_sample_proposal_voted_drawn"));
        CSLAM_TRY(use_device());
        CSLAM_TRY(check_voted_inputs(Z, m, "pf_sample_proposal_voted_drawn"));
        CSLAM_TRY(stage_drawn(Z, m, nullptr, step));
        return launch_proposal_assoc(m, static_cast<const T*>(Rv), miss_likelihood, vote.use());
    }

    int feature_update_voted(const void* Z, int m, const void* Rv) override
    {
        if (m < 0 || !Rv || (m > 0 && !Z))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_feature_update_voted: bad arguments");
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(check_voted_inputs(Z, m, "pf_feature_update_voted"));
        if (m == 0)
        {
            return CSLAM_OK;
        }
        CSLAM_TRY(stage(Z, m, nullptr));
        return launch_feature_update_assoc(m, static_cast<const T*>(Rv), vote.use());
    }

    // PF.cpp:9-60 of the voted observations, read where the vote kernel left them.  Allowed after a resample: ZN is per
    // observation.  A refusal leaves the store, the count and the vote as they were.
    int add_features_voted(const void* Rv, int* q_out) override
    {
        if (!Rv)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_add_features_voted: R is null");
        }
        CSLAM_TRY(vote_refused(vote.memo.check_add(), "pf_add_features_voted"));
        CSLAM_TRY(use_device());
        CSLAM_TRY(vote_arrive("pf_add_features_voted"));
        const int q = vote.memo.q();
        if (q_out)
        {
            *q_out = q;
        }
        if (nf + q > nfcap)
        {
            return fail(CSLAM_ERR_CAPACITY, "pf_add_features_voted: %d features would exceed max_features=%d", nf + q, nfcap);
        }
        if (q > 0)
        {
            const T* R = static_cast<const T*>(Rv);
            hipLaunchKernelGGL(pf_add_features_kernel<T>, dim3((np + 63) / 64, q), dim3(64), 0, stream, store(),
                               vote.b.ZN.get(), q, R[0], R[1], R[2], R[3]);
            CSLAM_HIP_TRY(hipGetLastError());
            nf += q;
        }
        vote.memo.features_added();
        return CSLAM_OK;
    }

    // One scan of the unknown-correspondence loop for a handle that holds the whole set: predict, associate + vote, the
    // proposal on the vote's mask, the resample with nothing returned -- all queued -- and only then the wait for the
    // vote's event and the voted features.  No dispatch to the sampled-pose branch of an all-new scan: q is not known
    // when the proposal is queued.
    int assoc_scan_step_drawn(double v, double swa, const void* Qv, double wb, double dt, const void* Z, int m, const void* Rv,
                              double gate1, double gate2, double new_fraction, double miss_likelihood, long long step,
                              double n_eff, int status, int* q_out) override
    {
        if (!Qv || !Rv || m < 0 || m > 65535 || (m > 0 && !Z) || !std::isfinite(gate1) || !std::isfinite(gate2) ||
            !std::isfinite(new_fraction) || !std::isfinite(miss_likelihood))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_assoc_scan_step_drawn: bad arguments (m=%d)", m);
        }
        CSLAM_TRY(need_whole_set("pf_assoc_scan_step_drawn"));
        CSLAM_TRY(use_device());
        if (q_out)
        {
            *q_out = 0;
        }
        if (m == 0)
        {
            return launch_predict(v, swa, static_cast<const T*>(Qv), wb, dt);
        }
        CSLAM_TRY(launch_predict(v, swa, static_cast<const T*>(Qv), wb, dt));
        CSLAM_TRY(associate_vote(nullptr, Z, m, Rv, gate1, gate2, new_fraction));
        CSLAM_TRY(sample_proposal_voted_drawn(Z, m, Rv, miss_likelihood, step));
        CSLAM_TRY(resample_local_drawn(step, n_eff, status, nullptr, nullptr));
        return add_features_voted(Rv, q_out);
    }

    // ------------------------------------------------------------------------------------------------
    // The control run (test/main.cpp:279-286, pf_control_kernels.hpp): k x (PF::predict, PF::observeHeading) for every
    // owned particle in one launch per kPfControlMax steps, and the whole-cycle calls that put it in front of a scan.
    // Poses change, slots and the feature count do not: the staging memo, the association memo and the vote are left as
    // cslam_pf_predict leaves them -- untouched.
    // ------------------------------------------------------------------------------------------------
    int check_control(int k, const double* v, const double* swa, const void* Qv, const double* phi, int use, const char* who)
    {
        switch (pf_control_check(k, v != nullptr, swa != nullptr, Qv != nullptr, phi != nullptr, use != 0))
        {
        case PfControlRefusal::none:
            return CSLAM_OK;
        case PfControlRefusal::bad_k:
            return fail(CSLAM_ERR_BAD_ARG, "%s: k=%d control steps", who, k);
        case PfControlRefusal::null_control:
            return fail(CSLAM_ERR_BAD_ARG, "%s: v, swa or Q is null (k=%d)", who, k);
        case PfControlRefusal::null_phi:
            break;
        }
        return fail(CSLAM_ERR_BAD_ARG, "%s: the heading is observed and phi is null (k=%d)", who, k);
    }
    // the launches of a checked run; every value is cast to T as cslam_pf_predict and cslam_pf_observe_heading cast it
    int launch_control_run(int k, const double* v, const double* swa, const void* Qv, double wb, double dt, const double* phi,
                           int use)
    {
        static_assert(kPfControlMax == kPfControlChunk, "the chunk split is that of the kernel");
        const T* Q     = static_cast<const T*>(Qv);
        const T  sigma = (T)(((double)0.01f * kPi) / 180.0); // PF.cpp:391
        int      first = 0, count = 0;
        for (int c = 0; pf_control_chunk(k, c, &first, &count); c++)
        {
            PfControls<T> ctl;
            std::memset(&ctl, 0, sizeof(ctl));
            for (int j = 0; j < count; j++)
            {
                ctl.v[j]   = (T)v[first + j];
                ctl.swa[j] = (T)swa[first + j];
                ctl.phi[j] = use ? (T)phi[first + j] : (T)0;
            }
            hipLaunchKernelGGL(pf_control_run_kernel<T>, dim3((np + 63) / 64), dim3(64), 0, stream, store(), count, ctl,
                               Q[0], Q[1], Q[2], Q[3], (T)wb, (T)dt, use ? 1 : 0, sigma * sigma);
            CSLAM_HIP_TRY(hipGetLastError());
            control_launches++;
        }
        return CSLAM_OK;
    }

    int control_run(int k, const double* v, const double* swa, const void* Qv, double wb, double dt, const double* phi,
                    int use) override
    {
        CSLAM_TRY(check_control(k, v, swa, Qv, phi, use, "pf_control_run"));
        if (k == 0)
        {
            return CSLAM_OK;
        }
        CSLAM_TRY(use_device());
        return launch_control_run(k, v, swa, Qv, wb, dt, phi, use);
    }

    // One iteration block of the reference's loop with known correspondences for a handle that holds the whole seeded
    // set: the control run, then the scan of test/main.cpp:294-328 WITHOUT a predict of its own, on the kernels of the
    // separate calls.  Everything that can refuse does so before the control run is launched.  Z of the known and of the
    // new features travel together as the producer kernel's arguments while they fit (mf + mn <= kPfDrawObsMax): the new
    // ones lie behind the known ones in the staging area until pf_add_features_kernel reads them, behind the resample.
    int cycle_drawn(int k, const double* v, const double* swa, const void* Qv, double wb, double dt, const double* phi,
                    int use, const void* ZF, int mf, const int* idf, const void* ZN, int mn, const void* Rv, long long step,
                    double n_eff, int status) override
    {
        const char* who = "pf_cycle_drawn";
        CSLAM_TRY(check_control(k, v, swa, Qv, phi, use, who));
        if (mf < 0 || mn < 0 || (mf > 0 && (!ZF || !idf)) || (mn > 0 && !ZN) || ((mf > 0 || mn > 0) && !Rv))
        {
            return fail(CSLAM_ERR_BAD_ARG, "%s: bad arguments (mf=%d, mn=%d)", who, mf, mn);
        }
        if (mf > 0)
        {
            CSLAM_TRY(need_whole_set(who));
            CSLAM_TRY(check_idf(idf, mf, who));
            if (mn > nfcap - nf)
            {
                return fail(CSLAM_ERR_CAPACITY, "%s: %d features would exceed max_features=%d", who, nf + mn, nfcap);
            }
        }
        else if (mn > 0)
        {
            CSLAM_TRY(check_new_features(ZN, mn, Rv, true, who));
            CSLAM_TRY(need_draws(who));
        }
        CSLAM_TRY(use_device());
        const bool together = mf > 0 && mn > 0 && mf + mn <= kPfDrawObsMax;
        if (mf > 0 || mn > 0)
        {
            CSLAM_TRY(ensure_m(together ? mf + mn : std::max(mf, mn)));
        }
        if (mf > 0)
        {
            CSLAM_TRY(rs.ensure(np, stream));
        }
        CSLAM_TRY(launch_control_run(k, v, swa, Qv, wb, dt, phi, use));
        if (mf == 0)
        {
            if (mn == 0)
            {
                return CSLAM_OK;
            }
            CSLAM_TRY(stage_drawn(ZN, mn, nullptr, step));
            return launch_new_feature_step(0.0, 0.0, nullptr, 0.0, 0.0, mn, Rv);
        }
        const T* R = static_cast<const T*>(Rv);
        obs.forget();
        if (together)
        {
            T   zz[2 * kPfDrawObsMax];
            int ii[kPfDrawObsMax];
            std::memset(ii, 0, sizeof(ii));
            std::memcpy(zz, ZF, (size_t)2 * mf * sizeof(T));
            std::memcpy(zz + 2 * mf, ZN, (size_t)2 * mn * sizeof(T));
            std::memcpy(ii, idf, (size_t)mf * sizeof(int));
            CSLAM_TRY(launch_draw(step, obs.dNormals(), obs.dSelect(), np, mf + mn, zz, ii));
        }
        else
        {
            const bool by_copy = mf > kPfDrawObsMax;
            if (by_copy)
            {
                CSLAM_TRY(stage(ZF, mf, idf));
            }
            CSLAM_TRY(launch_draw(step, obs.dNormals(), obs.dSelect(), np, by_copy ? 0 : mf, ZF, idf));
        }
        // the feature update rides in the proposal unless the list names a feature twice (launch_observation_step)
        const int fu = pf_has_duplicate(idf, mf) ? 0 : fused_update_gain();
        CSLAM_TRY(launch_proposal(mf, R, no_predict(), fu));
        if (fu == 0)
        {
            CSLAM_TRY(launch_feature_update(mf, R));
        }
        CSLAM_TRY(launch_resample(obs.dSelect(), n_eff, status));
        if (mn > 0)
        {
            const T* zn = obs.z() + 2 * mf;
            if (!together)
            {
                if (mn > kPfDrawObsMax)
                {
                    CSLAM_TRY(stage(ZN, mn, nullptr));
                }
                else // (a producer launch that only carries Z: no draw is taken)
                {
                    CSLAM_TRY(launch_draw(step, nullptr, nullptr, 0, mn, ZN, nullptr));
                }
                zn = obs.z();
            }
            hipLaunchKernelGGL(pf_add_features_kernel<T>, dim3((np + 63) / 64, mn), dim3(64), 0, stream, store(), zn, mn,
                               R[0], R[1], R[2], R[3]);
            CSLAM_HIP_TRY(hipGetLastError());
            nf += mn;
        }
        obs.forget(); // (the area holds this cycle's mix, not the Z || idf of one call)
        return CSLAM_OK;
    }

    // The control run followed by the body of assoc_scan_step_drawn behind its predict: associate + vote, the proposal on
    // the vote's mask, the resample with nothing returned, and only then the wait for the vote and its features.
    int assoc_cycle_drawn(int k, const double* v, const double* swa, const void* Qv, double wb, double dt, const double* phi,
                          int use, const void* Z, int m, const void* Rv, double gate1, double gate2, double new_fraction,
                          double miss_likelihood, long long step, double n_eff, int status, int* q_out) override
    {
        const char* who = "pf_assoc_cycle_drawn";
        CSLAM_TRY(check_control(k, v, swa, Qv, phi, use, who));
        if (m < 0 || m > 65535 || (m > 0 && (!Z || !Rv)) || !std::isfinite(gate1) || !std::isfinite(gate2) ||
            !std::isfinite(new_fraction) || !std::isfinite(miss_likelihood))
        {
            return fail(CSLAM_ERR_BAD_ARG, "%s: bad arguments (m=%d)", who, m);
        }
        CSLAM_TRY(need_whole_set(who));
        CSLAM_TRY(use_device());
        if (m > 0) // what can fail for want of memory, before anything is launched
        {
            CSLAM_TRY(ensure_m(m));
            CSLAM_TRY(vote.ensure(m, false, stream));
            CSLAM_TRY(assoc.ensure(m, (nf + kPfAssocFeatChunk - 1) / kPfAssocFeatChunk, np, stream));
            CSLAM_TRY(rs.ensure(np, stream));
        }
        if (q_out)
        {
            *q_out = 0;
        }
        CSLAM_TRY(launch_control_run(k, v, swa, Qv, wb, dt, phi, use));
        if (m == 0)
        {
            return CSLAM_OK;
        }
        CSLAM_TRY(associate_vote(nullptr, Z, m, Rv, gate1, gate2, new_fraction));
        CSLAM_TRY(sample_proposal_voted_drawn(Z, m, Rv, miss_likelihood, step));
        CSLAM_TRY(resample_local_drawn(step, n_eff, status, nullptr, nullptr));
        return add_features_voted(Rv, q_out);
    }
    // ------------------------------------------------------------------------------------------------
    // The FastSLAM-1 step (pf_fs1_kernels.hpp): the control run with every particle's own noisy controls (slam.h:149-159,
    // PF.cpp:419-471, 382-417), the likelihood weights with the feature update riding along (PF.cpp:343-359, 222-277), and
    // the iteration block made of them (test/main.cpp:249-334 with the proposal switched off, slam.h:102).  Every refusal
    // is decided by the plain functions of pf_host_parts.hpp before the first launch.  Slots do not move in the first two
    // calls: the association memo and the vote are left as cslam_pf_predict and cslam_pf_feature_update leave them.
    // ------------------------------------------------------------------------------------------------
    int refuse_fs1(PfFs1Refusal r, const char* who, int k, long long ctl_step, const int* idf, int index, int mf,
                   int mn)
    {
        switch (r)
        {
        case PfFs1Refusal::none:
            return CSLAM_OK;
        case PfFs1Refusal::bad_k:
            return fail(CSLAM_ERR_BAD_ARG, "%s: k=%d control steps", who, k);
        case PfFs1Refusal::null_control:
            return fail(CSLAM_ERR_BAD_ARG, "%s: v, swa, Q or the output is null (k=%d)", who, k);
        case PfFs1Refusal::null_phi:
            return fail(CSLAM_ERR_BAD_ARG, "%s: the heading is observed and phi is null (k=%d)", who, k);
        case PfFs1Refusal::bad_step:
            return fail(CSLAM_ERR_BAD_ARG, "%s: ctl_step=%lld", who, ctl_step);
        case PfFs1Refusal::bad_q:
            return fail(CSLAM_ERR_BAD_ARG, "%s: Q[0,0] and Q[1,1] must not be negative", who);
        case PfFs1Refusal::bad_idf:
            return fail(CSLAM_ERR_BAD_ARG, "%s: idf[%d]=%d outside 1..%d", who, index, idf[index], nf);
        case PfFs1Refusal::capacity:
            return fail(CSLAM_ERR_CAPACITY, "%s: %d features would exceed max_features=%d", who, nf + mn, nfcap);
        case PfFs1Refusal::bad_scan:
            break;
        }
        return fail(CSLAM_ERR_BAD_ARG, "%s: bad arguments (mf=%d, mn=%d: a negative count, or observations without Z, idf or R)", who,
                    mf, mn);
    }
    int check_fs1_control(int k, const double* v, const double* swa, const void* Qv, const double* phi, int use,
                          long long ctl_step, const char* who)
    {
        const T*     Q      = static_cast<const T*>(Qv);
        const double qd[2]  = {Q ? (double)Q[0] : 0.0, Q ? (double)Q[3] : 0.0};
        return refuse_fs1(pf_fs1_control_check(k, v != nullptr, swa != nullptr, Q ? qd : nullptr, phi != nullptr, use != 0,
                                               ctl_step),
                          who, k, ctl_step, nullptr, -1, 0, 0);
    }
    // the launches of a checked sampled run: launch_control_run's chunks, chunk c from control step ctl_step + 16 c
    int launch_control_run_sampled(int k, const double* v, const double* swa, const void* Qv, double wb, double dt,
                                   const double* phi, int use, long long ctl_step)
    {
        const T* Q     = static_cast<const T*>(Qv);
        const T  sigma = (T)(((double)0.01f * kPi) / 180.0); // PF.cpp:391
        int      first = 0, count = 0;
        for (int c = 0; pf_control_chunk(k, c, &first, &count); c++)
        {
            PfControls<T> ctl;
            std::memset(&ctl, 0, sizeof(ctl));
            for (int j = 0; j < count; j++)
            {
                ctl.v[j]   = (T)v[first + j];
                ctl.swa[j] = (T)swa[first + j];
                ctl.phi[j] = use ? (T)phi[first + j] : (T)0;
            }
            const PfControlNoise<T> nz{pf_control_seed(draws.seed), (unsigned long long)pf_fs1_chunk_step(ctl_step, c),
                                       (unsigned long long)draws.first, std::sqrt(Q[0]), std::sqrt(Q[3])};
            hipLaunchKernelGGL(pf_control_run_sampled_kernel<T>, dim3((np + 63) / 64), dim3(64), 0, stream, store(), count,
                               ctl, nz, Q[0], Q[1], Q[2], Q[3], (T)wb, (T)dt, use ? 1 : 0, sigma * sigma);
            CSLAM_HIP_TRY(hipGetLastError());
            control_launches++;
        }
        return CSLAM_OK;
    }

    int control_run_sampled(int k, const double* v, const double* swa, const void* Qv, double wb, double dt,
                            const double* phi, int use, long long ctl_step) override
    {
        const char* who = "pf_control_run_sampled";
        CSLAM_TRY(check_fs1_control(k, v, swa, Qv, phi, use, ctl_step, who));
        CSLAM_TRY(need_draws(who));
        if (k == 0)
        {
            return CSLAM_OK;
        }
        CSLAM_TRY(use_device());
        return launch_control_run_sampled(k, v, swa, Qv, wb, dt, phi, use, ctl_step);
    }

    // normals [k][2][np]: one launch and one copy per control step through the buffer of cslam_pf_get_draws
    int get_control_draws(long long ctl_step, int k, void* normals) override
    {
        const char* who = "pf_get_control_draws";
        CSLAM_TRY(refuse_fs1(pf_fs1_draws_check(k, ctl_step, normals != nullptr), who, k, ctl_step, nullptr, -1, 0, 0));
        CSLAM_TRY(need_draws(who));
        if (k == 0)
        {
            return CSLAM_OK;
        }
        CSLAM_TRY(use_device());
        T*           dn    = draws.out.get(); // (3 np + strata elements: room for 2 np)
        const size_t bytes = (size_t)2 * np * sizeof(T);
        for (int j = 0; j < k; j++)
        {
            hipLaunchKernelGGL(pf_control_draws_kernel<T>, dim3((np + 255) / 256), dim3(256), 0, stream,
                               pf_control_seed(draws.seed), (unsigned long long)(ctl_step + j),
                               (unsigned long long)draws.first, dn, np);
            CSLAM_HIP_TRY(hipGetLastError());
            CSLAM_HIP_TRY(hipMemcpyAsync(static_cast<char*>(normals) + (size_t)j * bytes, dn, bytes, hipMemcpyDeviceToHost,
                                         stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    // behind Z | idf in the staging area; the update rides unless the list names a feature twice (cycle_drawn's rule)
    int launch_likelihood_update(int m, const int* idf, const T* R, int update_features, int zero_pv)
    {
        const int fu = (update_features && !pf_has_duplicate(idf, m)) ? fused_update_gain() : 0;
        hipLaunchKernelGGL(pf_likelihood_update_kernel<T>, dim3((np + 63) / 64), dim3(64, kPfFs1Obs), 0, stream, store(),
                           obs.z(), obs.dIdf(), m, R[0], R[1], R[2], R[3], fu, zero_pv ? 1 : 0);
        CSLAM_HIP_TRY(hipGetLastError());
        if (update_features && fu == 0)
        {
            CSLAM_TRY(launch_feature_update(m, R));
        }
        return CSLAM_OK;
    }

    int likelihood_update(const void* Z, int m, const int* idf, const void* Rv, int update_features, int zero_pv) override
    {
        const char* who   = "pf_likelihood_update";
        int         index = -1;
        // (pf_fs1_scan_check is the whole rule: counts, NULLs -- R only where it is read -- and idf within 1..nf)
        CSLAM_TRY(refuse_fs1(pf_fs1_scan_check(m, Z != nullptr, idf, 0, false, Rv != nullptr, nf, nfcap, &index), who, 0, 0, idf,
                             index, m, 0));
        if (m == 0)
        {
            return CSLAM_OK;
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(stage(Z, m, idf));
        return launch_likelihood_update(m, idf, static_cast<const T*>(Rv), update_features, zero_pv);
    }

    // One iteration block of the FastSLAM-1 loop for a handle that holds the whole seeded set: the sampled run, then --
    // known features seen -- the likelihood weights with the feature update and Pv = 0, the resample on the strata of
    // `step`, and the new features at every particle's own pose (the particle IS the sample: no pose is drawn).  Z of
    // the known and of the new features travel as cycle_drawn sends them.
    int fs1_cycle_drawn(int k, const double* v, const double* swa, const void* Qv, double wb, double dt, const double* phi,
                        int use, long long ctl_step, const void* ZF, int mf, const int* idf, const void* ZN, int mn,
                        const void* Rv, long long step, double n_eff, int status) override
    {
        const char* who   = "pf_fs1_cycle_drawn";
        int         index = -1;
        CSLAM_TRY(check_fs1_control(k, v, swa, Qv, phi, use, ctl_step, who));
        CSLAM_TRY(need_whole_set(who));
        CSLAM_TRY(refuse_fs1(pf_fs1_scan_check(mf, ZF != nullptr, idf, mn, ZN != nullptr, Rv != nullptr, nf, nfcap, &index), who,
                             k, ctl_step, idf, index, mf, mn));
        CSLAM_TRY(use_device());
        const bool together = mf > 0 && mn > 0 && mf + mn <= kPfDrawObsMax;
        if (mf > 0 || mn > 0)
        {
            CSLAM_TRY(ensure_m(together ? mf + mn : std::max(mf, mn)));
        }
        if (mf > 0)
        {
            CSLAM_TRY(rs.ensure(np, stream));
        }
        CSLAM_TRY(launch_control_run_sampled(k, v, swa, Qv, wb, dt, phi, use, ctl_step));
        if (mf == 0 && mn == 0)
        {
            return CSLAM_OK;
        }
        const T* R = static_cast<const T*>(Rv);
        obs.forget();
        const T* zn = obs.z();
        if (mf > 0)
        {
            if (together)
            {
                T   zz[2 * kPfDrawObsMax];
                int ii[kPfDrawObsMax];
                std::memset(ii, 0, sizeof(ii));
                std::memcpy(zz, ZF, (size_t)2 * mf * sizeof(T));
                std::memcpy(zz + 2 * mf, ZN, (size_t)2 * mn * sizeof(T));
                std::memcpy(ii, idf, (size_t)mf * sizeof(int));
                CSLAM_TRY(launch_draw(step, nullptr, obs.dSelect(), np, mf + mn, zz, ii));
                zn = obs.z() + 2 * mf;
            }
            else
            {
                const bool by_copy = mf > kPfDrawObsMax;
                if (by_copy)
                {
                    CSLAM_TRY(stage(ZF, mf, idf));
                }
                CSLAM_TRY(launch_draw(step, nullptr, obs.dSelect(), np, by_copy ? 0 : mf, ZF, idf));
            }
            CSLAM_TRY(launch_likelihood_update(mf, idf, R, 1, 1));
            CSLAM_TRY(launch_resample(obs.dSelect(), n_eff, status));
        }
        if (mn > 0)
        {
            if (!together)
            {
                if (mn > kPfDrawObsMax)
                {
                    CSLAM_TRY(stage(ZN, mn, nullptr));
                }
                else // (a producer launch that only carries Z: no draw is taken)
                {
                    CSLAM_TRY(launch_draw(step, nullptr, nullptr, 0, mn, ZN, nullptr));
                }
            }
            hipLaunchKernelGGL(pf_add_features_kernel<T>, dim3((np + 63) / 64, mn), dim3(64), 0, stream, store(), zn, mn,
                               R[0], R[1], R[2], R[3]);
            CSLAM_HIP_TRY(hipGetLastError());
            nf += mn;
        }
        obs.forget(); // (the area holds this cycle's mix, not the Z || idf of one call)
        return CSLAM_OK;
    }
};

inline PfBase* B(cslam_pf_t h)
{
    return reinterpret_cast<PfBase*>(h);
}

} // namespace

extern "C" {

#define CSLAM_NEED(h)                                                \
    if (!(h))                                                        \
    {                                                                \
        return fail(CSLAM_ERR_BAD_ARG, "%s: null handle", __func__); \
    }

int cslam_pf_create(int n_particles, int max_features, int dtype, int device, int quirks, cslam_pf_t* out)
{
    if (!out || n_particles < 1 || max_features < 0 || (dtype != CSLAM_F32 && dtype != CSLAM_F64) ||
        (quirks & ~CSLAM_Q_REF_EXACT))
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_create: bad arguments");
    }
    *out  = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
    {
        return fail(CSLAM_ERR_NO_DEVICE, "pf_create: no HIP device (this engine has no CPU fallback)");
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess)
    {
        device = 0;
    }
    if (device >= c)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_create: device %d of %d", device, c);
    }
    PfBase* b = (dtype == CSLAM_F32) ? static_cast<PfBase*>(new (std::nothrow) Pf<float>())
                                     : static_cast<PfBase*>(new (std::nothrow) Pf<double>());
    if (!b)
    {
        return fail(CSLAM_ERR_ALLOC, "pf_create: out of host memory");
    }
    b->dtype  = dtype;
    b->device = device;
    b->quirks = quirks;
    b->np     = n_particles;
    b->nfcap  = max_features;
    int rc    = b->init();
    if (rc)
    {
        delete b;
        return rc;
    }
    *out = reinterpret_cast<cslam_pf_t>(b);
    return CSLAM_OK;
}

int cslam_pf_destroy(cslam_pf_t h)
{
    if (!h)
    {
        return CSLAM_OK;
    }
    (void)hipSetDevice(B(h)->device);
    delete B(h);
    return CSLAM_OK;
}

int cslam_pf_synchronize(cslam_pf_t h)
{
    CSLAM_NEED(h);
    CSLAM_HIP_TRY(hipSetDevice(B(h)->device));
    CSLAM_HIP_TRY(hipStreamSynchronize(B(h)->stream));
    return CSLAM_OK;
}

int cslam_pf_get_stream(cslam_pf_t h, void** stream)
{
    CSLAM_NEED(h);
    if (!stream)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_get_stream: null");
    }
    *stream = reinterpret_cast<void*>(B(h)->stream);
    return CSLAM_OK;
}

int cslam_pf_get_counts(cslam_pf_t h, int* n_particles, int* n_features)
{
    CSLAM_NEED(h);
    if (n_particles)
    {
        *n_particles = B(h)->np;
    }
    if (n_features)
    {
        *n_features = B(h)->nf;
    }
    return CSLAM_OK;
}

int cslam_pf_set_uniform_weight(cslam_pf_t h, double w0)
{
    CSLAM_NEED(h);
    return B(h)->set_uniform_weight(w0);
}

int cslam_pf_predict(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt)
{
    CSLAM_NEED(h);
    return B(h)->predict(v, swa, Q, wb, dt);
}

int cslam_pf_observe_heading(cslam_pf_t h, double phi, int use_heading)
{
    CSLAM_NEED(h);
    return B(h)->observe_heading(phi, use_heading);
}

int cslam_pf_sample_proposal(cslam_pf_t h, const void* Z, int m, const int* idf, const void* R, const void* normals)
{
    CSLAM_NEED(h);
    return B(h)->sample_proposal(Z, m, idf, R, normals);
}

int cslam_pf_feature_update(cslam_pf_t h, const void* Z, int m, const int* idf, const void* R)
{
    CSLAM_NEED(h);
    return B(h)->feature_update(Z, m, idf, R);
}

int cslam_pf_add_features(cslam_pf_t h, const void* Z, int q, const void* R)
{
    CSLAM_NEED(h);
    return B(h)->add_features(Z, q, R);
}

int cslam_pf_weight_sums(cslam_pf_t h, double* sums)
{
    CSLAM_NEED(h);
    return B(h)->weight_sums(sums);
}

int cslam_pf_scale_weights(cslam_pf_t h, double scale)
{
    CSLAM_NEED(h);
    return B(h)->scale_weights(scale);
}

int cslam_pf_set_degenerate_policy(cslam_pf_t h, int policy)
{
    CSLAM_NEED(h);
    return B(h)->set_degenerate_policy(policy);
}

int cslam_pf_divide_weights(cslam_pf_t h, double ws)
{
    CSLAM_NEED(h);
    return B(h)->divide_weights(ws);
}

int cslam_pf_weights_device_ptr(cslam_pf_t h, void** dptr)
{
    CSLAM_NEED(h);
    return B(h)->weights_ptr(dptr);
}

int cslam_pf_get_weights(cslam_pf_t h, void* w_host)
{
    CSLAM_NEED(h);
    return B(h)->get_weights(w_host);
}

int cslam_pf_set_weights(cslam_pf_t h, const void* w_host)
{
    CSLAM_NEED(h);
    return B(h)->set_weights(w_host);
}

int cslam_pf_record_bytes(cslam_pf_t h, long long* bytes)
{
    CSLAM_NEED(h);
    return B(h)->record_bytes(bytes);
}

int cslam_pf_pack(cslam_pf_t h, const int* src_idx, int count, void* d_records)
{
    CSLAM_NEED(h);
    return B(h)->pack(src_idx, count, d_records);
}

int cslam_pf_unpack(cslam_pf_t h, const int* dst_idx, int count, const void* d_records)
{
    CSLAM_NEED(h);
    return B(h)->unpack(dst_idx, count, d_records);
}

int cslam_pf_resample_local(cslam_pf_t h, const void* select, double n_effective, int resample_status, double* neff,
                            int* resampled)
{
    CSLAM_NEED(h);
    return B(h)->resample_local(select, n_effective, resample_status, neff, resampled);
}

int cslam_pf_gather_local(cslam_pf_t h, const int* keep, double w_new)
{
    CSLAM_NEED(h);
    if (!keep)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_gather_local: null");
    }
    return B(h)->gather_local(keep, w_new);
}

int cslam_pf_get_particle(cslam_pf_t h, int index, void* w, void* Xv, void* Pv, void* XF, void* PF)
{
    CSLAM_NEED(h);
    return B(h)->get_particle(index, w, Xv, Pv, XF, PF);
}

int cslam_pf_set_particle(cslam_pf_t h, int index, const void* w, const void* Xv, const void* Pv, const void* XF,
                          const void* PF, int nf)
{
    CSLAM_NEED(h);
    return B(h)->set_particle(index, w, Xv, Pv, XF, PF, nf);
}

int cslam_pf_observation_step(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt, const void* Z, int m,
                              const int* idf, const void* R, const void* normals, const void* select, double n_effective,
                              int resample_status)
{
    CSLAM_NEED(h);
    return B(h)->observation_step(v, swa, Q, wb, dt, Z, m, idf, R, normals, select, n_effective, resample_status);
}

int cslam_pf_resample_stats(cslam_pf_t h, double* calls, double* resamples, double* last_neff)
{
    CSLAM_NEED(h);
    return B(h)->resample_stats(calls, resamples, last_neff);
}

int cslam_comm_unique_id(void* id_bytes)
{
    if (!id_bytes)
    {
        return fail(CSLAM_ERR_BAD_ARG, "comm_unique_id: null");
    }
    Rccl* R = rccl();
    if (!R)
    {
        return fail(CSLAM_ERR_HIP, "comm_unique_id: librccl could not be loaded");
    }
    static_assert(sizeof(ncclUniqueId) == CSLAM_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    CSLAM_RCCL_TRY(R->GetUniqueId(&id));
    std::memcpy(id_bytes, &id, sizeof(id));
    return CSLAM_OK;
}

int cslam_comm_create(const void* id_bytes, int rank, int world, int device, cslam_comm_t* out)
{
    if (!id_bytes || !out || world < 1 || rank < 0 || rank >= world)
    {
        return fail(CSLAM_ERR_BAD_ARG, "comm_create: bad arguments");
    }
    *out    = nullptr;
    Rccl* R = rccl();
    if (!R)
    {
        return fail(CSLAM_ERR_HIP, "comm_create: librccl could not be loaded");
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess)
    {
        device = 0;
    }
    CSLAM_HIP_TRY(hipSetDevice(device));
    Comm* c = new (std::nothrow) Comm();
    if (!c)
    {
        return fail(CSLAM_ERR_ALLOC, "comm_create: out of host memory");
    }
    ncclUniqueId id;
    std::memcpy(&id, id_bytes, sizeof(id));
    ncclResult_t r = R->CommInitRank(&c->comm, world, id, rank);
    if (r != ncclSuccess)
    {
        delete c;
        return fail(CSLAM_ERR_HIP, "ncclCommInitRank failed: %s", R->GetErrorString ? R->GetErrorString(r) : "rccl error");
    }
    c->rank   = rank;
    c->world  = world;
    c->device = device;
    *out      = reinterpret_cast<cslam_comm_t>(c);
    return CSLAM_OK;
}

int cslam_comm_create_loopback(int world, int device, cslam_comm_t* out)
{
    if (!out || world < 1 || world > kLoopMaxWorld)
    {
        return fail(CSLAM_ERR_BAD_ARG, "comm_create_loopback: world must be 1..%d", kLoopMaxWorld);
    }
    for (int r = 0; r < world; r++)
    {
        out[r] = nullptr;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess)
    {
        device = 0;
    }
    LoopShared* sh = new (std::nothrow) LoopShared();
    if (!sh)
    {
        return fail(CSLAM_ERR_ALLOC, "comm_create_loopback: out of host memory");
    }
    sh->world = world;
    sh->refs  = world;
    sh->src.assign((size_t)world, nullptr);
    sh->sends.assign((size_t)world * world, LoopShared::P2P{});
    for (int r = 0; r < world; r++)
    {
        Comm* c = new (std::nothrow) Comm();
        if (!c)
        {
            for (int q = 0; q < r; q++)
            {
                delete reinterpret_cast<Comm*>(out[q]);
                out[q] = nullptr;
            }
            delete sh;
            return fail(CSLAM_ERR_ALLOC, "comm_create_loopback: out of host memory");
        }
        c->loop   = sh;
        c->rank   = r;
        c->world  = world;
        c->device = device;
        out[r]    = reinterpret_cast<cslam_comm_t>(c);
    }
    return CSLAM_OK;
}

int cslam_comm_destroy(cslam_comm_t c)
{
    if (!c)
    {
        return CSLAM_OK;
    }
    Comm* cc = reinterpret_cast<Comm*>(c);
    if (cc->loop)
    {
        bool last = false;
        {
            std::lock_guard<std::mutex> lk(cc->loop->mu);
            last = (--cc->loop->refs == 0);
        }
        if (last)
        {
            delete cc->loop;
        }
    }
    else if (Rccl* R = rccl())
    {
        (void)R->CommDestroy(cc->comm);
    }
    delete cc;
    return CSLAM_OK;
}

int cslam_comm_info(cslam_comm_t c, int* rank, int* world)
{
    if (!c)
    {
        return fail(CSLAM_ERR_BAD_ARG, "comm_info: null communicator");
    }
    const Comm* cc = reinterpret_cast<const Comm*>(c);
    if (rank)
    {
        *rank = cc->rank;
    }
    if (world)
    {
        *world = cc->world;
    }
    return CSLAM_OK;
}

int cslam_pf_debug_last_exchange(cslam_pf_t h, int* counts, int* send_idx, int capacity, int* n_send)
{
    CSLAM_NEED(h);
    return B(h)->debug_last_exchange(counts, send_idx, capacity, n_send);
}

int cslam_pf_resample_sharded(cslam_pf_t h, cslam_comm_t comm, const void* select, double n_effective,
                              int resample_status, double* neff, int* resampled)
{
    CSLAM_NEED(h);
    return B(h)->resample_sharded(reinterpret_cast<Comm*>(comm), select, n_effective, resample_status, neff, resampled);
}

int cslam_pf_best_particle(cslam_pf_t h, int pick, int* index, void* w, void* Xv, void* Pv, void* XF, void* PF)
{
    CSLAM_NEED(h);
    long long i  = 0;
    const int rc = B(h)->best_particle(nullptr, pick, &i, w, Xv, Pv, XF, PF);
    if (rc == CSLAM_OK && index)
    {
        *index = (int)i;
    }
    return rc;
}

int cslam_pf_estimate(cslam_pf_t h, double* w_sum, double* neff, void* Xv, void* Pv, void* XF, void* PF)
{
    CSLAM_NEED(h);
    return B(h)->estimate(nullptr, w_sum, neff, Xv, Pv, XF, PF);
}

int cslam_pf_get_all_features(cslam_pf_t h, void* XF_all)
{
    CSLAM_NEED(h);
    return B(h)->get_all_features(XF_all);
}

/* the score of the estimate test/main.cpp:330 prints (slam.h:493-511; the map: slam.h:513-539), kept on the device */
int cslam_pf_score_reset(cslam_pf_t h, int estimator, int series_capacity, double gate_pose, double gate_lm)
{
    CSLAM_NEED(h);
    return B(h)->score_reset(estimator, series_capacity, gate_pose, gate_lm);
}

int cslam_pf_score_set_truth(cslam_pf_t h, const double* lm_true, int count)
{
    CSLAM_NEED(h);
    return B(h)->score_set_truth(lm_true, count);
}

int cslam_pf_score(cslam_pf_t h, const double* xv_true, int with_map)
{
    CSLAM_NEED(h);
    return B(h)->score(nullptr, xv_true, with_map);
}

int cslam_pf_score_sharded(cslam_pf_t h, cslam_comm_t comm, const double* xv_true, int with_map)
{
    CSLAM_NEED(h);
    if (!comm)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_score_sharded: null communicator");
    }
    return B(h)->score(reinterpret_cast<Comm*>(comm), xv_true, with_map);
}

int cslam_pf_get_scores(cslam_pf_t h, double* totals, float* series, double* track, int capacity_records, int* records,
                        long long* calls)
{
    CSLAM_NEED(h);
    return B(h)->get_scores(totals, series, track, capacity_records, records, calls);
}

/* EKF.cpp:131-144, 235-326 on every particle's own state */
int cslam_pf_associate(cslam_pf_t h, const void* Z, int m, const void* R, double gate1, double gate2)
{
    CSLAM_NEED(h);
    return B(h)->associate(Z, m, R, gate1, gate2);
}

/* the tables of the last associate (EKF.cpp:131-144, 235-326 per particle) */
int cslam_pf_get_association(cslam_pf_t h, int* idf_host, int* kind_host, double* summary_host)
{
    CSLAM_NEED(h);
    return B(h)->get_association(idf_host, kind_host, summary_host);
}

/* PF.cpp:502-544 + 222-277 with every particle's own correspondences (EKF.cpp:131-144, 235-326) */
int cslam_pf_sample_proposal_assoc(cslam_pf_t h, const void* Z, int m, const void* R, const void* normals, const int* use,
                                   double miss_likelihood)
{
    CSLAM_NEED(h);
    return B(h)->sample_proposal_assoc(Z, m, R, normals, use, miss_likelihood);
}

/* PF.cpp:222-277 alone with every particle's own correspondences (EKF.cpp:131-144, 235-326) */
int cslam_pf_feature_update_assoc(cslam_pf_t h, const void* Z, int m, const void* R, const int* use)
{
    CSLAM_NEED(h);
    return B(h)->feature_update_assoc(Z, m, R, use);
}

/* slam.h:587-594: the seed of every draw the _drawn calls make */
int cslam_pf_seed_draws(cslam_pf_t h, long long seed, long long first_global, long long n_global)
{
    CSLAM_NEED(h);
    return B(h)->seed_draws(seed, first_global, n_global);
}

/* slam.h:753-764 and PF.cpp:557, 579-596 of one step, read back */
int cslam_pf_get_draws(cslam_pf_t h, long long step, void* normals, void* select)
{
    CSLAM_NEED(h);
    return B(h)->get_draws(step, normals, select);
}

/* PF.cpp:502-544 with the normals of slam.h:753-764 drawn on the device */
int cslam_pf_sample_proposal_drawn(cslam_pf_t h, const void* Z, int m, const int* idf, const void* R, long long step)
{
    CSLAM_NEED(h);
    return B(h)->sample_proposal_drawn(Z, m, idf, R, step);
}

int cslam_pf_sample_proposal_assoc_drawn(cslam_pf_t h, const void* Z, int m, const void* R, const int* use,
                                         double miss_likelihood, long long step)
{
    CSLAM_NEED(h);
    return B(h)->sample_proposal_assoc_drawn(Z, m, R, use, miss_likelihood, step);
}

/* PF.cpp:473-500 with the strata of PF.cpp:557, 579-596 drawn on the device */
int cslam_pf_resample_local_drawn(cslam_pf_t h, long long step, double n_effective, int resample_status, double* neff,
                                  int* resampled)
{
    CSLAM_NEED(h);
    return B(h)->resample_local_drawn(step, n_effective, resample_status, neff, resampled);
}

int cslam_pf_resample_sharded_drawn(cslam_pf_t h, cslam_comm_t comm, long long step, double n_effective,
                                    int resample_status, double* neff, int* resampled)
{
    CSLAM_NEED(h);
    return B(h)->resample_sharded_drawn(reinterpret_cast<Comm*>(comm), step, n_effective, resample_status, neff, resampled);
}

int cslam_pf_observation_step_drawn(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt,
                                    const void* Z, int m, const int* idf, const void* R, long long step,
                                    double n_effective, int resample_status)
{
    CSLAM_NEED(h);
    return B(h)->observation_step_drawn(v, swa, Q, wb, dt, Z, m, idf, R, step, n_effective, resample_status);
}

int cslam_pf_stage_copies(cslam_pf_t h, long long* copies)
{
    CSLAM_NEED(h);
    return B(h)->get_stage_copies(copies);
}

/* test/main.cpp:321-324: X <- X + chol(P) z (slam.h:753-764, 413-436), P <- 0 */
int cslam_pf_sample_pose(cslam_pf_t h, const void* normals)
{
    CSLAM_NEED(h);
    return B(h)->sample_pose(normals);
}

int cslam_pf_sample_pose_drawn(cslam_pf_t h, long long step)
{
    CSLAM_NEED(h);
    return B(h)->sample_pose_drawn(step);
}

/* test/main.cpp:314-328 behind PF.cpp:419-471: predict, sample the pose, zero Pv, PF.cpp:9-60 at the sampled pose */
int cslam_pf_new_feature_step(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt, const void* Z, int q,
                              const void* R, const void* normals)
{
    CSLAM_NEED(h);
    return B(h)->new_feature_step(v, swa, Q, wb, dt, Z, q, R, normals);
}

int cslam_pf_new_feature_step_drawn(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt, const void* Z,
                                    int q, const void* R, long long step)
{
    CSLAM_NEED(h);
    return B(h)->new_feature_step_drawn(v, swa, Q, wb, dt, Z, q, R, step);
}

int cslam_pf_best_particle_sharded(cslam_pf_t h, cslam_comm_t comm, int pick, long long* global_index, void* w, void* Xv,
                                   void* Pv, void* XF, void* PF)
{
    CSLAM_NEED(h);
    if (!comm)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_best_particle_sharded: null communicator");
    }
    return B(h)->best_particle(reinterpret_cast<Comm*>(comm), pick, global_index, w, Xv, Pv, XF, PF);
}

int cslam_pf_estimate_sharded(cslam_pf_t h, cslam_comm_t comm, double* w_sum, double* neff, void* Xv, void* Pv, void* XF,
                              void* PF)
{
    CSLAM_NEED(h);
    if (!comm)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_estimate_sharded: null communicator");
    }
    return B(h)->estimate(reinterpret_cast<Comm*>(comm), w_sum, neff, Xv, Pv, XF, PF);
}

/* EKF.cpp:131-144, 235-326 on every particle's own state, then the split of test/main.cpp:279-328 voted on the device */
int cslam_pf_associate_vote(cslam_pf_t h, const void* Z, int m, const void* R, double gate1, double gate2, double new_fraction)
{
    CSLAM_NEED(h);
    return B(h)->associate_vote(nullptr, Z, m, R, gate1, gate2, new_fraction);
}

int cslam_pf_associate_vote_sharded(cslam_pf_t h, cslam_comm_t comm, const void* Z, int m, const void* R, double gate1,
                                    double gate2, double new_fraction)
{
    CSLAM_NEED(h);
    if (!comm)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_associate_vote_sharded: null communicator");
    }
    return B(h)->associate_vote(reinterpret_cast<Comm*>(comm), Z, m, R, gate1, gate2, new_fraction);
}

int cslam_pf_vote_wait(cslam_pf_t h, int* q, int* use)
{
    CSLAM_NEED(h);
    return B(h)->vote_wait(q, use);
}

int cslam_pf_get_vote(cslam_pf_t h, int* use, int* new_idx, void* ZN, int* q)
{
    CSLAM_NEED(h);
    return B(h)->get_vote(use, new_idx, ZN, q);
}

/* PF.cpp:502-544 + 222-277 with every particle's own correspondences (EKF.cpp:131-144, 235-326), the mask from the vote */
int cslam_pf_sample_proposal_voted(cslam_pf_t h, const void* Z, int m, const void* R, const void* normals,
                                   double miss_likelihood)
{
    CSLAM_NEED(h);
    return B(h)->sample_proposal_voted(Z, m, R, normals, miss_likelihood);
}

int cslam_pf_sample_proposal_voted_drawn(cslam_pf_t h, const void* Z, int m, const void* R, double miss_likelihood,
                                         long long step)
{
    CSLAM_NEED(h);
    return B(h)->sample_proposal_voted_drawn(Z, m, R, miss_likelihood, step);
}

/* PF.cpp:222-277 alone, the mask from the vote */
int cslam_pf_feature_update_voted(cslam_pf_t h, const void* Z, int m, const void* R)
{
    CSLAM_NEED(h);
    return B(h)->feature_update_voted(Z, m, R);
}

/* PF.cpp:9-60 of the voted observations */
int cslam_pf_add_features_voted(cslam_pf_t h, const void* R, int* q_out)
{
    CSLAM_NEED(h);
    return B(h)->add_features_voted(R, q_out);
}

/* test/main.cpp:279-328 with unknown correspondences in one call */
int cslam_pf_assoc_scan_step_drawn(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt, const void* Z,
                                   int m, const void* R, double gate1, double gate2, double new_fraction,
                                   double miss_likelihood, long long step, double n_effective, int resample_status,
                                   int* q_out)
{
    CSLAM_NEED(h);
    return B(h)->assoc_scan_step_drawn(v, swa, Q, wb, dt, Z, m, R, gate1, gate2, new_fraction, miss_likelihood, step,
                                       n_effective, resample_status, q_out);
}

/* k iterations of test/main.cpp:279-286 (PF.cpp:419-471, 382-417) in one launch per 16 steps */
int cslam_pf_control_run(cslam_pf_t h, int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                         const double* phi, int use_heading)
{
    CSLAM_NEED(h);
    return B(h)->control_run(k, v, swa, Q, wb, dt, phi, use_heading);
}

int cslam_pf_control_launches(cslam_pf_t h, long long* launches)
{
    CSLAM_NEED(h);
    if (!launches)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_control_launches: null");
    }
    *launches = B(h)->control_launches;
    return CSLAM_OK;
}

/* test/main.cpp:249-334: the control steps of one iteration block and its scan with known correspondences, in one call */
int cslam_pf_cycle_drawn(cslam_pf_t h, int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                         const double* phi, int use_heading, const void* ZF, int mf, const int* idf, const void* ZN, int mn,
                         const void* R, long long step, double n_effective, int resample_status)
{
    CSLAM_NEED(h);
    return B(h)->cycle_drawn(k, v, swa, Q, wb, dt, phi, use_heading, ZF, mf, idf, ZN, mn, R, step, n_effective,
                             resample_status);
}

/* the same with unknown correspondences */
int cslam_pf_assoc_cycle_drawn(cslam_pf_t h, int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                               const double* phi, int use_heading, const void* Z, int m, const void* R, double gate1,
                               double gate2, double new_fraction, double miss_likelihood, long long step,
                               double n_effective, int resample_status, int* q)
{
    CSLAM_NEED(h);
    return B(h)->assoc_cycle_drawn(k, v, swa, Q, wb, dt, phi, use_heading, Z, m, R, gate1, gate2, new_fraction,
                                   miss_likelihood, step, n_effective, resample_status, q);
}

/* slam.h:102, the FastSLAM-1.0 sibling of test/main.cpp:277-286: k iterations with every particle's own noisy controls
   (slam.h:149-159, then PF.cpp:419-471 and PF.cpp:382-417) in one launch per 16 steps */
int cslam_pf_control_run_sampled(cslam_pf_t h, int k, const double* v, const double* swa, const void* Q, double wb,
                                 double dt, const double* phi, int use_heading, long long ctl_step)
{
    CSLAM_NEED(h);
    return B(h)->control_run_sampled(k, v, swa, Q, wb, dt, phi, use_heading, ctl_step);
}

/* the normals slam.h:149-159 consumes in cslam_pf_control_run_sampled */
int cslam_pf_get_control_draws(cslam_pf_t h, long long ctl_step, int k, void* normals)
{
    CSLAM_NEED(h);
    return B(h)->get_control_draws(ctl_step, k, normals);
}

/* PF.cpp:343-359 (PF.cpp:279-317 per observation) at every particle's pose, with PF.cpp:222-277 riding along */
int cslam_pf_likelihood_update(cslam_pf_t h, const void* Z, int m, const int* idf, const void* R, int update_features,
                               int zero_pv)
{
    CSLAM_NEED(h);
    return B(h)->likelihood_update(Z, m, idf, R, update_features, zero_pv);
}

/* test/main.cpp:249-334 with the proposal switched off (slam.h:102): the sampled run, PF.cpp:343-359 + 222-277,
   PF.cpp:473-500, PF.cpp:9-60, in one call */
int cslam_pf_fs1_cycle_drawn(cslam_pf_t h, int k, const double* v, const double* swa, const void* Q, double wb, double dt,
                             const double* phi, int use_heading, long long ctl_step, const void* ZF, int mf, const int* idf,
                             const void* ZN, int mn, const void* R, long long step, double n_effective, int resample_status)
{
    CSLAM_NEED(h);
    return B(h)->fs1_cycle_drawn(k, v, swa, Q, wb, dt, phi, use_heading, ctl_step, ZF, mf, idf, ZN, mn, R, step,
                                 n_effective, resample_status);
}

} // extern "C"
