"""Host-side mirror of the reference's EKF back-end over the C ABI (include/cslam.h).

`EKF` offers the reference's call surface for the hot path -- predict / update / augment /
observeHeading (slam.h:841-847, 938-943, 190-191, 788; EKF.cpp) -- with the same argument meaning:
feature indices are 1-based, Z is 2 x m (range; bearing), Q and R are 2 x 2.  The difference to the
reference is ownership: X and P live on the GPU inside the handle instead of being passed by reference
into every call; `X` / `P` properties (or get_state) download them.

All arithmetic happens in the HIP library; this file only marshals pointers.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import (F32, F64, Q_REF_EXACT, Q_TEXTBOOK, check)


def _vp(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class EKF:
    def __init__(self, max_landmarks: int, dtype=np.float32, device: int = -1, quirks: int = Q_REF_EXACT,
                 sync_mode: bool = True):
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("dtype must be float32 or float64")
        self._L = _capi.lib()
        self._h = C.c_void_p(None)
        code = F32 if self.dtype == np.float32 else F64
        check(self._L.cslam_ekf_create(C.c_int(max_landmarks), C.c_int(code), C.c_int(device), C.c_int(quirks),
                                       C.byref(self._h)))
        self.max_landmarks = max_landmarks
        self.quirks = quirks
        if not sync_mode:
            self.set_sync_mode(False)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.cslam_ekf_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ helpers
    def _arr(self, a, shape=None):
        a = np.ascontiguousarray(np.asarray(a, dtype=self.dtype).reshape(-1, order="F"))
        return a

    def _mat22(self, M):
        return np.asfortranarray(np.asarray(M, dtype=self.dtype).reshape(2, 2))

    def set_sync_mode(self, on: bool):
        check(self._L.cslam_ekf_set_sync_mode(self._h, C.c_int(1 if on else 0)))

    def set_deferred(self, max_pending_columns: int):
        """Keep up to this many W1 columns pending and apply them in one P-GEMM (0 = apply at once)."""
        check(self._L.cslam_ekf_set_deferred(self._h, C.c_int(int(max_pending_columns))))

    def flush(self):
        check(self._L.cslam_ekf_flush(self._h))

    def set_pgemm_workgroups(self, workgroups: int):
        """Cap the persistent P-GEMM grid (0 = whole chip): for instances that co-run on one GPU."""
        check(self._L.cslam_ekf_set_pgemm_workgroups(self._h, C.c_int(int(workgroups))))

    # ------------------------------------------------------------------ state
    @property
    def n(self) -> int:
        v = C.c_int(0)
        check(self._L.cslam_ekf_get_n(self._h, C.byref(v)))
        return v.value

    def set_state(self, X, P):
        X = np.ascontiguousarray(X, dtype=self.dtype)
        P = np.asfortranarray(P, dtype=self.dtype)
        n = X.shape[0]
        assert P.shape == (n, n)
        check(self._L.cslam_ekf_set_state(self._h, _vp(X), C.c_int(n), _vp(P), C.c_int(n)))

    def get_state(self):
        n = self.n
        X = np.zeros(n, dtype=self.dtype)
        P = np.zeros((n, n), dtype=self.dtype, order="F")
        check(self._L.cslam_ekf_get_state(self._h, _vp(X), _vp(P), C.c_int(n)))
        return X, P

    def get_x(self):
        n = self.n
        X = np.zeros(n, dtype=self.dtype)
        check(self._L.cslam_ekf_get_x(self._h, _vp(X), C.c_int(n)))
        return X

    def get_p(self):
        return self.get_state()[1]

    X = property(get_x)
    P = property(get_p)

    def trace(self) -> float:
        t = C.c_double(0.0)
        check(self._L.cslam_ekf_trace(self._h, C.byref(t)))
        return t.value

    def synchronize(self):
        check(self._L.cslam_ekf_synchronize(self._h))

    def pgemm_split(self):
        """(whole tiles, strips) of the handle's last f32 P-GEMM launch of at most 128 columns (cslam_ekf_pgemm_split)"""
        w, s = C.c_int(0), C.c_int(0)
        check(self._L.cslam_ekf_pgemm_split(self._h, C.byref(w), C.byref(s)))
        return w.value, s.value

    def lookahead_windows(self) -> int:
        """look-ahead windows this handle has launched (cslam_ekf_lookahead_windows)"""
        w = C.c_longlong(0)
        check(self._L.cslam_ekf_lookahead_windows(self._h, C.byref(w)))
        return w.value

    def streams(self):
        """(chain stream, P-GEMM stream) of the handle as integer hipStream_t values (cslam_ekf_get_streams): for callers
        that order their own work, or the reuse of their input buffers, against the engine's"""
        a, b = C.c_void_p(None), C.c_void_p(None)
        check(self._L.cslam_ekf_get_streams(self._h, C.byref(a), C.byref(b)))
        return a.value or 0, b.value or 0

    def stage_launches(self) -> int:
        """launches of the kernel that snapshots a queued update's device inputs (cslam_ekf_stage_launches)"""
        w = C.c_longlong(0)
        check(self._L.cslam_ekf_stage_launches(self._h, C.byref(w)))
        return w.value

    def rows_launches(self) -> int:
        """launches of the kernel that gathers pending-panel rows for a look-ahead window (cslam_ekf_rows_launches)"""
        w = C.c_longlong(0)
        check(self._L.cslam_ekf_rows_launches(self._h, C.byref(w)))
        return w.value

    def landmarks(self, first: int = 1, count: int = None):
        """(x [c, 2], P [c, 2, 2], Pvl [c, 3, 2]) of landmarks first .. first + c - 1 (1-based; count None: to the
        last): means, marginal 2 x 2 blocks and pose-landmark blocks P[0:3, fx:fx+2], read without applying the pending
        covariance downdate (cslam_ekf_get_landmarks): the run continues bit for bit as without the read."""
        if count is None:
            count = max((self.n - 3) // 2 - first + 1, 0)
        x = np.empty((count, 2), dtype=self.dtype)
        pll = np.empty((count, 4), dtype=self.dtype)
        pvl = np.empty((count, 6), dtype=self.dtype)
        check(self._L.cslam_ekf_get_landmarks(self._h, int(first), int(count), _vp(x), _vp(pll), _vp(pvl)))
        # (column-major blocks per landmark)
        return x, pll.reshape(count, 2, 2).transpose(0, 2, 1).copy(), pvl.reshape(count, 2, 3).transpose(0, 2, 1).copy()

    def pose(self):
        """(x [3], pvv [3, 3]): the pose and the 3 x 3 pose block after launching what is queued, read from the pose
        stripe without the covariance downdate or a copy of P (cslam_ekf_get_pose).  Synchronises."""
        x = np.empty(3, dtype=self.dtype)
        pv = np.empty(9, dtype=self.dtype)
        check(self._L.cslam_ekf_get_pose(self._h, _vp(x), _vp(pv)))
        return x, pv.reshape(3, 3).T.copy()  # (column-major)

    def factor_status(self, clear: bool = False) -> int:
        f = C.c_int(0)
        check(self._L.cslam_ekf_factor_status(self._h, C.byref(f), C.c_int(1 if clear else 0)))
        return f.value

    # ------------------------------------------------------------------ the score, kept on the device
    def score_reset(self, series_capacity: int = 0, gate_pose: float = 0.0, gate_lm: float = 0.0):
        """Zero the totals, the series and the track (room for `series_capacity` records, one per score call) and the call
        count.  A gate <= 0 is the 95 % chi-square point (7.8147 for the pose, 5.9915 for a landmark).  Keeps the truth."""
        check(self._L.cslam_ekf_score_reset(self._h, C.c_int(int(series_capacity)), C.c_double(float(gate_pose)),
                                            C.c_double(float(gate_lm))))

    def score_set_truth(self, lm_true):
        """Row j of lm_true ([count, 2]) is the true position of state feature j + 1.  Features beyond count are not scored."""
        t = np.ascontiguousarray(np.asarray(lm_true, dtype=np.float64).reshape(-1, 2))
        check(self._L.cslam_ekf_score_set_truth(self._h, _vp(t) if t.size else None, C.c_int(t.shape[0])))

    def score(self, xv_true, with_map: bool = True):
        """One score step against the true pose (x, y, phi): pose error and NEES, map error and landmark NEES enter the
        totals on the device, and the call's series and track records are written.  Launches what is queued as landmarks()
        does; does not synchronise, copies nothing back and leaves the run bit for bit as without the call
        (cslam_ekf_score)."""
        x = np.ascontiguousarray(np.asarray(xv_true, dtype=np.float64).reshape(3))
        check(self._L.cslam_ekf_score(self._h, _vp(x), C.c_int(1 if with_map else 0)))

    def scores(self, capacity_records: int = None):
        """-> (totals [SCORE_FIELDS] float64, series [records, 4] float32, track [records, 5] float64, calls): the one
        synchronising call of the score (cslam_ekf_get_scores).  The fields of totals are _capi.SCORE_FIELD_NAMES; a
        series record holds pose err^2, pose NEES, mean landmark err^2 and mean landmark NEES of one call (NaN where there
        is none), a track record X[0], X[1], X[2], trace(P) and n."""
        rec, calls = C.c_int(0), C.c_longlong(0)
        check(self._L.cslam_ekf_get_scores(self._h, None, None, None, C.c_int(0), C.byref(rec), C.byref(calls)))
        n = rec.value if capacity_records is None else min(rec.value, int(capacity_records))
        totals = np.zeros(_capi.SCORE_FIELDS, np.float64)
        series = np.zeros((n, _capi.EKF_SCORE_SERIES), np.float32)
        track = np.zeros((n, _capi.EKF_SCORE_TRACK), np.float64)
        check(self._L.cslam_ekf_get_scores(self._h, _vp(totals), _vp(series) if n else None, _vp(track) if n else None,
                                           C.c_int(n), C.byref(rec), C.byref(calls)))
        return totals, series, track, int(calls.value)

    # ------------------------------------------------------------------ the hot path
    def predict(self, v, swa, Q, wb, dt):
        """Slam::predict(X, P, v, swa, Q, wb, dt) -- EKF.cpp:406-455."""
        Q = self._mat22(Q)
        check(self._L.cslam_ekf_predict(self._h, C.c_double(float(v)), C.c_double(float(swa)), _vp(Q),
                                        C.c_double(float(wb)), C.c_double(float(dt))))

    def update(self, Z, R, idf, batch: bool = False):
        """Slam::update(X, P, Z, R, idf, batch) -- EKF.cpp:481-496 (batch defaults to false, slam.h:943)."""
        Z = np.asarray(Z, dtype=self.dtype)
        m = 0 if Z.size == 0 else Z.reshape(2, -1, order="F").shape[1]
        Zc = self._arr(Z) if m else np.zeros(2, dtype=self.dtype)
        R = self._mat22(R)
        idf = np.ascontiguousarray(idf, dtype=np.int32)
        assert idf.shape[0] == m
        idp = idf.ctypes.data_as(C.c_void_p) if m else None
        check(self._L.cslam_ekf_update(self._h, _vp(Zc), C.c_int(m), _vp(R), idp, C.c_int(1 if batch else 0)))

    def update_device(self, dZ_ptr: int, m: int, R, d_idf_ptr: int, batch: bool = True):
        """update() with Z (2 x m scalars) and idf (m int32) already in HBM (raw device pointers)."""
        R = self._mat22(R)
        check(self._L.cslam_ekf_update_device(self._h, C.c_void_p(dZ_ptr), C.c_int(m), _vp(R), C.c_void_p(d_idf_ptr),
                                              C.c_int(1 if batch else 0)))

    def augment(self, Z, R):
        """Slam::augment(X, P, Z, R) -- EKF.cpp:9-26."""
        Z = np.asarray(Z, dtype=self.dtype)
        q = 0 if Z.size == 0 else Z.reshape(2, -1, order="F").shape[1]
        Zc = self._arr(Z) if q else np.zeros(2, dtype=self.dtype)
        R = self._mat22(R)
        check(self._L.cslam_ekf_augment(self._h, _vp(Zc), C.c_int(q), _vp(R)))

    def observe_heading(self, phi, use_heading: bool = False):
        """Slam::observeHeading(X, P, phi, useHeading) -- EKF.cpp:328-352 (default false, slam.h:788)."""
        check(self._L.cslam_ekf_observe_heading(self._h, C.c_double(float(phi)), C.c_int(1 if use_heading else 0)))

    def associate(self, Z, R, gate1, gate2):
        """Raw result of the gated nearest-neighbour search (EKF.cpp:235-326 with computeAssociation EKF.cpp:131-144):
        (idf[m], kind[m]); kind 1 = associated with the 1-based feature idf[i], 2 = new feature, 0 = dropped."""
        Z = np.asarray(Z, dtype=self.dtype, order="F").reshape(2, -1, order="F")
        R = np.asarray(R, dtype=self.dtype, order="F")
        m = Z.shape[1]
        idf = np.zeros(max(m, 1), dtype=np.int32)
        kind = np.zeros(max(m, 1), dtype=np.int32)
        check(self._L.cslam_ekf_associate(self._h, Z.ctypes.data_as(C.c_void_p), C.c_int(m), R.ctypes.data_as(C.c_void_p),
                                          C.c_double(float(gate1)), C.c_double(float(gate2)),
                                          idf.ctypes.data_as(C.POINTER(C.c_int)), kind.ctypes.data_as(C.POINTER(C.c_int))))
        return idf[:m], kind[:m]

    def data_associate(self, Z, R, gate1, gate2):
        """Slam::dataAssociate(X, P, Z, R, gate1, gate2) -> (ZF, ZN, idf) -- EKF.cpp:235-326.
        Under REF_EXACT quirks ZN is EMPTY, as in the reference (EKF.cpp:307 re-declares ZN inside the try block, so the
        returned matrix is the 0 x 0 one of line 243); TEXTBOOK returns the new-feature observations the loop found."""
        Z = np.asarray(Z, dtype=self.dtype, order="F").reshape(2, -1, order="F")
        idf, kind = self.associate(Z, R, gate1, gate2)
        ZF = np.asfortranarray(Z[:, kind == 1])
        if self.quirks == Q_REF_EXACT:
            ZN = np.zeros((0, 0), dtype=self.dtype)
        else:
            ZN = np.asfortranarray(Z[:, kind == 2])
        return ZF, ZN, idf[kind == 1].astype(np.int32)

    def associate_deferred(self, Z, R, gate1, gate2, with_counts: bool = False):
        """associate() read from the deferred covariance as it stands (cslam_ekf_associate_deferred): nothing pending is
        applied and the run continues bit for bit as without the call.  -> (idf[m], kind[m]), and with_counts also
        counts[3] = (associated, new, dropped).  The split stays on the device: association_device_ptrs()."""
        Z = np.asarray(Z, dtype=self.dtype, order="F").reshape(2, -1, order="F")
        R = np.asarray(R, dtype=self.dtype, order="F")
        m = Z.shape[1]
        idf = np.zeros(max(m, 1), dtype=np.int32)
        kind = np.zeros(max(m, 1), dtype=np.int32)
        counts = np.zeros(3, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        check(self._L.cslam_ekf_associate_deferred(self._h, _vp(Z) if m else None, C.c_int(m), _vp(R),
                                                   C.c_double(float(gate1)), C.c_double(float(gate2)),
                                                   idf.ctypes.data_as(ip), kind.ctypes.data_as(ip), counts.ctypes.data_as(ip)))
        return (idf[:m], kind[:m], counts) if with_counts else (idf[:m], kind[:m])

    def data_associate_deferred(self, Z, R, gate1, gate2):
        """data_associate() on associate_deferred(): (ZF, ZN, idf), with the same REF_EXACT rule for ZN."""
        Z = np.asarray(Z, dtype=self.dtype, order="F").reshape(2, -1, order="F")
        idf, kind = self.associate_deferred(Z, R, gate1, gate2)
        ZF = np.asfortranarray(Z[:, kind == 1])
        if self.quirks == Q_REF_EXACT:
            ZN = np.zeros((0, 0), dtype=self.dtype)
        else:
            ZN = np.asfortranarray(Z[:, kind == 2])
        return ZF, ZN, idf[kind == 1].astype(np.int32)

    def association_device_ptrs(self):
        """(dZF, d_idf, dZN, d_counts): raw device pointers of the split the last associate_deferred() call with m > 0 left
        in HBM -- ZF (2 x mf), idf (mf int32), ZN (2 x mn), counts (3 int32) -- valid until the next such call; dZF and d_idf
        are fit for update_device(dZF, mf, R, d_idf) (cslam_ekf_association_device_ptrs)."""
        p = [C.c_void_p(None) for _ in range(4)]
        check(self._L.cslam_ekf_association_device_ptrs(self._h, *(C.byref(q) for q in p)))
        return tuple(q.value or 0 for q in p)

    def update_counted(self, dZ_ptr: int, m_cap: int, R, d_idf_ptr: int, d_count_ptr: int):
        """update_device(dZ, c, R, d_idf, batch=True) with c = clamp(*d_count, 0, m_cap) read on the device in stream order
        (cslam_ekf_update_counted): the host never learns c and never waits.  Raw device pointers; entries c .. m_cap-1 of
        dZ / d_idf are never read.  m_cap <= 64 (f32) or 32 (f64), asynchronous mode only."""
        R = self._mat22(R)
        check(self._L.cslam_ekf_update_counted(self._h, C.c_void_p(dZ_ptr), C.c_int(m_cap), _vp(R), C.c_void_p(d_idf_ptr),
                                               C.c_void_p(d_count_ptr), C.c_int(1)))

    def associate_deferred_async(self, Z, R, gate1, gate2):
        """associate_deferred() without the wait (cslam_ekf_associate_deferred_async): Z is consumed before the call returns,
        the answer is handed out by association_wait(), and association_device_ptrs() may be used at once on the stream."""
        Z = np.asarray(Z, dtype=self.dtype, order="F").reshape(2, -1, order="F")
        R = np.asarray(R, dtype=self.dtype, order="F")
        self._assoc_m = m = Z.shape[1]
        check(self._L.cslam_ekf_associate_deferred_async(self._h, _vp(Z) if m else None, C.c_int(m), _vp(R),
                                                         C.c_double(float(gate1)), C.c_double(float(gate2))))

    def association_wait(self, with_counts: bool = False):
        """The answer of the outstanding associate_deferred_async() call: (idf[m], kind[m]), and with_counts also counts[3]
        (cslam_ekf_association_wait).  Waits for the association only, not for work enqueued behind it."""
        m = getattr(self, "_assoc_m", 0)
        idf = np.zeros(max(m, 1), dtype=np.int32)
        kind = np.zeros(max(m, 1), dtype=np.int32)
        counts = np.zeros(3, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        check(self._L.cslam_ekf_association_wait(self._h, idf.ctypes.data_as(ip), kind.ctypes.data_as(ip),
                                                 counts.ctypes.data_as(ip)))
        return (idf[:m], kind[:m], counts) if with_counts else (idf[:m], kind[:m])

    def associate_update_counted(self, Z, R, gate1, gate2):
        """One observation step with no host round trip between association and update: associate_deferred_async(), then
        update_counted() on the device lists with m_cap = m (the count mf is read on the device), then association_wait().
        -> (idf[m], kind[m], counts[3])."""
        Z = np.asarray(Z, dtype=self.dtype, order="F").reshape(2, -1, order="F")
        self.associate_deferred_async(Z, R, gate1, gate2)
        if Z.shape[1]:
            dZF, d_idf, _, d_counts = self.association_device_ptrs()
            self.update_counted(dZF, Z.shape[1], R, d_idf, d_counts)
        return self.association_wait(with_counts=True)

    def augment_device(self, dZ_ptr: int, q: int, R):
        """augment() with Z (2 x q scalars, column-major, the handle's dtype) already in HBM (a raw device pointer): one
        launch per 64 features instead of one per feature, the same bits (cslam_ekf_augment_device).  Entries beyond 2q
        are never read; q stays a host value."""
        R = self._mat22(R)
        check(self._L.cslam_ekf_augment_device(self._h, C.c_void_p(dZ_ptr) if dZ_ptr else None, C.c_int(int(q)), _vp(R)))

    def augment_launches(self) -> int:
        """augment kernel launches of this handle, from augment() and augment_device() (cslam_ekf_augment_launches)"""
        w = C.c_longlong(0)
        check(self._L.cslam_ekf_augment_launches(self._h, C.byref(w)))
        return w.value

    def associate_update_augment(self, Z, R, gate1, gate2):
        """One whole observation step of the reference's loop (test/main.cpp:180-189) from the device lists:
        associate_deferred_async(), update_counted() on ZF / idf, association_wait() -- which waits for the association
        only, the update runs behind it -- and then augment_device() on the ZN the association left in HBM, with the count
        the wait returned.  Under REF_EXACT quirks nothing is augmented: the reference returns an empty ZN there
        (EKF.cpp:307, see data_associate_deferred).  -> (idf[m], kind[m], counts[3])."""
        idf, kind, counts = self.associate_update_counted(Z, R, gate1, gate2)
        if counts[1] > 0 and self.quirks != Q_REF_EXACT:
            dZN = self.association_device_ptrs()[2]
            self.augment_device(dZN, int(counts[1]), R)
        return idf, kind, counts

    # reference-style aliases
    observeHeading = observe_heading
    dataAssociate = data_associate

    # ------------------------------------------------------------------ measurement / introspection
    def set_profiling(self, mode: int):
        """0 off, 1 every stage of update(), 2 every downdate (P-GEMM) launch, 3 one downdate launch in sixteen."""
        check(self._L.cslam_ekf_set_profiling(self._h, C.c_int(mode)))

    def stage_times(self):
        ms = (C.c_double * _capi.N_STAGES)()
        cnt = (C.c_int * _capi.N_STAGES)()
        check(self._L.cslam_ekf_get_stage_times(self._h, ms, cnt))
        return {name: (ms[i], cnt[i]) for i, name in enumerate(_capi.STAGE_NAMES)}

    def debug_last_update(self):
        n = self.n
        k = C.c_int(0)
        check(self._L.cslam_ekf_debug_last_update(self._h, None, None, None, None, None, C.byref(k)))
        k = k.value
        out = {
            "PHT": np.zeros((n, k), self.dtype, order="F"),
            "S": np.zeros((k, k), self.dtype, order="F"),
            "G": np.zeros((k, k), self.dtype, order="F"),
            "W1": np.zeros((n, k), self.dtype, order="F"),
            "V": np.zeros(k, self.dtype),
        }
        if k:
            check(self._L.cslam_ekf_debug_last_update(self._h, _vp(out["PHT"]), _vp(out["S"]), _vp(out["G"]),
                                                      _vp(out["W1"]), _vp(out["V"]), C.byref(C.c_int(0))))
        return out


def run_many(engines, steps: int, v, swa, Q, wb: float, dt: float, dZ_ptrs, d_idf_ptrs, m: int, R, batch: bool = True):
    """steps x {predict(v[t], swa[t], Q, wb, dt); update_device(Z_t, R, idf_t, batch)} on every EKF of `engines` at once,
    one host thread and one stream pair per handle (cslam_ekf_run_many).  The handles may differ in size but share one
    dtype: Q and R are read in it.  dZ_ptrs / d_idf_ptrs: one device pointer per engine (steps x 2m scalars / steps x m
    int32, step-major).  An entry of None goes to the library as a null pointer, which answers ERR_BAD_ARG."""
    engines = list(engines)
    if len(dZ_ptrs) != len(engines) or len(d_idf_ptrs) != len(engines):
        raise ValueError("run_many: not one input pointer per engine")
    dtypes = {e.dtype for e in engines if e is not None}
    if len(dtypes) > 1:
        raise ValueError("run_many: the engines must share one dtype (Q and R are read in it)")
    dtype = dtypes.pop() if dtypes else np.dtype(np.float32)
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    swa = np.ascontiguousarray(swa, dtype=np.float64).reshape(-1)
    if v.shape[0] < steps or swa.shape[0] < steps:
        raise ValueError("run_many: controls shorter than `steps`")
    Q = np.asfortranarray(np.asarray(Q, dtype=dtype).reshape(2, 2))
    R = np.asfortranarray(np.asarray(R, dtype=dtype).reshape(2, 2))
    cnt = len(engines)
    hs = (C.c_void_p * cnt)(*[e._h if e is not None else None for e in engines])
    zs = (C.c_void_p * cnt)(*[int(p) if p else None for p in dZ_ptrs])
    ids = (C.c_void_p * cnt)(*[int(p) if p else None for p in d_idf_ptrs])
    check(_capi.lib().cslam_ekf_run_many(hs, C.c_int(cnt), C.c_int(int(steps)), v.ctypes.data_as(C.POINTER(C.c_double)),
                                         swa.ctypes.data_as(C.POINTER(C.c_double)), _vp(Q), C.c_double(float(wb)),
                                         C.c_double(float(dt)), zs, ids, C.c_int(int(m)), _vp(R),
                                         C.c_int(1 if batch else 0)))


class EKFBatch:
    """`instances` independent f32 filters of `n_landmarks` landmarks each, advancing in lockstep (cslam_ekf_batch_*):
    the Monte-Carlo unit of BASELINE configs[4] (test/main.cpp:132-200 x I) with one launch per stage for all
    instances.

    max_landmarks: capacity for augment_device (default: n_landmarks, a map of fixed size); n_landmarks defaults to
    max_landmarks (0 = the reference driver's X = 0_3, P = 0_3x3).  The reference's loop runs through predict /
    observe_heading / update_device / augment_device, one call per reference call for all instances."""

    def __init__(self, instances: int, n_landmarks: int = None, device: int = -1, quirks: int = Q_REF_EXACT, *,
                 max_landmarks: int = None):
        if n_landmarks is None and max_landmarks is None:
            raise ValueError("EKFBatch: give n_landmarks and / or max_landmarks")
        if max_landmarks is None:
            max_landmarks = n_landmarks
        if n_landmarks is None:
            n_landmarks = max_landmarks
        self._L = _capi.lib()
        self._h = C.c_void_p(None)
        check(self._L.cslam_ekf_batch_create_capacity(C.c_int(instances), C.c_int(max_landmarks), C.c_int(n_landmarks),
                                                      C.c_int(device), C.c_int(quirks), C.byref(self._h)))
        self.instances, self.max_landmarks = instances, max_landmarks
        self.quirks = quirks

    @property
    def n(self) -> int:
        """current state size 3 + 2 * landmarks (common to the instances; grows with augment_device)"""
        n = C.c_int(0)
        check(self._L.cslam_ekf_batch_info(self._h, None, C.byref(n), None))
        return n.value

    @property
    def n_landmarks(self) -> int:
        return (self.n - 3) // 2

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.cslam_ekf_batch_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_state(self, instance: int, X, P):
        X = np.ascontiguousarray(X, dtype=np.float32)
        P = np.asfortranarray(P, dtype=np.float32)
        if X.shape != (self.n,) or P.shape != (self.n, self.n):
            raise ValueError(f"state of {X.shape} / {P.shape}: the batch holds filters of n = {self.n}")
        check(self._L.cslam_ekf_batch_set_state(self._h, C.c_int(instance), _vp(X), C.c_int(self.n), _vp(P), C.c_int(self.n)))

    def get_state(self, instance: int):
        X = np.empty(self.n, dtype=np.float32)
        P = np.empty((self.n, self.n), dtype=np.float32, order="F")
        check(self._L.cslam_ekf_batch_get_state(self._h, C.c_int(instance), _vp(X), _vp(P), C.c_int(self.n)))
        return X, P

    def run(self, steps: int, v, swa, Q, wb: float, dt: float, dZ_ptrs, d_idf_ptrs, m: int, R):
        """steps x {predict; update} on every instance.  v / swa: `steps` controls (common to the instances);
        dZ_ptrs / d_idf_ptrs: one device pointer per instance (steps x 2m float32 / steps x m int32, step-major)."""
        v = np.ascontiguousarray(v, dtype=np.float64)
        swa = np.ascontiguousarray(swa, dtype=np.float64)
        if v.shape[0] < steps or swa.shape[0] < steps or len(dZ_ptrs) != self.instances or len(d_idf_ptrs) != self.instances:
            raise ValueError("run: controls shorter than `steps`, or not one input pointer per instance")
        Q = np.asfortranarray(Q, dtype=np.float32)
        R = np.asfortranarray(R, dtype=np.float32)
        zs = (C.c_void_p * self.instances)(*[int(p) for p in dZ_ptrs])
        ids = (C.c_void_p * self.instances)(*[int(p) for p in d_idf_ptrs])
        check(self._L.cslam_ekf_batch_run(self._h, C.c_int(steps), v.ctypes.data_as(C.POINTER(C.c_double)),
                                          swa.ctypes.data_as(C.POINTER(C.c_double)), _vp(Q), C.c_double(wb), C.c_double(dt),
                                          zs, ids, C.c_int(m), _vp(R)))

    def predict(self, v: float, swa: float, Q, wb: float, dt: float):
        """Slam::predict on every instance (held until the next call that needs it, as a single handle's)."""
        Q = np.asfortranarray(Q, dtype=np.float32)
        check(self._L.cslam_ekf_batch_predict(self._h, C.c_double(v), C.c_double(swa), _vp(Q), C.c_double(wb),
                                              C.c_double(dt)))

    def predict_each(self, v, swa, Q, wb: float, dt: float):
        """Slam::predict with controls per instance: v / swa hold `instances` values (the reference's control noise,
        slam.h:149-159).  Held until the next call; observe_heading joins it, anything else launches it as a
        predict-only step (never inside an update's window, see cslam_ekf_batch_predict_each)."""
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        swa = np.ascontiguousarray(swa, dtype=np.float64).reshape(-1)
        if v.shape[0] != self.instances or swa.shape[0] != self.instances:
            raise ValueError(f"predict_each: v / swa need {self.instances} values, one per instance")
        Q = np.asfortranarray(Q, dtype=np.float32)
        check(self._L.cslam_ekf_batch_predict_each(self._h, v.ctypes.data_as(C.POINTER(C.c_double)),
                                                   swa.ctypes.data_as(C.POINTER(C.c_double)), _vp(Q), C.c_double(wb),
                                                   C.c_double(dt)))

    def poses(self):
        """(x [I, 3], pvv [I, 3, 3]): every instance's pose and 3 x 3 pose block after launching what is queued --
        48 bytes per instance, without the covariance downdate or a copy of P (cslam_ekf_batch_get_poses)."""
        x = np.empty((self.instances, 3), dtype=np.float32)
        pv = np.empty((self.instances, 9), dtype=np.float32)
        check(self._L.cslam_ekf_batch_get_poses(self._h, _vp(x), _vp(pv)))
        return x, pv.reshape(self.instances, 3, 3).transpose(0, 2, 1).copy()  # (column-major per instance)

    def landmarks(self, first: int = 1, count: int = None):
        """EKF.landmarks for every instance: (x [I, c, 2], P [I, c, 2, 2], Pvl [I, c, 3, 2]) after launching what is
        queued, without the covariance downdate or a copy of P (cslam_ekf_batch_get_landmarks)."""
        if count is None:
            count = max(self.n_landmarks - first + 1, 0)
        I = self.instances
        x = np.empty((I, count, 2), dtype=np.float32)
        pll = np.empty((I, count, 4), dtype=np.float32)
        pvl = np.empty((I, count, 6), dtype=np.float32)
        check(self._L.cslam_ekf_batch_get_landmarks(self._h, int(first), int(count), _vp(x), _vp(pll), _vp(pvl)))
        return (x, pll.reshape(I, count, 2, 2).transpose(0, 1, 3, 2).copy(),
                pvl.reshape(I, count, 2, 3).transpose(0, 1, 3, 2).copy())

    def observe_heading(self, phi: float, use: bool = True):
        """Slam::observeHeading on every instance (phi common).  An instance with P22 + R <= 0 skips it and raises
        FACTOR_HEADING_SKIPPED (see cslam_ekf_batch_observe_heading)."""
        check(self._L.cslam_ekf_batch_observe_heading(self._h, C.c_double(phi), C.c_int(1 if use else 0)))

    def update_device(self, dZ_ptrs, d_idf_ptrs, m: int, R):
        """Slam::update(batch = true) on every instance: one device pointer per instance to its 2 x m float32
        observations (column-major) and m int32 feature indices, read in stream order; 1 <= m <= 32 (m = 0: nothing)."""
        if len(dZ_ptrs) != self.instances or len(d_idf_ptrs) != self.instances:
            raise ValueError("update_device: not one input pointer per instance")
        R = np.asfortranarray(R, dtype=np.float32)
        zs = (C.c_void_p * self.instances)(*[int(p) for p in dZ_ptrs])
        ids = (C.c_void_p * self.instances)(*[int(p) for p in d_idf_ptrs])
        check(self._L.cslam_ekf_batch_update(self._h, zs, ids, C.c_int(m), _vp(R)))

    def augment_device(self, dZn_ptrs, q: int, R):
        """Slam::augment on every instance: one device pointer per instance to its 2 x q float32 new-feature
        observations (column-major), read in stream order."""
        if len(dZn_ptrs) != self.instances:
            raise ValueError("augment_device: not one input pointer per instance")
        R = np.asfortranarray(R, dtype=np.float32)
        zs = (C.c_void_p * self.instances)(*[int(p) for p in dZn_ptrs])
        check(self._L.cslam_ekf_batch_augment(self._h, zs, C.c_int(q), _vp(R)))

    def update_scan(self, sim, R):
        """Slam::update(batch = true) on every instance with the current scan of a BatchSimulator: update_device with
        that scan's ZF / idf, without a pointer table passing through the host.  mf = 0: nothing."""
        R = np.asfortranarray(R, dtype=np.float32)
        check(self._L.cslam_ekf_batch_update_scan(self._h, sim._h, _vp(R)))

    def augment_scan(self, sim, R):
        """Slam::augment on every instance with the new-feature part of a BatchSimulator's current scan (after
        update_scan when the scan has known features).  mn = 0: nothing."""
        R = np.asfortranarray(R, dtype=np.float32)
        check(self._L.cslam_ekf_batch_augment_scan(self._h, sim._h, _vp(R)))

    # ------------------------------------------------------------------ the score, kept on the device
    def score_reset(self, series_capacity: int = 0, gate_pose: float = 0.0, gate_lm: float = 0.0):
        """Zeroes the totals, the series (room for `series_capacity` records, one per score call) and the call count.  A
        gate <= 0 is the 95 % chi-square point (7.8147 for the pose, 5.9915 for a landmark)."""
        check(self._L.cslam_ekf_batch_score_reset(self._h, C.c_int(int(series_capacity)), C.c_double(gate_pose),
                                                  C.c_double(gate_lm)))
        self._series_capacity = int(series_capacity)

    def score_set_truth(self, lm_true):
        """lm_true [count, 2]: the true position of state feature j + 1 in row j.  Features beyond count are not scored."""
        t = np.ascontiguousarray(lm_true, dtype=np.float32).reshape(-1, 2)
        check(self._L.cslam_ekf_batch_score_set_truth(self._h, _vp(t) if t.size else None, C.c_int(t.shape[0])))

    def score(self, xv_true):
        """One score step against the true pose (x, y, phi): pose error and NEES, map error and landmark NEES of every
        instance enter the totals on the device.  Launches what is queued as landmarks() does; does not synchronise, copies
        nothing back and leaves the run bit for bit as without the call (cslam_ekf_batch_score)."""
        xv = np.ascontiguousarray(xv_true, dtype=np.float32).reshape(3)
        check(self._L.cslam_ekf_batch_score(self._h, _vp(xv)))

    def score_scan(self, sim, xv_true):
        """score() with the true positions taken from a BatchSimulator's map through its association table."""
        xv = np.ascontiguousarray(xv_true, dtype=np.float32).reshape(3)
        check(self._L.cslam_ekf_batch_score_scan(self._h, sim._h, _vp(xv)))

    def scores(self):
        """-> (totals [I, SCORE_FIELDS] float64, series [records, I, 4] float32, calls).  Synchronises.  The columns of
        totals are _capi.SCORE_FIELD_NAMES; a series record holds pose err^2, pose NEES, mean landmark err^2 and mean
        landmark NEES of one call (NaN where there is none)."""
        I = self.instances
        cap = getattr(self, "_series_capacity", 0)
        totals = np.zeros((I, _capi.SCORE_FIELDS), dtype=np.float64)
        series = np.zeros((max(cap, 1), I, 4), dtype=np.float32)
        rec, calls = C.c_int(0), C.c_longlong(0)
        check(self._L.cslam_ekf_batch_get_scores(self._h, _vp(totals), _vp(series), C.c_int(cap), C.byref(rec),
                                                 C.byref(calls)))
        return totals, series[: min(rec.value, cap)].copy(), calls.value

    def flush(self):
        check(self._L.cslam_ekf_batch_flush(self._h))

    def synchronize(self):
        check(self._L.cslam_ekf_batch_synchronize(self._h))

    def trace(self):
        tr = (C.c_double * self.instances)()
        check(self._L.cslam_ekf_batch_trace(self._h, tr))
        return [float(t) for t in tr]

    def factor_status(self):
        fl = (C.c_int * self.instances)()
        check(self._L.cslam_ekf_batch_factor_status(self._h, fl))
        return [int(f) for f in fl]

    def windows(self) -> int:
        w = C.c_longlong(0)
        check(self._L.cslam_ekf_batch_info(self._h, None, None, C.byref(w)))
        return w.value

    def pgemm_split(self):
        """(whole tiles, strips) of the batch's last P-GEMM launch (cslam_ekf_batch_pgemm_split)"""
        w, s = C.c_int(0), C.c_int(0)
        check(self._L.cslam_ekf_batch_pgemm_split(self._h, C.byref(w), C.byref(s)))
        return w.value, s.value

    def set_profiling(self, every: int):
        check(self._L.cslam_ekf_batch_set_profiling(self._h, C.c_int(every)))

    def pgemm_time(self):
        """(sum of ms, launches) of the covariance-downdate launches timed since set_profiling(every > 0)."""
        ms, cnt = C.c_double(0.0), C.c_int(0)
        check(self._L.cslam_ekf_batch_get_pgemm_time(self._h, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value
