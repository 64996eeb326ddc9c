"""Host-side mirror of the reference's FastSLAM-2 back-end (PF.cpp) over the C ABI, sharded one shard per GPU.

`ParticleShard` wraps one `cslam_pf_t` handle: the particles this process owns, structure-of-arrays in HBM.
Its methods carry the reference's names and argument meaning applied to EVERY owned particle:
predict / observe_heading / sample_proposal / feature_update / add_features (PF.cpp:419-471, 382-417,
502-544, 222-277, 9-60).

`resample_particles` is the one step that couples particles (PF.cpp:473-500).  With the particle set
block-partitioned over `world` ranks it runs as SURVEY.md 8e describes:
  1. all-reduce(SUM) of the two local scalars [sum w, sum w^2]  -> global weight sum, Neff
  2. every rank scales its weights by 1/ws                        (PF.cpp:482-487)
  3. only if Neff < Nmin and resampling is on (PF.cpp:490):
       all-gather of the normalised weights -> every rank derives the identical keep[] from the shared
       select[] (stratified resample, PF.cpp:546-577 with the indexing defect of SURVEY 2.1 #8 removed),
       particle records whose source rank differs from the destination rank travel in ONE all-to-all-v;
       weights become 1/N.
The collectives go through a small `Comm` interface: `TorchComm` is torch.distributed (backend "nccl" = RCCL
over xGMI on the GPU box, "gloo" in the CPU tests), `SingleComm` is the world-size-1 case with no
communication at all.  The planning logic (who sends which particle where) is pure host code and is what the
world_size-2 gloo tests exercise with a numpy stand-in for the shard.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import List, Sequence, Tuple

import numpy as np

from . import _capi
from ._capi import F32, F64, Q_REF_EXACT, check


def _vp(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------
# stratified resampling on the host (N is at most a few thousand scalars)
# ------------------------------------------------------------------------------------------------
def stratified_random(n: int, uniforms: np.ndarray, dtype=np.float32) -> np.ndarray:
    """PF.cpp:579-596 with uniform[0,1) strata offsets (Bailey's stratified_random; the reference's Gaussian
    offsets are defect #10 of SURVEY 2.1): select[i] = k/2 + i*k + (u[i]*k - k/2), k = 1/n."""
    t = np.dtype(dtype).type
    k = t(1) / t(n)
    # di_0 = k/2, di_i = di_(i-1) + k: a running sum in the particle dtype (np.cumsum accumulates sequentially in the
    # requested dtype, i.e. with the same roundings as the reference's loop); the rest is elementwise in that dtype
    steps = np.full(n, k, dtype=dtype)
    steps[0] = k / t(2)
    di = np.cumsum(steps, dtype=dtype)
    u = np.asarray(uniforms)[:n].astype(dtype)
    return (di + (u * k - k / t(2))).astype(dtype)


def stratified_keep(w_norm: np.ndarray, select: np.ndarray) -> np.ndarray:
    """PF.cpp:559-574 (intended form): 0-based index of the particle each slot keeps = the first i whose running weight
    sum exceeds the slot's stratum position (none: 0, as the reference's zero-initialised Keep).  The running sum is
    sequential in the particle dtype (np.cumsum accumulates in index order in the requested dtype: the reference's
    sequence of roundings); the search is what pf_resample_plan_kernel / pf_keep_kernel do on the device."""
    dtype = w_norm.dtype
    n = w_norm.shape[0]
    cum = np.cumsum(w_norm, dtype=dtype)
    keep = np.searchsorted(cum, np.asarray(select, dtype=dtype), side="right")
    keep[keep >= n] = 0
    return keep.astype(np.int32)


def plan_exchange(keep: np.ndarray, rank: int, world: int, n_local: int):
    """Who sends what where.  Global slot g lives on rank g // n_local at local index g % n_local.
    Returns (send_src_local, send_counts, recv_dst_local, recv_counts):
      send_src_local: local source indices, grouped by destination rank (rank order, ascending slot)
      recv_dst_local: local destination slots, grouped by source rank in the same canonical order."""
    n = keep.shape[0]
    assert n == world * n_local
    dst_rank = np.arange(n) // n_local
    src_rank = keep // n_local
    send_src, send_counts, recv_dst, recv_counts = [], [], [], []
    for d in range(world):
        sel = np.nonzero((src_rank == rank) & (dst_rank == d))[0]
        send_src.extend((keep[sel] % n_local).tolist())
        send_counts.append(int(sel.shape[0]))
    for s in range(world):
        sel = np.nonzero((dst_rank == rank) & (src_rank == s))[0]
        recv_dst.extend((sel % n_local).tolist())
        recv_counts.append(int(sel.shape[0]))
    return (np.array(send_src, dtype=np.int32), send_counts, np.array(recv_dst, dtype=np.int32), recv_counts)


# ------------------------------------------------------------------------------------------------
# communicators
# ------------------------------------------------------------------------------------------------
class SingleComm:
    rank, world = 0, 1

    def all_reduce_sum(self, vals: Sequence[float]) -> List[float]:
        return list(vals)


class TorchComm:
    """torch.distributed process group: backend 'nccl' is RCCL over xGMI on ROCm, 'gloo' on CPU."""

    def __init__(self, group=None, device=None):
        import torch
        import torch.distributed as dist

        self.torch, self.dist, self.group = torch, dist, group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        self.device = device if device is not None else torch.device("cpu")

    def all_reduce_sum(self, vals):
        t = self.torch.tensor(list(vals), dtype=self.torch.float64, device=self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
        return t.cpu().tolist()

    def all_gather(self, local):
        local = local.contiguous().reshape(-1)
        out = self.torch.empty(self.world * local.numel(), dtype=local.dtype, device=local.device)
        self.dist.all_gather_into_tensor(out, local, group=self.group)
        return out

    def all_to_all_v(self, send, send_counts, recv_counts, rec_len):
        out = self.torch.empty((sum(recv_counts), rec_len), dtype=send.dtype, device=send.device)
        self.dist.all_to_all_single(out, send, output_split_sizes=list(recv_counts), input_split_sizes=list(send_counts),
                                    group=self.group)
        return out


class RcclComm:
    """The engine's own RCCL communicator (cslam_comm_create, include/cslam.h): the sharded resample then runs entirely
    behind the C ABI (cslam_pf_resample_sharded) -- all-gather, the sums and the keep[] plan on the device and one grouped
    send/recv -- with no tensor library in the data path.  The 128-byte unique id is created on rank 0 and handed to
    the other ranks through torch.distributed (any backend; gloo will do), which is used for nothing else."""

    def __init__(self, device: int, group=None):
        import torch
        import torch.distributed as dist

        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        L = _capi.lib()
        buf = (C.c_ubyte * 128)()
        if self.rank == 0:
            check(L.cslam_comm_unique_id(buf))
        t = torch.tensor(list(buf), dtype=torch.uint8)
        backend = dist.get_backend(group)
        if backend == "nccl":
            t = t.cuda(device)
        dist.broadcast(t, src=0, group=group)
        raw = bytes(t.cpu().tolist())
        self._h = C.c_void_p(None)
        check(L.cslam_comm_create(C.c_char_p(raw), C.c_int(self.rank), C.c_int(self.world), C.c_int(device),
                                  C.byref(self._h)))
        self._L = L

    def all_reduce_sum(self, vals):  # (kept for callers that only want the sums)
        raise NotImplementedError("RcclComm is used through ParticleShard.resample_sharded")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.cslam_comm_destroy(self._h)
            self._h = C.c_void_p(None)


class LoopbackComm:
    """One rank of an in-process loopback communicator (cslam_comm_create_loopback): `world` ranks on ONE device, each
    driven from its own host thread.  Lets the multi-rank paths of cslam_pf_resample_sharded run on a one-GPU box."""

    def __init__(self, handle, rank: int, world: int, owner):
        self._h, self.rank, self.world, self._owner = handle, rank, world, owner

    @staticmethod
    def create(world: int, device: int = -1):
        L = _capi.lib()
        arr = (C.c_void_p * world)()
        check(L.cslam_comm_create_loopback(C.c_int(world), C.c_int(device), arr))
        owner = {"L": L, "open": world}
        return [LoopbackComm(C.c_void_p(arr[r]), r, world, owner) for r in range(world)]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._owner["L"].cslam_comm_destroy(self._h)
            self._h = C.c_void_p(None)


# what the read path returns (arrays in the shard's dtype: Xv 3, Pv 3x3, XF 2 x nf, PF 4 x nf, column-major)
BestParticle = namedtuple("BestParticle", "index w Xv Pv XF PF")
Estimate = namedtuple("Estimate", "w_sum neff Xv Pv XF PF")  # XF / PF are None when the map was not asked for
_PICKS = {"max": _capi.PF_PICK_MAX, "min": _capi.PF_PICK_MIN}
# what scores() returns: totals [SCORE_FIELDS] float64, series [records, 4] float32, track [records, 5] float64, calls
PfScores = namedtuple("PfScores", "totals series track calls")
_ESTIMATORS = {"mean": _capi.PF_SCORE_MEAN, "best": _capi.PF_SCORE_BEST}


# ------------------------------------------------------------------------------------------------
# the shard on the GPU
# ------------------------------------------------------------------------------------------------
class ParticleShard:
    def __init__(self, n_particles: int, max_features: int, dtype=np.float32, device: int = -1,
                 quirks: int = Q_REF_EXACT, n_global: int | None = None):
        self.dtype = np.dtype(dtype)
        self._L = _capi.lib()
        self._h = C.c_void_p(None)
        check(self._L.cslam_pf_create(C.c_int(n_particles), C.c_int(max_features),
                                      C.c_int(F32 if self.dtype == np.float32 else F64), C.c_int(device),
                                      C.c_int(quirks), C.byref(self._h)))
        self.n_local = n_particles
        self.n_global = n_global or n_particles
        # PF.cpp:327: w = 1/numParticles of the whole filter
        check(self._L.cslam_pf_set_uniform_weight(self._h, C.c_double(1.0 / self.n_global)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.cslam_pf_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers
    def _m22(self, M):
        return np.asfortranarray(np.asarray(M, dtype=self.dtype).reshape(2, 2))

    def _z(self, Z):
        Z = np.asarray(Z, dtype=self.dtype)
        m = 0 if Z.size == 0 else Z.reshape(2, -1, order="F").shape[1]
        return (np.ascontiguousarray(Z.reshape(-1, order="F")) if m else np.zeros(2, self.dtype)), m

    @property
    def n_features(self) -> int:
        a, b = C.c_int(0), C.c_int(0)
        check(self._L.cslam_pf_get_counts(self._h, C.byref(a), C.byref(b)))
        return b.value

    def synchronize(self):
        check(self._L.cslam_pf_synchronize(self._h))

    def stream_ptr(self) -> int:
        """The hipStream_t every call of this shard is ordered on (e.g. for torch.cuda.ExternalStream and timing events)."""
        p = C.c_void_p(None)
        check(self._L.cslam_pf_get_stream(self._h, C.byref(p)))
        return p.value

    # ---- the per-particle path (every owned particle)
    def predict(self, v, swa, Q, wb, dt):
        """PF::predict -- PF.cpp:419-471."""
        Q = self._m22(Q)
        check(self._L.cslam_pf_predict(self._h, C.c_double(float(v)), C.c_double(float(swa)), _vp(Q),
                                       C.c_double(float(wb)), C.c_double(float(dt))))

    def observe_heading(self, phi, use_heading=False):
        """PF::observeHeading -- PF.cpp:382-417."""
        check(self._L.cslam_pf_observe_heading(self._h, C.c_double(float(phi)), C.c_int(1 if use_heading else 0)))

    def sample_proposal(self, Z, idf, R, normals):
        """PF::sampleProposal -- PF.cpp:502-544. normals: 3 x n_local standard-normal draws (input)."""
        Zc, m = self._z(Z)
        idf = np.ascontiguousarray(idf, dtype=np.int32)
        nrm = np.ascontiguousarray(np.asarray(normals, dtype=self.dtype).reshape(3, self.n_local))
        check(self._L.cslam_pf_sample_proposal(self._h, _vp(Zc), C.c_int(m), _vp(idf) if m else None,
                                               _vp(self._m22(R)), _vp(nrm)))

    def feature_update(self, Z, idf, R):
        """PF::featureUpdate -- PF.cpp:222-277."""
        Zc, m = self._z(Z)
        idf = np.ascontiguousarray(idf, dtype=np.int32)
        check(self._L.cslam_pf_feature_update(self._h, _vp(Zc), C.c_int(m), _vp(idf) if m else None,
                                              _vp(self._m22(R))))

    def add_features(self, Z, R):
        """PF::addOneNewFeature -- PF.cpp:9-60."""
        Zc, q = self._z(Z)
        check(self._L.cslam_pf_add_features(self._h, _vp(Zc), C.c_int(q), _vp(self._m22(R))))

    # ---- unknown correspondences: every particle carries its own association (EKF.cpp:131-144, 235-326 per particle)
    def associate(self, Z, R, gate1, gate2):
        """Gated nearest-neighbour association of the observations Z (2 x m) against every particle's own map
        (cslam_pf_associate).  Fills the shard's device tables; asynchronous.  See association()."""
        Zc, m = self._z(Z)
        self._assoc_m = None  # (a refused call leaves nothing this wrapper can size its buffers from)
        check(self._L.cslam_pf_associate(self._h, _vp(Zc), C.c_int(m), _vp(self._m22(R)), C.c_double(float(gate1)),
                                         C.c_double(float(gate2))))
        self._assoc_m = m

    def association(self):
        """-> (idf, kind, summary) of the last associate(): idf and kind are m x n_local int32 (idf 1-based, 0 = none;
        kind 1 matched, 2 new, 0 ambiguous), summary is m x 4 float64 = (sum w matched, sum w new, sum w ambiguous,
        number of particles matched) over THIS shard's particles."""
        m = getattr(self, "_assoc_m", None)
        if m is None:
            check(self._L.cslam_pf_get_association(self._h, None, None, None))  # raises if associate was never called
            raise _capi.CslamError(_capi.ERR_BAD_ARG, "association(): the last associate() on this shard was refused")
        idf = np.zeros((m, self.n_local), np.int32)
        kind = np.zeros((m, self.n_local), np.int32)
        summary = np.zeros((m, 4), np.float64)
        check(self._L.cslam_pf_get_association(self._h, _vp(idf), _vp(kind), _vp(summary)))
        return idf, kind, summary

    def sample_proposal_assoc(self, Z, R, normals, use=None, miss_likelihood=1.0):
        """PF::sampleProposal + PF::featureUpdate where every particle takes its correspondences from the table of the
        last associate(Z, ...).  use: m flags (default all 1), 0 = nobody sees that observation; a particle without a
        match for a used observation multiplies its weight by miss_likelihood instead."""
        Zc, m = self._z(Z)
        use = np.ones(m, np.int32) if use is None else np.ascontiguousarray(use, dtype=np.int32)
        assert use.shape[0] == m
        nrm = np.ascontiguousarray(np.asarray(normals, dtype=self.dtype).reshape(3, self.n_local))
        check(self._L.cslam_pf_sample_proposal_assoc(self._h, _vp(Zc), C.c_int(m), _vp(self._m22(R)), _vp(nrm),
                                                     _vp(use) if m else None, C.c_double(float(miss_likelihood))))

    def feature_update_assoc(self, Z, R, use=None):
        """PF::featureUpdate alone from the table of the last associate(Z, ...) (the unfused form)."""
        Zc, m = self._z(Z)
        use = np.ones(m, np.int32) if use is None else np.ascontiguousarray(use, dtype=np.int32)
        assert use.shape[0] == m
        check(self._L.cslam_pf_feature_update_assoc(self._h, _vp(Zc), C.c_int(m), _vp(self._m22(R)),
                                                    _vp(use) if m else None))

    # ---- the vote on new features kept on the device: data_associate's policy without the host in the scan
    def associate_vote(self, Z, R, gate1, gate2, new_fraction=0.5, comm=None):
        """associate(Z, ...), then new_feature_votes on the device (cslam_pf_associate_vote): use[], the new observations
        compacted in order and their count stay in HBM for the _voted calls.  comm: the vote reads the sum over the ranks
        of the shards' summaries (cslam_pf_associate_vote_sharded).  Asynchronous; see vote_wait() and vote()."""
        Zc, m = self._z(Z)
        if np.isfinite(float(new_fraction)):  # (a non-finite fraction is refused before anything changes)
            self._assoc_m = None
        args = (_vp(Zc), C.c_int(m), _vp(self._m22(R)), C.c_double(float(gate1)), C.c_double(float(gate2)),
                C.c_double(float(new_fraction)))
        if comm is None:
            check(self._L.cslam_pf_associate_vote(self._h, *args))
        else:
            check(self._L.cslam_pf_associate_vote_sharded(self._h, comm._h, *args))
        self._assoc_m = m
        self._voted(m)

    def _voted(self, m):
        # a refused call leaves the live vote (and its m) as it was; buffers are sized for the largest m ever voted on
        self._vote_m, self._vote_cap = m, max(m, getattr(self, "_vote_cap", 1))

    def vote_wait(self):
        """-> (q, use) of the live vote, waiting for the vote alone and not for what has been queued behind it."""
        m = getattr(self, "_vote_m", 0)
        q, use = C.c_int(0), np.zeros(getattr(self, "_vote_cap", 1), np.int32)
        check(self._L.cslam_pf_vote_wait(self._h, C.byref(q), _vp(use)))
        return q.value, use[:m]

    def vote(self):
        """-> (use [m], new_idx [q], ZN [2 x q], q) of the live vote, read from the device (synchronises)."""
        m, cap = getattr(self, "_vote_m", 0), getattr(self, "_vote_cap", 1)
        use, idx = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        ZN, q = np.zeros((2, cap), self.dtype, order="F"), C.c_int(0)
        check(self._L.cslam_pf_get_vote(self._h, _vp(use), _vp(idx), _vp(ZN), C.byref(q)))
        return use[:m], idx[:q.value], np.asfortranarray(ZN[:, :q.value]), q.value

    def sample_proposal_voted(self, Z, R, normals, miss_likelihood=1.0):
        """sample_proposal_assoc with the mask of the live vote, read on the device."""
        Zc, m = self._z(Z)
        check(self._L.cslam_pf_sample_proposal_voted(self._h, _vp(Zc), C.c_int(m), _vp(self._m22(R)),
                                                     _vp(self._normals(normals)), C.c_double(float(miss_likelihood))))

    def sample_proposal_voted_drawn(self, Z, R, step: int, miss_likelihood=1.0):
        """sample_proposal_assoc_drawn with the mask of the live vote, read on the device."""
        Zc, m = self._z(Z)
        check(self._L.cslam_pf_sample_proposal_voted_drawn(self._h, _vp(Zc), C.c_int(m), _vp(self._m22(R)),
                                                           C.c_double(float(miss_likelihood)), C.c_longlong(int(step))))

    def feature_update_voted(self, Z, R):
        """feature_update_assoc with the mask of the live vote, read on the device."""
        Zc, m = self._z(Z)
        check(self._L.cslam_pf_feature_update_voted(self._h, _vp(Zc), C.c_int(m), _vp(self._m22(R))))

    def add_features_voted(self, R) -> int:
        """add_features of the voted observations, read from the device (cslam_pf_add_features_voted) -> q."""
        q = C.c_int(0)
        check(self._L.cslam_pf_add_features_voted(self._h, _vp(self._m22(R)), C.byref(q)))
        return q.value

    def assoc_scan_step_drawn(self, v, swa, Q, wb, dt, Z, R, gate1, gate2, step: int, n_effective: float,
                              resample_status: bool, new_fraction=0.5, miss_likelihood=1.0) -> int:
        """One scan with unknown correspondences on a shard that holds the whole set, in one C call
        (cslam_pf_assoc_scan_step_drawn): predict, associate_vote, sample_proposal_voted_drawn, resample_local_drawn with
        nothing returned, add_features_voted -> q.  No observations: the predict alone."""
        Zc, m = self._z(Z)
        q = C.c_int(0)
        if m:
            self._assoc_m = None
            self._vote_cap = max(m, getattr(self, "_vote_cap", 1))
        rc = self._L.cslam_pf_assoc_scan_step_drawn(
            self._h, C.c_double(float(v)), C.c_double(float(swa)), _vp(self._m22(Q)), C.c_double(float(wb)),
            C.c_double(float(dt)), _vp(Zc), C.c_int(m), _vp(self._m22(R)), C.c_double(float(gate1)),
            C.c_double(float(gate2)), C.c_double(float(new_fraction)), C.c_double(float(miss_likelihood)),
            C.c_longlong(int(step)), C.c_double(float(n_effective)), C.c_int(1 if resample_status else 0), C.byref(q))
        if m and rc in (_capi.OK, _capi.ERR_CAPACITY):  # (on a capacity overflow the scan ran and its vote is live)
            self._assoc_m = m
            self._voted(m)
        check(rc)
        return q.value

    # ---- a run of control steps in one launch, and the whole iteration block in one call (test/main.cpp:249-334)
    def _controls(self, v, swa, Q, wb, dt, phi, use_heading):
        """-> (arrays kept alive, the C arguments k, v, swa, Q, wb, dt, phi, use_heading).  v and swa: scalars or
        sequences of equal length (a scalar is broadcast to the other's length); a scalar phi is broadcast."""
        va, sa = np.atleast_1d(np.asarray(v, np.float64)), np.atleast_1d(np.asarray(swa, np.float64))
        k = max(va.shape[0], sa.shape[0]) if va.size and sa.size else 0
        if np.ndim(v) == 0:
            va = np.full(k, float(v))
        if np.ndim(swa) == 0:
            sa = np.full(k, float(swa))
        assert va.shape == sa.shape == (k,), "v and swa: scalars or sequences of equal length"
        va, sa = np.ascontiguousarray(va), np.ascontiguousarray(sa)
        pa = None
        if phi is not None:
            pa = np.full(k, float(phi)) if np.ndim(phi) == 0 else np.ascontiguousarray(phi, dtype=np.float64)
            assert pa.shape == (k,), "phi: a scalar or one value per control step"
        Qc = None if Q is None else self._m22(Q)
        keep = (va, sa, pa, Qc)
        return keep, (C.c_int(k), _vp(va), _vp(sa), _vp(Qc) if Qc is not None else None, C.c_double(float(wb)),
                      C.c_double(float(dt)), _vp(pa) if pa is not None else None, C.c_int(1 if use_heading else 0))

    def control_run(self, v, swa, Q, wb, dt, phi=None, use_heading=False):
        """k x (predict(v[j], swa[j], Q, wb, dt); observe_heading(phi[j], use_heading)) for every owned particle -- k
        iterations of test/main.cpp:279-286 -- bit for bit, in one launch per 16 steps (cslam_pf_control_run)."""
        keep, args = self._controls(v, swa, Q, wb, dt, phi, use_heading)
        check(self._L.cslam_pf_control_run(self._h, *args))

    def control_launches(self) -> int:
        """Control-run kernel launches of this shard so far (cslam_pf_control_launches)."""
        n = C.c_longlong(0)
        check(self._L.cslam_pf_control_launches(self._h, C.byref(n)))
        return n.value

    def cycle_drawn(self, v, swa, Q, wb, dt, ZF, idf, ZN, R, step: int, n_effective: float, resample_status: bool,
                    phi=None, use_heading=False):
        """One iteration block of the reference's loop on a shard that holds the whole seeded set, in one C call
        (cslam_pf_cycle_drawn): control_run over all of v / swa / phi, then the scan without a predict of its own.  Known
        features seen (ZF, idf): sample_proposal_drawn, feature_update, resample_local_drawn with nothing returned, then
        add_features(ZN).  Only new ones: new_feature_step_drawn(Q=None).  Neither: the control run alone."""
        keep, args = self._controls(v, swa, Q, wb, dt, phi, use_heading)
        ZFc, mf = self._z(ZF if ZF is not None else [])
        ZNc, mn = self._z(ZN if ZN is not None else [])
        idf = np.ascontiguousarray(idf if mf else [], dtype=np.int32)
        Rc = None if R is None else self._m22(R)
        check(self._L.cslam_pf_cycle_drawn(self._h, *args, _vp(ZFc), C.c_int(mf), _vp(idf) if mf else None, _vp(ZNc),
                                           C.c_int(mn), _vp(Rc) if Rc is not None else None, C.c_longlong(int(step)),
                                           C.c_double(float(n_effective)), C.c_int(1 if resample_status else 0)))

    def assoc_cycle_drawn(self, v, swa, Q, wb, dt, Z, R, gate1, gate2, step: int, n_effective: float,
                          resample_status: bool, phi=None, use_heading=False, new_fraction=0.5,
                          miss_likelihood=1.0) -> int:
        """The same with unknown correspondences (cslam_pf_assoc_cycle_drawn): control_run, then associate_vote,
        sample_proposal_voted_drawn, resample_local_drawn with nothing returned, add_features_voted -> q.  No
        observations: the control run alone."""
        keep, args = self._controls(v, swa, Q, wb, dt, phi, use_heading)
        Zc, m = self._z(Z)
        q = C.c_int(0)
        had_assoc, had_cap = getattr(self, "_assoc_m", None), getattr(self, "_vote_cap", 1)
        if m:
            self._assoc_m = None
            self._vote_cap = max(m, had_cap)
        Rc = None if R is None else self._m22(R)
        rc = self._L.cslam_pf_assoc_cycle_drawn(
            self._h, *args, _vp(Zc), C.c_int(m), _vp(Rc) if Rc is not None else None, C.c_double(float(gate1)),
            C.c_double(float(gate2)), C.c_double(float(new_fraction)), C.c_double(float(miss_likelihood)),
            C.c_longlong(int(step)), C.c_double(float(n_effective)), C.c_int(1 if resample_status else 0), C.byref(q))
        if m and rc in (_capi.OK, _capi.ERR_CAPACITY):  # (on a capacity overflow the scan ran and its vote is live)
            self._assoc_m = m
            self._voted(m)
        elif m:  # (refused before anything was launched: the tables are those of before)
            self._assoc_m = had_assoc
        check(rc)
        return q.value

    # ---- the FastSLAM-1.0 step (slam.h:102): per-particle control noise, likelihood weights, the block in one call
    def control_run_sampled(self, v, swa, Q, wb, dt, ctl_step: int, phi=None, use_heading=False):
        """control_run with every particle's own noisy controls (slam.h:149-159 per particle, Q taken as diagonal): step j
        uses the normals of control step ctl_step + j (synth.pf_control_normals / pf_control_noise restate them).  Any
        shard of a seeded set (cslam_pf_control_run_sampled)."""
        keep, args = self._controls(v, swa, Q, wb, dt, phi, use_heading)
        check(self._L.cslam_pf_control_run_sampled(self._h, *args, C.c_longlong(int(ctl_step))))

    def control_draws(self, ctl_step: int, k: int) -> np.ndarray:
        """-> normals [k, 2, n_local] that control_run_sampled consumes for control steps ctl_step .. ctl_step + k - 1."""
        out = np.zeros((max(int(k), 0), 2, self.n_local), self.dtype)
        check(self._L.cslam_pf_get_control_draws(self._h, C.c_longlong(int(ctl_step)), C.c_int(int(k)), _vp(out)))
        return out

    def likelihood_update(self, Z, idf, R, update_features: bool = True, zero_pv: bool = True):
        """PF::likelihood at every particle's own pose, w <- w * like (PF.cpp:343-359), in one launch; update_features:
        PF::featureUpdate rides along (PF.cpp:222-277); zero_pv: Pv = 0 afterwards (cslam_pf_likelihood_update)."""
        Zc, m = self._z(Z)
        idf = np.ascontiguousarray(idf, dtype=np.int32)
        check(self._L.cslam_pf_likelihood_update(self._h, _vp(Zc), C.c_int(m), _vp(idf) if m else None,
                                                 _vp(self._m22(R)), C.c_int(1 if update_features else 0),
                                                 C.c_int(1 if zero_pv else 0)))

    def fs1_cycle_drawn(self, v, swa, Q, wb, dt, ctl_step: int, ZF, idf, ZN, R, step: int, n_effective: float,
                        resample_status: bool, phi=None, use_heading=False):
        """One iteration block of the FastSLAM-1 loop on a shard that holds the whole seeded set, in one C call
        (cslam_pf_fs1_cycle_drawn): control_run_sampled from ctl_step, then -- known features seen (ZF, idf) --
        likelihood_update(update_features, zero_pv) and resample_local_drawn(step) with nothing returned, then
        add_features(ZN) at every particle's own pose."""
        keep, args = self._controls(v, swa, Q, wb, dt, phi, use_heading)
        ZFc, mf = self._z(ZF if ZF is not None else [])
        ZNc, mn = self._z(ZN if ZN is not None else [])
        idf = np.ascontiguousarray(idf if mf else [], dtype=np.int32)
        Rc = None if R is None else self._m22(R)
        check(self._L.cslam_pf_fs1_cycle_drawn(self._h, *args, C.c_longlong(int(ctl_step)), _vp(ZFc), C.c_int(mf),
                                               _vp(idf) if mf else None, _vp(ZNc), C.c_int(mn),
                                               _vp(Rc) if Rc is not None else None, C.c_longlong(int(step)),
                                               C.c_double(float(n_effective)), C.c_int(1 if resample_status else 0)))

    # ---- pieces of the resample step
    def weight_sums(self) -> Tuple[float, float]:
        s = (C.c_double * 2)()
        check(self._L.cslam_pf_weight_sums(self._h, s))
        return s[0], s[1]

    def scale_weights(self, scale: float):
        check(self._L.cslam_pf_scale_weights(self._h, C.c_double(float(scale))))

    def set_degenerate_policy(self, report: bool):
        """What the resample calls do with a weight sum that is not a positive finite number
        (cslam_pf_set_degenerate_policy): report=True, the rule -- no resample, Neff NaN, weights w / sum w; False (what a
        new shard starts with), the former repair onto particle 0.  resample_particles follows `report_degenerate`."""
        check(self._L.cslam_pf_set_degenerate_policy(self._h, C.c_int(1 if report else 0)))
        self.report_degenerate = bool(report)

    def divide_weights(self, ws: float):
        check(self._L.cslam_pf_divide_weights(self._h, C.c_double(float(ws))))

    def set_uniform_weight(self, w0: float):
        check(self._L.cslam_pf_set_uniform_weight(self._h, C.c_double(float(w0))))

    def get_weights(self) -> np.ndarray:
        w = np.zeros(self.n_local, dtype=self.dtype)
        check(self._L.cslam_pf_get_weights(self._h, _vp(w)))
        return w

    def set_weights(self, w):
        w = np.ascontiguousarray(w, dtype=self.dtype)
        assert w.shape[0] == self.n_local
        check(self._L.cslam_pf_set_weights(self._h, _vp(w)))

    def weights_device_ptr(self) -> int:
        p = C.c_void_p(None)
        check(self._L.cslam_pf_weights_device_ptr(self._h, C.byref(p)))
        return p.value

    @property
    def record_len(self) -> int:
        b = C.c_longlong(0)
        check(self._L.cslam_pf_record_bytes(self._h, C.byref(b)))
        return b.value // self.dtype.itemsize

    def gather_local(self, keep, w_new: float):
        keep = np.ascontiguousarray(keep, dtype=np.int32)
        assert keep.shape[0] == self.n_local
        check(self._L.cslam_pf_gather_local(self._h, _vp(keep), C.c_double(float(w_new))))

    def resample_local(self, select, n_effective: float, resample_status: bool, want_result: bool = True):
        """PF::resampleParticles (PF.cpp:473-500) for a shard that holds every particle, entirely on the device.
        -> (neff, resampled) or None when want_result is False (nothing returns to the host)."""
        select = np.ascontiguousarray(select, dtype=self.dtype)
        assert select.shape[0] == self.n_local
        if not want_result:
            check(self._L.cslam_pf_resample_local(self._h, _vp(select), C.c_double(float(n_effective)),
                                                  C.c_int(1 if resample_status else 0), None, None))
            return None
        neff, did = C.c_double(0.0), C.c_int(0)
        check(self._L.cslam_pf_resample_local(self._h, _vp(select), C.c_double(float(n_effective)),
                                              C.c_int(1 if resample_status else 0), C.byref(neff), C.byref(did)))
        return float(neff.value), bool(did.value)

    def resample_sharded(self, comm: "RcclComm", select, n_effective: float, resample_status: bool):
        """PF::resampleParticles over the particle set sharded across comm.world ranks, behind the C ABI
        (cslam_pf_resample_sharded).  select: the world * n_local strata positions, identical on every rank."""
        select = np.ascontiguousarray(select, dtype=self.dtype)
        assert select.shape[0] == self.n_local * comm.world
        neff, did = C.c_double(0.0), C.c_int(0)
        check(self._L.cslam_pf_resample_sharded(self._h, comm._h, _vp(select), C.c_double(float(n_effective)),
                                                C.c_int(1 if resample_status else 0), C.byref(neff), C.byref(did)))
        return float(neff.value), bool(did.value)

    def debug_last_exchange(self, world: int):
        """(send counts per destination, receive counts per source, local send indices) of the last sharded resample."""
        counts = (C.c_int * (2 * world))()
        n_send = C.c_int(0)
        check(self._L.cslam_pf_debug_last_exchange(self._h, counts, None, C.c_int(0), C.byref(n_send)))
        idx = np.zeros(max(n_send.value, 1), dtype=np.int32)
        if n_send.value:
            check(self._L.cslam_pf_debug_last_exchange(self._h, None, idx.ctypes.data_as(C.c_void_p), C.c_int(idx.shape[0]),
                                                       C.byref(n_send)))
        c = list(counts)
        return c[:world], c[world:], idx[: n_send.value]

    def observation_step(self, v, swa, Q, wb, dt, Z, idf, R, normals, select, n_effective: float, resample_status: bool):
        """predict + sampleProposal + featureUpdate + resampleParticles for a shard that holds every particle, in one
        C call with one staged copy; nothing returns to the host (see resample_stats)."""
        Zc, m = self._z(Z)
        idf = np.ascontiguousarray(idf, dtype=np.int32)
        nrm = np.ascontiguousarray(np.asarray(normals, dtype=self.dtype).reshape(3, self.n_local))
        sel = np.ascontiguousarray(select, dtype=self.dtype)
        assert sel.shape[0] == self.n_local
        check(self._L.cslam_pf_observation_step(self._h, C.c_double(float(v)), C.c_double(float(swa)), _vp(self._m22(Q)),
                                                C.c_double(float(wb)), C.c_double(float(dt)), _vp(Zc), C.c_int(m),
                                                _vp(idf) if m else None, _vp(self._m22(R)), _vp(nrm), _vp(sel),
                                                C.c_double(float(n_effective)), C.c_int(1 if resample_status else 0)))

    # ---- the random inputs drawn on the device (synth.pf_draw_normals / pf_draw_select restate them)
    def seed_draws(self, seed: int, first_global: int = 0, n_global: int | None = None):
        """Seed the draws of the *_drawn calls (cslam_pf_seed_draws).  first_global: the global slot of this shard's
        particle 0; n_global: the size of the whole set (default: the shard's own n_global)."""
        n_global = self.n_global if n_global is None else int(n_global)
        check(self._L.cslam_pf_seed_draws(self._h, C.c_longlong(int(seed)), C.c_longlong(int(first_global)),
                                          C.c_longlong(n_global)))
        self._draw_n = n_global

    def draws(self, step: int, normals: bool = True, select: bool = True):
        """-> (normals 3 x n_local, select n_global) that the *_drawn calls of `step` consume (None where not asked)."""
        n = getattr(self, "_draw_n", None)
        nrm = np.zeros((3, self.n_local), self.dtype) if normals else None
        # (unseeded, or a set beyond 2^31 - 1 that has no strata: the call refuses before it writes)
        sel = np.zeros(n if n and n < 2**31 else 1, self.dtype) if select else None
        check(self._L.cslam_pf_get_draws(self._h, C.c_longlong(int(step)), _vp(nrm) if normals else None,
                                         _vp(sel) if select else None))
        return nrm, sel

    def sample_proposal_drawn(self, Z, idf, R, step: int):
        """sample_proposal with the normals of `step` drawn on the device (streams 0..2)."""
        Zc, m = self._z(Z)
        idf = np.ascontiguousarray(idf, dtype=np.int32)
        check(self._L.cslam_pf_sample_proposal_drawn(self._h, _vp(Zc), C.c_int(m), _vp(idf) if m else None,
                                                     _vp(self._m22(R)), C.c_longlong(int(step))))

    def sample_proposal_assoc_drawn(self, Z, R, step: int, use=None, miss_likelihood=1.0):
        """sample_proposal_assoc with the normals of `step` drawn on the device."""
        Zc, m = self._z(Z)
        use = np.ones(m, np.int32) if use is None else np.ascontiguousarray(use, dtype=np.int32)
        assert use.shape[0] == m
        check(self._L.cslam_pf_sample_proposal_assoc_drawn(self._h, _vp(Zc), C.c_int(m), _vp(self._m22(R)),
                                                           _vp(use) if m else None, C.c_double(float(miss_likelihood)),
                                                           C.c_longlong(int(step))))

    def resample_local_drawn(self, step: int, n_effective: float, resample_status: bool, want_result: bool = True):
        """resample_local with the strata of `step` drawn on the device (stream 3)."""
        neff, did = C.c_double(0.0), C.c_int(0)
        check(self._L.cslam_pf_resample_local_drawn(self._h, C.c_longlong(int(step)), C.c_double(float(n_effective)),
                                                    C.c_int(1 if resample_status else 0),
                                                    C.byref(neff) if want_result else None,
                                                    C.byref(did) if want_result else None))
        return (float(neff.value), bool(did.value)) if want_result else None

    def resample_sharded_drawn(self, comm, step: int, n_effective: float, resample_status: bool):
        """resample_sharded with the strata of `step` drawn on every rank's device: nobody distributes select."""
        neff, did = C.c_double(0.0), C.c_int(0)
        check(self._L.cslam_pf_resample_sharded_drawn(self._h, comm._h, C.c_longlong(int(step)),
                                                      C.c_double(float(n_effective)), C.c_int(1 if resample_status else 0),
                                                      C.byref(neff), C.byref(did)))
        return float(neff.value), bool(did.value)

    def observation_step_drawn(self, v, swa, Q, wb, dt, Z, idf, R, step: int, n_effective: float, resample_status: bool):
        """observation_step with every random input of `step` drawn on the device: launches only when m <= 32."""
        Zc, m = self._z(Z)
        idf = np.ascontiguousarray(idf, dtype=np.int32)
        check(self._L.cslam_pf_observation_step_drawn(self._h, C.c_double(float(v)), C.c_double(float(swa)),
                                                      _vp(self._m22(Q)), C.c_double(float(wb)), C.c_double(float(dt)),
                                                      _vp(Zc), C.c_int(m), _vp(idf) if m else None, _vp(self._m22(R)),
                                                      C.c_longlong(int(step)), C.c_double(float(n_effective)),
                                                      C.c_int(1 if resample_status else 0)))

    # ---- the scan that observes only new features (test/main.cpp:314-328)
    def _normals(self, normals):
        return np.ascontiguousarray(np.asarray(normals, dtype=self.dtype).reshape(3, self.n_local))

    def sample_pose(self, normals):
        """X <- X + chol(P) z, P <- 0 for every owned particle (test/main.cpp:321-324, slam.h:753-764, 413-436); the
        weights stay.  normals: 3 x n_local standard-normal draws (input)."""
        check(self._L.cslam_pf_sample_pose(self._h, _vp(self._normals(normals))))

    def sample_pose_drawn(self, step: int):
        """sample_pose with the normals of `step` drawn on the device (streams 0..2); any shard of a seeded set."""
        check(self._L.cslam_pf_sample_pose_drawn(self._h, C.c_longlong(int(step))))

    def _new_feature_args(self, v, swa, Q, wb, dt, Z, R):
        Zc, q = self._z(Z)
        Qc = None if Q is None else self._m22(Q)
        Rc = None if R is None else self._m22(R)
        keep = (Zc, Qc, Rc)  # (alive until the call has consumed them)
        return keep, (C.c_double(float(v)), C.c_double(float(swa)), _vp(Qc) if Qc is not None else None,
                      C.c_double(float(wb)), C.c_double(float(dt)), _vp(Zc), C.c_int(q),
                      _vp(Rc) if Rc is not None else None)

    def new_feature_step(self, v, swa, Q, wb, dt, Z, R, normals):
        """The whole all-new scan in one launch (test/main.cpp:314-328): predict (PF.cpp:419-471; Q=None: none), sample
        the pose, zero Pv, add the features Z (2 x q) at the sampled pose (PF.cpp:9-60)."""
        keep, args = self._new_feature_args(v, swa, Q, wb, dt, Z, R)
        check(self._L.cslam_pf_new_feature_step(self._h, *args, _vp(self._normals(normals))))

    def new_feature_step_drawn(self, v, swa, Q, wb, dt, Z, R, step: int):
        """new_feature_step with the normals of `step` drawn on the device: launches only when q <= 32."""
        keep, args = self._new_feature_args(v, swa, Q, wb, dt, Z, R)
        check(self._L.cslam_pf_new_feature_step_drawn(self._h, *args, C.c_longlong(int(step))))

    def scan_step_drawn(self, v, swa, Q, wb, dt, ZF, idf, ZN, R, step: int, n_effective: float, resample_status: bool):
        """One scan of the reference's loop (test/main.cpp:279-328) on a shard that holds the whole set, every random
        input of `step` drawn on the device.  ZF / idf: the observations of known features, ZN: those of new ones.
        Known features seen: observation_step_drawn, then add_features(ZN) at the proposal's pose.  Only new ones:
        new_feature_step_drawn (the pose is sampled, Pv zeroed, the features added there).  Neither: predict."""
        mf = 0 if ZF is None else self._z(ZF)[1]
        mn = 0 if ZN is None else self._z(ZN)[1]
        if mf > 0:
            self.observation_step_drawn(v, swa, Q, wb, dt, ZF, idf, R, step, n_effective, resample_status)
            if mn > 0:
                self.add_features(ZN, R)
        elif mn > 0:
            self.new_feature_step_drawn(v, swa, Q, wb, dt, ZN, R, step)
        else:
            self.predict(v, swa, Q, wb, dt)

    def stage_copies(self) -> int:
        """Host-to-device copy commands this shard has enqueued for per-step inputs (cslam_pf_stage_copies)."""
        n = C.c_longlong(0)
        check(self._L.cslam_pf_stage_copies(self._h, C.byref(n)))
        return n.value

    def resample_stats(self):
        """(resample calls, resamples performed, last Neff) from the device-side counters."""
        a, b, c = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        check(self._L.cslam_pf_resample_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), float(c.value)

    def pack_into(self, src_idx: np.ndarray, dptr: int):
        src_idx = np.ascontiguousarray(src_idx, dtype=np.int32)
        check(self._L.cslam_pf_pack(self._h, _vp(src_idx), C.c_int(src_idx.shape[0]), C.c_void_p(dptr)))

    def unpack_from(self, dst_idx: np.ndarray, dptr: int):
        dst_idx = np.ascontiguousarray(dst_idx, dtype=np.int32)
        check(self._L.cslam_pf_unpack(self._h, _vp(dst_idx), C.c_int(dst_idx.shape[0]), C.c_void_p(dptr)))

    # torch-tensor flavoured pack/unpack used by resample_particles (device buffers come from torch: plumbing)
    def pack(self, src_idx):
        import torch

        tdt = torch.float32 if self.dtype == np.float32 else torch.float64
        buf = torch.empty((len(src_idx), self.record_len), dtype=tdt, device="cuda")
        if len(src_idx):
            self.pack_into(src_idx, buf.data_ptr())
        return buf

    def unpack(self, dst_idx, buf):
        import torch

        if len(dst_idx):
            torch.cuda.synchronize()
            self.unpack_from(dst_idx, buf.contiguous().data_ptr())

    def weights_tensor(self):
        import torch

        return torch.from_numpy(self.get_weights()).cuda()

    # ---- host access to single particles (tests, reporting)
    def get_particle(self, i: int):
        nf = self.n_features
        w = np.zeros(1, self.dtype)
        Xv = np.zeros(3, self.dtype)
        Pv = np.zeros((3, 3), self.dtype, order="F")
        XF = np.zeros((2, nf), self.dtype, order="F")
        PF = np.zeros((4, nf), self.dtype, order="F")
        check(self._L.cslam_pf_get_particle(self._h, C.c_int(i), _vp(w), _vp(Xv), _vp(Pv), _vp(XF) if nf else None,
                                            _vp(PF) if nf else None))
        return w[0], Xv, Pv, XF, PF

    # ---- the estimate, read from the set in HBM (no per-particle downloads)
    def _record(self, with_map: bool):
        nf = self.n_features if with_map else 0
        bufs = [np.zeros(3, self.dtype), np.zeros((3, 3), self.dtype, order="F"),
                np.zeros((2, nf), self.dtype, order="F"), np.zeros((4, nf), self.dtype, order="F")]
        ptrs = [_vp(bufs[0]), _vp(bufs[1]), _vp(bufs[2]) if nf else None, _vp(bufs[3]) if nf else None]
        return bufs, ptrs

    def best_particle(self, pick: str = "max") -> BestParticle:
        """Slam::extractStatesFromParticles -- slam.h:493-511 -- with the whole record of the chosen particle.
        pick="max": the maximum-weight particle; "min": the reference's own choice (slam.h:505-506)."""
        bufs, ptrs = self._record(True)
        w, idx = np.zeros(1, self.dtype), C.c_int(0)
        check(self._L.cslam_pf_best_particle(self._h, C.c_int(_PICKS[pick]), C.byref(idx), _vp(w), *ptrs))
        return BestParticle(idx.value, w[0], *bufs)

    def best_particle_sharded(self, comm, pick: str = "max") -> BestParticle:
        """best_particle over the set sharded across comm.world ranks; index is the GLOBAL index."""
        bufs, ptrs = self._record(True)
        w, idx = np.zeros(1, self.dtype), C.c_longlong(0)
        check(self._L.cslam_pf_best_particle_sharded(self._h, comm._h, C.c_int(_PICKS[pick]), C.byref(idx), _vp(w), *ptrs))
        return BestParticle(idx.value, w[0], *bufs)

    def _estimate(self, comm, want_map: bool) -> Estimate:
        bufs, ptrs = self._record(want_map)
        ws, ne = C.c_double(0.0), C.c_double(0.0)
        if comm is None:
            check(self._L.cslam_pf_estimate(self._h, C.byref(ws), C.byref(ne), *ptrs))
        else:
            check(self._L.cslam_pf_estimate_sharded(self._h, comm._h, C.byref(ws), C.byref(ne), *ptrs))
        if not want_map:
            bufs[2:] = [None, None]
        return Estimate(float(ws.value), float(ne.value), *bufs)

    def estimate(self, want_map: bool = True) -> Estimate:
        """Moments of the weighted mixture (cslam_pf_estimate): sum w, Neff, the pose mean (circular in the heading) and
        covariance, and -- unless want_map is False -- every feature's mean and covariance."""
        return self._estimate(None, want_map)

    def estimate_sharded(self, comm, want_map: bool = True) -> Estimate:
        """estimate over the set sharded across comm.world ranks: identical bits on every rank."""
        return self._estimate(comm, want_map)

    # ---- the score of the estimate and its trajectory log, kept on the device (cslam_pf_score*)
    def score_reset(self, estimator: str = "mean", series_capacity: int = 0, gate_pose: float = 0.0, gate_lm: float = 0.0):
        """Zero the totals, the series, the track and the call count; estimator "mean" scores what estimate() returns,
        "best" what best_particle("max") returns.  A gate <= 0 selects the 95 % chi-square point.  Keeps the truth."""
        est = _ESTIMATORS[estimator] if isinstance(estimator, str) else int(estimator)
        check(self._L.cslam_pf_score_reset(self._h, C.c_int(est), C.c_int(int(series_capacity)),
                                           C.c_double(float(gate_pose)), C.c_double(float(gate_lm))))

    def score_set_truth(self, lm_true):
        """Row j of lm_true ([count, 2]) is the true position of state feature j + 1."""
        t = np.ascontiguousarray(np.asarray(lm_true, dtype=np.float64).reshape(-1, 2))
        check(self._L.cslam_pf_score_set_truth(self._h, _vp(t) if t.size else None, C.c_int(t.shape[0])))

    @staticmethod
    def _xv_true(xv_true):
        return np.ascontiguousarray(np.asarray(xv_true, dtype=np.float64).reshape(3))

    def score(self, xv_true, with_map: bool = True):
        """One score step of the current estimate against the true pose (cslam_pf_score): asynchronous, nothing returns."""
        x = self._xv_true(xv_true)
        check(self._L.cslam_pf_score(self._h, _vp(x), C.c_int(1 if with_map else 0)))

    def score_sharded(self, comm, xv_true, with_map: bool = True):
        """score over the set sharded across comm.world ranks: every rank ends with identical totals, series and track."""
        x = self._xv_true(xv_true)
        check(self._L.cslam_pf_score_sharded(self._h, comm._h, _vp(x), C.c_int(1 if with_map else 0)))

    def scores(self, capacity_records: int | None = None) -> PfScores:
        """The one synchronising call of the score (cslam_pf_get_scores): totals, the series and track records held (at
        most capacity_records of them) and the number of score calls since the reset."""
        rec, calls = C.c_int(0), C.c_longlong(0)
        check(self._L.cslam_pf_get_scores(self._h, None, None, None, C.c_int(0), C.byref(rec), C.byref(calls)))
        n = rec.value if capacity_records is None else min(rec.value, int(capacity_records))
        totals = np.zeros(_capi.SCORE_FIELDS, np.float64)
        series = np.zeros((n, _capi.PF_SCORE_SERIES), np.float32)
        track = np.zeros((n, _capi.PF_SCORE_TRACK), np.float64)
        check(self._L.cslam_pf_get_scores(self._h, _vp(totals), _vp(series) if n else None, _vp(track) if n else None,
                                          C.c_int(n), C.byref(rec), C.byref(calls)))
        return PfScores(totals, series, track, int(calls.value))

    def all_features(self) -> np.ndarray:
        """Slam::extractFeaturesFromParticles -- slam.h:513-539: 2 x (n_local * nf), particle p's block at column p * nf."""
        out = np.zeros((2, self.n_local * self.n_features), self.dtype, order="F")
        if out.size:
            check(self._L.cslam_pf_get_all_features(self._h, _vp(out)))
        return out

    def set_particle(self, i: int, w, Xv, Pv, XF, PF):
        XF = np.asfortranarray(np.asarray(XF, dtype=self.dtype).reshape(2, -1, order="F"))
        nf = XF.shape[1]
        PF = np.asfortranarray(np.asarray(PF, dtype=self.dtype).reshape(4, -1, order="F"))
        wv = np.array([w], dtype=self.dtype)
        Xv = np.ascontiguousarray(Xv, dtype=self.dtype)
        Pv = np.asfortranarray(np.asarray(Pv, dtype=self.dtype).reshape(3, 3))
        check(self._L.cslam_pf_set_particle(self._h, C.c_int(i), _vp(wv), _vp(Xv), _vp(Pv), _vp(XF) if nf else None,
                                            _vp(PF) if nf else None, C.c_int(nf)))


# ------------------------------------------------------------------------------------------------
# PF::resampleParticles over a sharded particle set
# ------------------------------------------------------------------------------------------------
def _sum_usable(ws: float) -> bool:
    return 0.0 < ws <= float(np.finfo(np.float64).max)


def normalise_weights(shard, ws: float):
    """w / ws on the shard by the device's rule (pf_kernels.hpp, at pf_use_scale): the scale 1/ws where it is a normal
    number of the particle dtype, as ever; a division where it overflows (a subnormal sum) or is subnormal (a sum near
    the top of the range), and for a sum that is not a positive finite number on a shard whose `report_degenerate` is set
    (the IEEE quotients NaN / 0 are the answer).  Such a sum is scaled as ever otherwise."""
    fi = np.finfo(np.dtype(shard.dtype))
    if _sum_usable(ws):
        if not float(fi.tiny) <= 1.0 / ws <= float(fi.max):
            shard.divide_weights(ws)
            return
    elif getattr(shard, "report_degenerate", False):
        shard.divide_weights(ws)
        return
    shard.scale_weights(1.0 / ws)


def resample_particles(shard, comm, n_effective: int, resample_status: bool, select: np.ndarray | None = None,
                       uniforms: np.ndarray | None = None, step: int | None = None):
    """PF::resampleParticles(particles, numEffective, resampleStatus) -- PF.cpp:473-500 -- for the particle set
    block-partitioned over comm.world shards.  `shard` is a ParticleShard (or anything with its resample
    surface: weight_sums, scale_weights, weights_tensor, pack, unpack, gather_local, set_uniform_weight,
    n_local, dtype).  `select` are the N strata positions (PF.cpp:557); when None they are built from
    `uniforms` (N uniform[0,1) draws that every rank must pass identically).  With `step` (and neither of the two) the
    strata are drawn on the device of a shard seeded with seed_draws: resample_local_drawn for one shard,
    resample_sharded_drawn over an RcclComm.  Returns (neff, resampled)."""
    n_local = shard.n_local
    n = n_local * comm.world
    if step is not None:
        assert select is None and uniforms is None, "step= draws the strata on the device: pass no select / uniforms"
        if comm.world == 1:
            return shard.resample_local_drawn(step, n_effective, resample_status)
        assert isinstance(comm, (RcclComm, LoopbackComm)), "the drawn sharded resample runs behind the C ABI"
        return shard.resample_sharded_drawn(comm, step, n_effective, resample_status)
    if comm.world == 1 and hasattr(shard, "resample_local") and not getattr(shard, "host_resample", False):
        # one shard holds everything: sums, normalisation, Neff, decision, keep[] and the moves stay on the device
        if select is None:
            assert uniforms is not None, "pass select[] or the uniform draws it is built from"
            select = stratified_random(n, uniforms, shard.dtype)
        return shard.resample_local(np.asarray(select, dtype=shard.dtype), n_effective, resample_status)
    if isinstance(comm, RcclComm):
        # sharded over GPUs: the three collectives, the plan and the moves all run behind the C ABI on the device
        if select is None:
            assert uniforms is not None, "pass select[] or the uniform draws it is built from"
            select = stratified_random(n, uniforms, shard.dtype)
        return shard.resample_sharded(comm, select, n_effective, resample_status)
    s1, s2 = shard.weight_sums()
    ws, ws2 = comm.all_reduce_sum([s1, s2])          # collective 1: two scalars
    normalise_weights(shard, ws)                      # PF.cpp:482-487
    if not _sum_usable(ws) and getattr(shard, "report_degenerate", False):
        return float("nan"), False                   # cslam.h, DEGENERATE SUMS: no Neff, no resample
    neff = (ws * ws) / ws2 if ws2 > 0 else 0.0        # 1 / sum (w/ws)^2, PF.cpp:549-554
    fmax, fmin = float(np.finfo(np.float64).max), float(np.finfo(np.float64).tiny)
    if np.dtype(shard.dtype).itemsize == 8 and _sum_usable(ws) and not (fmin <= ws2 <= fmax and ws * ws <= fmax):
        s1, s2 = comm.all_reduce_sum(list(shard.weight_sums()))  # f64: the raw squares left the range of double,
        neff = (s1 * s1) / s2                                    # those of the normalised weights have not
    if not (neff < n_effective and resample_status):  # PF.cpp:490
        return neff, False
    if comm.world == 1:
        w_all = shard.get_weights()
    else:
        w_all = comm.all_gather(shard.weights_tensor()).cpu().numpy()  # collective 2: N weights
    w_all = np.ascontiguousarray(w_all, dtype=shard.dtype)
    if select is None:
        assert uniforms is not None, "pass select[] or the uniform draws it is built from"
        select = stratified_random(n, uniforms, shard.dtype)
    keep = stratified_keep(w_all, np.asarray(select, dtype=shard.dtype))
    if comm.world == 1:
        shard.gather_local(keep, 1.0 / n)
        return neff, True
    send_src, send_counts, recv_dst, recv_counts = plan_exchange(keep, comm.rank, comm.world, n_local)
    send = shard.pack(send_src)
    rec_len = send.shape[1]
    recv = comm.all_to_all_v(send, send_counts, recv_counts, rec_len)  # collective 3: particle records
    shard.unpack(recv_dst, recv)
    shard.set_uniform_weight(1.0 / n)                 # PF.cpp:495
    return neff, True


# ------------------------------------------------------------------------------------------------
# what to do with the association: a policy, and it lives on the host
# ------------------------------------------------------------------------------------------------
def new_feature_votes(summary: np.ndarray, new_fraction: float = 0.5) -> np.ndarray:
    """Per observation: does the weight mass of the particles that call it NEW reach new_fraction of the whole?
    summary: m x 4 as ParticleShard.association() returns it (a sharded caller passes the sum over the shards).
    An observation nobody calls new, or a set without weight mass, is never new (whatever new_fraction is)."""
    summary = np.asarray(summary, dtype=np.float64).reshape(-1, 4)
    total = summary[:, :3].sum(axis=1)
    return (total > 0) & (summary[:, 1] > 0) & (summary[:, 1] >= new_fraction * total)


def data_associate(shard, Z, R, gate1, gate2, new_fraction: float = 0.5):
    """One policy for a FastSLAM-2 step with unknown correspondences -> (use, ZN).

    The C ABI supplies the mechanism only (cslam_pf_associate and the consumers that read its table); which
    observations become new features is decided HERE, on the host, because the feature index space is shared by all
    particles: observation j is declared new, for every particle, when summary[j].new / sum w >= new_fraction.  Then
    use[j] = 0 (no particle updates from it) and its column goes to ZN for add_features after the resample; every other
    observation keeps use[j] = 1, and a particle that has no match for it pays miss_likelihood in sample_proposal_assoc."""
    shard.associate(Z, R, gate1, gate2)
    _, _, summary = shard.association()
    Z = np.asarray(Z, dtype=shard.dtype)
    Z = Z.reshape(2, -1, order="F") if Z.size else np.zeros((2, 0), shard.dtype)
    new = new_feature_votes(summary, new_fraction) if summary.shape[0] else np.zeros(0, bool)
    use = np.where(new, 0, 1).astype(np.int32)
    return use, np.asfortranarray(Z[:, new])
