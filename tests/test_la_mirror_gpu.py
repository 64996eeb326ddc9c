"""Look-ahead windows that read the pending panels' rows from the row-major mirror the k = 64 wide kernel leaves behind
(ekf_lookahead.hpp: MIRROR forms of ekf_la_wide_body and ekf_la_blocks_impl) and launch no rows kernel.

Every comparison is bitwise, on get_state(): the other side is the SAME call sequence with CSLAM_LA_MIRROR=0, the rows +
blocks path with the wide kernel that stores no mirror.  Each side runs in a fresh child process of its own (this file,
run as a script: the switch is read when the engine is created; every case in turn, one handle alive at a time) and
leaves its results in an .npz file; the tests below compare the two files.  One case per shape also goes against the
oracle, with the helpers and tolerances of tests/test_timed_path_gpu.py for this path.

Shapes: N = 40 (n = 83: one 128-row tile, a last block of 32 rows that is partly beyond n) and N = 70 (n = 143: crosses
the tile edge; landmark 63 has rows 127 and 128); f32, TEXTBOOK, a deferral window of 128 columns, CSLAM_LOOKAHEAD=1,
m = 32 observations per update (the k = 64 form of the wide kernel) unless a case says otherwise.

Feature ids of the 8 updates (windows are the pairs (0, 1), (2, 3), ...): landmarks 1 and N in update 0, landmark 2 in
updates 0 and 1 (both updates of one window), landmark 3 in updates 1 and 2 (two consecutive windows), landmark 63 in
every update at N = 70; the rest at random, so most landmarks recur anyway.

How many rows kernels a sequence launches with the mirror (rows_launches()): a window launches one exactly when it starts
from pending columns the mirror does not cover.  A window that starts from an EMPTY pending store needs no panel rows and
takes the mirror form too, so the plain sequence, a flush() and a set_deferred() change launch none at all; the window
after a general-wide window (its 104 columns have no mirror) and the window after a classic update (its 16 columns
neither) launch one each.  With CSLAM_LA_MIRROR=0 every window launches one.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conan_slam_amd.synth import Workload, normal  # noqa: E402

pytestmark = pytest.mark.gpu

TEXTBOOK = 0
F32 = np.float32
SHAPES = (40, 70)
M = 32
STEPS = 8


class _Picked(Workload):
    """The synthetic workload of the timed path with feature ids chosen here (per update: m_of[t] of them)."""

    def __init__(self, N):
        super().__init__(N, M, F32)
        rng = np.random.default_rng(4000 + N)
        self.m_of = [M] * STEPS
        self.picks = []
        for t in range(STEPS):
            must = {0: [1, N, 2], 1: [2, 3], 2: [3]}.get(t, []) + ([63] if N >= 63 else [])
            rest = [int(f) for f in rng.permutation(N) + 1 if f not in must]
            idf = np.array(must + rest[: M - len(must)], dtype=np.int32)
            self.picks.append(idf[rng.permutation(M)])

    def observations(self, t):
        idf = self.picks[t][: self.m_of[t]]
        m, s = len(idf), 1000 * self.seed
        pose = self.true_pose_after(t)
        dx, dy = self.LM[0, idf - 1] - pose[0], self.LM[1, idf - 1] - pose[1]
        nz = normal(s + 5 + 104729 * (t + 1), np.arange(2 * m, dtype=np.uint64))
        Z = np.empty((2, m), dtype=np.float64)
        Z[0] = np.sqrt(dx * dx + dy * dy) + nz[0::2] * np.sqrt(float(self.R[0, 0]))
        Z[1] = np.arctan2(dy, dx) - pose[2] + nz[1::2] * np.sqrt(float(self.R[1, 1]))
        return np.asfortranarray(Z.astype(self.dtype)), idf.copy()


def _inputs(N, m_of=None):
    w = _Picked(N)
    if m_of:
        w.m_of = list(m_of)
    ctrl = [w.controls(t) for t in range(STEPS)]
    obs = [w.observations(t) for t in range(STEPS)]
    return w, ctrl, obs


# ------------------------------------------------------------------------------------------------ the child's side
def _run(N, between=None, m_of=None, mode="dev"):
    """8 predict + update steps as bench.py drives them (async, update_device, a deferral window of 128); `between` is
    called once after update 3 (two windows).  mode: "dev" (device buffers of their own), "host" (host pointers),
    "streams" (ONE device buffer pair, rewritten after waiting for the handle's streams only)."""
    import torch

    from conan_slam_amd import EKF

    w, ctrl, obs = _inputs(N, m_of)
    e = EKF(N, dtype=F32, quirks=TEXTBOOK, sync_mode=False)
    e.set_state(w.X0, w.P0)
    e.set_deferred(128)
    keep = []
    dZ = torch.zeros(2 * M, dtype=torch.float32, device="cuda")
    dI = torch.zeros(M, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ext = [torch.cuda.ExternalStream(p) for p in dict.fromkeys(e.streams()) if p]
    for t in range(STEPS):
        if between is not None and t == 4:
            between(e, w)
        Z, idf = obs[t]
        m = len(idf)
        e.predict(*ctrl[t], w.QE, w.wb, w.dt)
        zf = np.ascontiguousarray(Z.reshape(-1, order="F"))
        if mode == "host":
            e.update(Z, w.RE, idf, True)
        elif mode == "dev":
            sZ, sI = torch.from_numpy(zf).cuda(), torch.from_numpy(idf).cuda()
            torch.cuda.synchronize()
            keep += [sZ, sI]
            e.update_device(sZ.data_ptr(), m, w.RE, sI.data_ptr(), batch=True)
        else:
            # cslam.h: the caller's buffers may be rewritten "once the handle's streams have been synchronised".  Nothing
            # here waits for the device as a whole, so the engine's internal chain stream is not covered: with the wide
            # launch held, update b's buffers are read by main-stream kernels of b's call only -- with the mirror that is
            # the blocks kernel alone, which also keeps the copies the chain kernel and the held wide kernel read.
            sZ, sI = torch.from_numpy(zf).cuda(), torch.from_numpy(idf).cuda()
            keep += [sZ, sI]
            torch.cuda.current_stream().synchronize()
            for st in ext:
                st.synchronize()
            dZ[: 2 * m].copy_(sZ)
            dI[:m].copy_(sI)
            torch.cuda.current_stream().synchronize()
            e.update_device(dZ.data_ptr(), m, w.RE, dI.data_ptr(), batch=True)
    tr = e.trace()  # (flushes what is pending)
    X, P = e.get_state()
    out = {"X": X, "P": P, "trace": tr, "counts": [e.lookahead_windows(), e.rows_launches(), e.factor_status(),
                                                    e.stage_launches()]}
    e.close()
    return out


def _classic_m8(e, w):
    """an update of 8 observations (k = 16: below the windows' range, the classic deferred path)"""
    ww = _Picked(w.N)
    ww.m_of = [8] * STEPS
    Z, idf = ww.observations(0)
    e.predict(w.v, 0.0, w.QE, w.wb, w.dt)
    e.update(Z, w.RE, idf, True)


def _set_deferred(e, w):
    e.set_deferred(0)
    e.set_deferred(128)


CASES = {
    "steady": dict(),
    "general": dict(m_of=[M, M, M, 20, M, M, M, M]),  # window 1 ends in the general wide kernel: window 2 falls back
    "classic": dict(between=_classic_m8),
    "flush": dict(between=lambda e, w: e.flush()),
    "set_deferred": dict(between=_set_deferred),
    "streams": dict(mode="streams"),
    "streams_host": dict(mode="host"),
}
# rows_launches() with the mirror / lookahead_windows(), see the module docstring
ROWS_MIRROR = {"steady": 0, "general": 1, "classic": 1, "flush": 0, "set_deferred": 0, "streams": 0, "streams_host": 0}
WINDOWS = 4


def _child_main(path):
    res = {}
    for N in SHAPES:
        for name, kw in CASES.items():
            r = _run(N, **kw)
            cid = f"{name}-N{N}"
            res[cid + "/X"] = r["X"]
            res[cid + "/Psha"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(r["P"]).tobytes()).digest(), np.uint8)
            res[cid + "/counts"] = np.array(r["counts"], dtype=np.int64)
            if name == "steady":
                res[cid + "/P"] = r["P"]
                res[cid + "/trace"] = np.array([r["trace"]], dtype=np.float64)
    np.savez(path, **res)


# ------------------------------------------------------------------------------------------------ the tests' side
def _run_child(path, mirror):
    env = dict(os.environ)
    env["CSLAM_LOOKAHEAD"] = "1"
    env["CSLAM_LA_MIRROR"] = mirror
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, f"child (CSLAM_LA_MIRROR={mirror}) ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(gpu_required, tmp_path_factory):
    d = tmp_path_factory.mktemp("la_mirror")
    return {mirror: _run_child(str(d / f"mirror{mirror}.npz"), mirror) for mirror in ("1", "0")}


def _same(runs, cid, other=None, other_mirror="0"):
    """bitwise: case cid with the mirror against case `other` (default: itself) under other_mirror; no factor flags"""
    a, b, oid = runs["1"], runs[other_mirror], other or cid
    dx = float(np.abs(a[cid + "/X"].astype(np.float64) - b[oid + "/X"].astype(np.float64)).max())
    print(f"{cid} vs {oid} (mirror {other_mirror}): max |dX| = {dx:.3e}, counts {a[cid + '/counts']} / {b[oid + '/counts']}")
    assert a[cid + "/counts"][2] == 0 and b[oid + "/counts"][2] == 0, "factor_status"
    assert a[cid + "/counts"][0] == b[oid + "/counts"][0], "lookahead_windows differ"
    assert np.array_equal(a[cid + "/X"], b[oid + "/X"]), f"X differs: max |dX| = {dx:.3e}"
    assert np.array_equal(a[cid + "/Psha"], b[oid + "/Psha"]), "P differs"


@pytest.mark.parametrize("N", SHAPES)
def test_four_windows_bitwise_and_no_rows_kernel(runs, N):
    """Four consecutive windows of two 32-observation updates: X and the full P bit for bit those of CSLAM_LA_MIRROR=0, no
    factor flag, and no rows kernel at all with the mirror (the first window starts from an empty pending store and needs
    no panel rows; every later one finds all 128 pending columns mirrored) against one per window without."""
    cid = f"steady-N{N}"
    _same(runs, cid)
    assert np.array_equal(runs["1"][cid + "/P"], runs["0"][cid + "/P"])
    assert int(runs["1"][cid + "/counts"][0]) == WINDOWS
    assert int(runs["1"][cid + "/counts"][1]) == 0, "rows kernel launches with the mirror"
    assert int(runs["0"][cid + "/counts"][1]) == WINDOWS, "rows kernel launches with CSLAM_LA_MIRROR=0"


@pytest.mark.parametrize("case", ["general", "classic", "flush", "set_deferred"])
@pytest.mark.parametrize("N", SHAPES)
def test_windows_fall_back_where_the_mirror_does_not_cover_the_store(runs, N, case):
    """general: the second window's b has m = 20, so that window ends in the general wide kernel, which writes no mirror,
    and the third window must take the rows + blocks path.  classic: an m = 8 update (classic deferred path) between
    windows 2 and 3 leaves 16 unmirrored columns.  flush / set_deferred: the store is applied between the windows, and the
    next window starts from an empty one.  Each bit for bit the CSLAM_LA_MIRROR=0 run, with the rows launches the module
    docstring derives."""
    cid = f"{case}-N{N}"
    _same(runs, cid)
    assert int(runs["1"][cid + "/counts"][0]) == WINDOWS
    assert int(runs["1"][cid + "/counts"][1]) == ROWS_MIRROR[case], "rows kernel launches with the mirror"
    assert int(runs["0"][cid + "/counts"][1]) == WINDOWS, "rows kernel launches with CSLAM_LA_MIRROR=0"


@pytest.mark.parametrize("N", SHAPES)
def test_mirror_windows_match_the_oracle(runs, N):
    """The four-window case against the oracle's plain sequence: test_timed_path_gpu.py's comparison for this path
    (1e-5 on X, 1e-4 on P and the trace, the f64 oracle as the fairness reference), so that a fault common to both forms
    of the blocks kernel still shows."""
    from pyoracle import TEXTBOOK as O_TEXTBOOK
    from test_timed_path_gpu import _compare, _run_oracle

    cid = f"steady-N{N}"
    w, ctrl, obs = _inputs(N)
    inputs = (ctrl, [0.0] * STEPS, obs)
    Xo, Po, codes = _run_oracle(w, np.float32, O_TEXTBOOK, inputs, heading=False)
    assert codes == [0] * STEPS, codes
    Xh, Ph, _ = _run_oracle(w, np.float64, O_TEXTBOOK, inputs, heading=False)
    got = (runs["1"][cid + "/X"], runs["1"][cid + "/P"], float(runs["1"][cid + "/trace"][0]))
    print(f"{cid}: max |X - oracle| = {float(np.abs(got[0] - Xo).max()):.3e}, max |P - oracle| = {float(np.abs(got[1] - Po).max()):.3e}")
    _compare("mirror " + cid, got, (Xo, Po), (Xh, Ph), 1e-5, 1e-4, 1e-4)


@pytest.mark.parametrize("N", SHAPES)
def test_buffers_rewritten_after_waiting_for_the_handles_streams_only(runs, N):
    """The lifetime rule of cslam_ekf_update_device with the mirror on: after the handle's streams (fetched once) have
    been synchronised the caller rewrites its one buffer pair, with no device-wide wait.  Under the held wide launch b's
    caller buffers are read by the blocks kernel only, which keeps the copies for the chain kernel and the wide kernel:
    bitwise the host-pointer filter and the CSLAM_LA_MIRROR=0 run."""
    cid, host = f"streams-N{N}", f"streams_host-N{N}"
    _same(runs, cid)
    _same(runs, cid, other=host, other_mirror="1")
    _same(runs, cid, other=host)
    assert int(runs["1"][cid + "/counts"][0]) == WINDOWS
    assert int(runs["1"][cid + "/counts"][1]) == 0
    assert int(runs["1"][cid + "/counts"][3]) == 1, "stage kernel launches"


if __name__ == "__main__":
    _child_main(sys.argv[1])
