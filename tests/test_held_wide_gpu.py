"""Look-ahead windows whose wide launch is held until the next call (cslam_ekf.hip: la_launch_held_wide) and carries the
snapshot of the next window's first update (LaSnapJob).

Every comparison is bitwise, on get_state() and lookahead_windows(): the other side is the SAME call sequence with
CSLAM_LA_HOLD_WIDE=0, which launches every wide kernel in the call that completes its window and snapshots every queued
device-resident update with ekf_stage_obs_kernel.  Each side runs in a fresh child process of its own (this file, run as a
script: every case in turn, one handle alive at a time, so that the single-engine schedule is the one under test) and
leaves its results in an .npz file; the tests below compare the two files.  One case per shape is also compared with the
oracle and f64, with the tolerance of test_ekf_gpu.py::test_lookahead_windows_match_the_oracle, so that a fault common to
both launch orders still shows.

Shapes: N = 62, 63, 64 landmarks (n = 127, 129, 131: around the 128-row tile edge; landmark 63 straddles it) and N = 317
(n = 637: several blocks of rows, a last block of 29), m = 9 (the general wide kernel) and m = 32 (the k = 64 form); f32,
TEXTBOOK, a deferral window of 128 columns, CSLAM_LOOKAHEAD=1.
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

from helpers import OracleState, P_RTOL, X_RTOL, assert_close, make_obs, make_scenario  # noqa: E402

pytestmark = pytest.mark.gpu

TEXTBOOK = 0
F32 = np.float32
SHAPES = [(N, m) for N in (62, 63, 64, 317) for m in (9, 32)]
ENTRIES = ["get_x", "get_state", "landmarks", "trace", "flush", "synchronize", "augment", "observe_heading",
           "set_deferred", "set_state", "sequential", "m4", "host_update", "predict", "close"]
ORACLE_ENTRY = "host_update"  # (device- and host-staged updates, a window of one at the end)
WRAP_SHAPE, WRAP_UPDATES = (62, 9), 260  # 130 windows: the 64 slots of the staging ring come round twice
R = np.diag([0.08, 0.0024]).astype(F32)
Q = np.diag([0.18, 6e-4]).astype(F32)
ZN = np.array([[280.0], [-0.3]], dtype=F32)
PHI = 0.3004  # (the scenario's heading is 0.3)


def _sid(N, m):
    return f"N{N}-m{m}"


def _pick(N, m, rng):
    """m distinct landmarks: the last one and the tile-straddling one (63) always among them"""
    special = [f for f in (N, 63) if f <= N]
    special = list(dict.fromkeys(special))
    rest = [int(f) for f in rng.permutation(N) + 1 if f not in special]
    idf = np.array(special + rest[: m - len(special)], dtype=np.int32)
    return idf[rng.permutation(m)]


def _inputs(N, m, steps, seed):
    X0, P0 = make_scenario(N, F32, seed=500 + N, corr=0.1, pose_scale=1e-4)
    rng = np.random.default_rng(1000 * seed + 10 * N + m)
    idfs = [_pick(N, m, rng) for _ in range(steps)]
    obs = [make_obs(X0, idf, F32, seed=97 * seed + t) for t, idf in enumerate(idfs)]
    return X0, P0, idfs, obs


def _ctrl(t):
    return 83.33, 0.01 * (t % 5)


def _extra_update(N, mm, seed):
    X0, _ = make_scenario(N, F32, seed=500 + N, corr=0.1, pose_scale=1e-4)
    idf = _pick(N, mm, np.random.default_rng(seed))
    return make_obs(X0, idf, F32, seed=seed), idf


# ------------------------------------------------------------------------------------------------ the child's side
class _Driver:
    """One handle and the three ways an update reaches it."""

    def __init__(self, N, X0, P0):
        import torch

        from conan_slam_amd import EKF

        self.torch = torch
        self.e = EKF(N + 2, dtype=F32, quirks=TEXTBOOK, sync_mode=False)
        self.e.set_state(X0, P0)
        self.e.set_deferred(128)
        self.keep = []
        self.dZ = torch.zeros(64, dtype=torch.float32, device="cuda")
        self.dI = torch.zeros(32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        # the handle's streams, fetched ONCE (cslam_ekf_get_streams), as a caller that orders its buffer reuse against them does
        self.ext = [torch.cuda.ExternalStream(p) for p in dict.fromkeys(self.e.streams()) if p]

    def step(self, t, Z, idf, mode):
        torch, e, m = self.torch, self.e, len(idf)
        e.predict(*_ctrl(t), Q, 73.0, 0.01)
        zf = np.ascontiguousarray(Z.reshape(-1, order="F"))
        if mode == "host":
            e.update(Z, R, idf, True)
        elif mode == "dev":  # buffers of its own, never rewritten
            dZ, dI = torch.from_numpy(zf).cuda(), torch.from_numpy(idf).cuda()
            torch.cuda.synchronize()
            self.keep += [dZ, dI]
            e.update_device(dZ.data_ptr(), m, R, dI.data_ptr(), batch=True)
        elif mode == "streams":
            # ONE buffer pair again, but the caller waits for the handle's two streams only (cslam.h: "until the handle's
            # streams have been synchronised") and then rewrites the buffers at once, device to device, on a stream of its
            # own.  Nothing here waits for the device as a whole: the engine's internal chain stream is not covered, so
            # no kernel on it may still be reading the caller's buffers once the handle's streams have drained.
            sZ, sI = torch.from_numpy(zf).cuda(), torch.from_numpy(idf).cuda()  # (staged copies: the rewrite is quick)
            self.keep += [sZ, sI]
            torch.cuda.current_stream().synchronize()
            for st in self.ext:  # everything the previous call enqueued on the handle's streams has run ...
                st.synchronize()
            self.dZ[: 2 * m].copy_(sZ)  # ... so its inputs may be overwritten
            self.dI[:m].copy_(sI)
            torch.cuda.current_stream().synchronize()  # (the caller's writes are complete when the call is made)
            e.update_device(self.dZ.data_ptr(), m, R, self.dI.data_ptr(), batch=True)
        else:  # "reuse": ONE buffer pair, rewritten before every call; only device-wide waits in between
            self.dZ[: 2 * m].copy_(torch.from_numpy(zf))
            self.dI[:m].copy_(torch.from_numpy(idf))
            torch.cuda.synchronize()
            e.update_device(self.dZ.data_ptr(), m, R, self.dI.data_ptr(), batch=True)
            torch.cuda.synchronize()

    def result(self):
        e = self.e
        e.flush()
        X, P = e.get_state()
        out = {"X": X, "P": P, "windows": e.lookahead_windows(), "stage": e.stage_launches(),
               "status": e.factor_status()}
        e.close()
        return out


def _entry_call(d, entry, N, m, t):
    """makes the call; returns what a read-only entry point returned (arrays), for the comparison of the two orders"""
    e = d.e
    if entry == "get_x":
        return [e.get_x()]
    elif entry == "get_state":
        return list(e.get_state())
    elif entry == "landmarks":
        return list(e.landmarks())
    elif entry == "trace":
        return [np.array([e.trace()], dtype=np.float64)]
    elif entry == "flush":
        e.flush()
    elif entry == "synchronize":
        e.synchronize()
    elif entry == "augment":
        e.augment(ZN, R)
    elif entry == "observe_heading":
        e.observe_heading(PHI, True)
    elif entry == "set_deferred":
        e.set_deferred(0)
        e.set_deferred(128)
    elif entry == "set_state":
        X1, P1 = make_scenario(N, F32, seed=700 + N, corr=0.1, pose_scale=1e-4)
        e.set_state(X1, P1)
    elif entry == "sequential":
        Z, idf = _extra_update(N, 5, 31)
        e.predict(*_ctrl(t), Q, 73.0, 0.01)
        e.update(Z, R, idf, False)
    elif entry == "m4":
        Z, idf = _extra_update(N, 4, 32)
        e.predict(*_ctrl(t), Q, 73.0, 0.01)
        e.update(Z, R, idf, True)
    elif entry == "host_update":
        Z, idf = _extra_update(N, m, 33)
        e.predict(*_ctrl(t), Q, 73.0, 0.01)
        e.update(Z, R, idf, True)
    elif entry == "predict":
        e.predict(*_ctrl(t), Q, 73.0, 0.01)
    else:
        raise ValueError(entry)
    return []


def _case_entry(N, m, entry):
    """two windows (a wide launch is held), the call, two more windows, flush"""
    X0, P0, idfs, obs = _inputs(N, m, 8, seed=1)
    d = _Driver(N, X0, P0)
    for t in range(4):
        d.step(t, obs[t], idfs[t], "dev")
    if entry == "close":
        wins = d.e.lookahead_windows()
        d.e.close()  # with the wide launch held: must return and free the handle ...
        d = _Driver(N, X0, P0)  # ... and a new handle must work
        for t in range(4, 6):
            d.step(t, obs[t], idfs[t], "dev")
        out = d.result()
        out["windows"] += 100 * wins
        return out
    ret = _entry_call(d, entry, N, m, 4)
    for t in range(4, 8):
        d.step(t, obs[t], idfs[t], "dev")
    out = d.result()
    out["ret"] = ret
    return out


def _case_modes(N, m, modes):
    X0, P0, idfs, obs = _inputs(N, m, len(modes), seed=2)
    d = _Driver(N, X0, P0)
    for t, mode in enumerate(modes):
        d.step(t, obs[t], idfs[t], mode)
    return d.result()


MODE_CASES = {
    "snapshot": ["reuse"] * 6,         # the carried copy: one buffer pair rewritten before every call
    "snapshot_host": ["host"] * 6,     # the same filter through host pointers
    "tail": ["reuse"] * 5,             # the last window has one update
    "tail_host": ["host"] * 5,
    "mixed_hd": ["host", "reuse"] * 3,  # first update host-staged, second device-resident
    "mixed_dh": ["reuse", "host"] * 3,  # and the reverse
    "streams": ["streams"] * 8,        # buffers rewritten after waiting for the handle's own streams only
    "streams_host": ["host"] * 8,
}


def _all_cases():
    out = []
    for N, m in SHAPES:
        out += [(f"entry-{e}-{_sid(N, m)}", _case_entry, (N, m, e)) for e in ENTRIES]
        out += [(f"{k}-{_sid(N, m)}", _case_modes, (N, m, v)) for k, v in MODE_CASES.items()]
    out.append((f"wrap-{_sid(*WRAP_SHAPE)}", _case_modes, (*WRAP_SHAPE, ["reuse"] * WRAP_UPDATES)))
    return out


def _child_main(path):
    res = {}
    for cid, fn, args in _all_cases():
        r = fn(*args)
        res[cid + "/X"] = r["X"]
        res[cid + "/Psha"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(r["P"]).tobytes()).digest(), np.uint8)
        res[cid + "/counts"] = np.array([r["windows"], r["stage"], r["status"]], dtype=np.int64)
        ret = b"".join(np.ascontiguousarray(a).tobytes() for a in r.get("ret", []))
        res[cid + "/ret"] = np.frombuffer(hashlib.sha256(ret).digest(), np.uint8)
        res[cid + "/retlen"] = np.array([len(ret)], dtype=np.int64)
        if cid.startswith(f"entry-{ORACLE_ENTRY}-"):
            res[cid + "/P"] = r["P"]
    np.savez(path, **res)


# ------------------------------------------------------------------------------------------------ the tests' side
def _run_child(path, hold):
    env = dict(os.environ)
    env["CSLAM_LOOKAHEAD"] = "1"
    env["CSLAM_LA_HOLD_WIDE"] = hold
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, f"child (CSLAM_LA_HOLD_WIDE={hold}) ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(gpu_required, tmp_path_factory):
    d = tmp_path_factory.mktemp("held_wide")
    return {hold: _run_child(str(d / f"hold{hold}.npz"), hold) for hold in ("1", "0")}


def _same(runs, cid, other=None, other_hold="0"):
    """bitwise: case cid with the wide launch held against case `other` (default: itself) under other_hold"""
    a, b, oid = runs["1"], runs[other_hold], other or cid
    dx = float(np.abs(a[cid + "/X"].astype(np.float64) - b[oid + "/X"].astype(np.float64)).max())
    print(f"{cid} vs {oid} (hold {other_hold}): max |dX| = {dx:.3e}, windows {a[cid + '/counts'][0]} / {b[oid + '/counts'][0]}")
    assert a[cid + "/counts"][0] == b[oid + "/counts"][0], "lookahead_windows differ"
    assert a[cid + "/counts"][2] == 0 and b[oid + "/counts"][2] == 0, "factor_status"
    assert np.array_equal(a[cid + "/X"], b[oid + "/X"]), f"X differs: max |dX| = {dx:.3e}"
    assert np.array_equal(a[cid + "/Psha"], b[oid + "/Psha"]), "P differs"


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("N,m", SHAPES, ids=[_sid(*s) for s in SHAPES])
def test_every_entry_point_meets_a_held_wide_launch(runs, N, m, entry):
    """Two windows, so that a wide launch is held; one call of another kind; two more windows; flush."""
    cid = f"entry-{entry}-{_sid(N, m)}"
    _same(runs, cid)
    wins = int(runs["1"][cid + "/counts"][0])
    if entry == "observe_heading":
        # (the heading column stays pending in the store, and a store with a heading column takes no window: how many
        # of the later updates pair up depends on when the deferral window flushes it -- the same in both launch orders)
        assert wins >= 2, wins
        return
    if entry in ("get_x", "get_state", "landmarks", "trace"):
        # what the call itself returned with the wide launch held: the state after the second window, bit for bit what
        # the other order returns (a read that did not submit the held launch first would miss that window)
        assert int(runs["1"][cid + "/retlen"][0]) > 0
        assert np.array_equal(runs["1"][cid + "/retlen"], runs["0"][cid + "/retlen"])
        assert np.array_equal(runs["1"][cid + "/ret"], runs["0"][cid + "/ret"]), "the value read while the wide launch was held differs"
    expected = {"close": 201, "host_update": 5}.get(entry, 4)
    # (close: 2 windows before it, 1 on the new handle; host_update: the extra update pairs up, the last one is drained alone)
    assert wins == expected, wins


@pytest.mark.parametrize("N,m", SHAPES, ids=[_sid(*s) for s in SHAPES])
def test_held_wide_sequence_matches_the_oracle(runs, N, m):
    """The oracle leg: the host_update case of every shape against the oracle's plain sequence and f64."""
    cid = f"entry-{ORACLE_ENTRY}-{_sid(N, m)}"
    X0, P0, idfs, obs = _inputs(N, m, 8, seed=1)
    Zx, ix = _extra_update(N, m, 33)
    seq = [(t, obs[t], idfs[t]) for t in range(4)] + [(4, Zx, ix)] + [(t, obs[t], idfs[t]) for t in range(4, 8)]
    orc = OracleState(X0, P0, F32, TEXTBOOK, extra=2)
    hi = OracleState(X0.astype(np.float64), P0.astype(np.float64), np.float64, TEXTBOOK, extra=2)
    for t, Z, idf in seq:
        v, swa = _ctrl(t)
        orc.predict(v, swa, Q, 73.0, 0.01)
        hi.predict(v, swa, Q.astype(np.float64), 73.0, 0.01)
        assert orc.update(Z, R, idf, True) == 0
        hi.update(Z.astype(np.float64), R.astype(np.float64), idf, True)
    X, P = runs["1"][cid + "/X"], runs["1"][cid + "/P"]
    dt = np.dtype(F32)
    print(f"{cid}: max |X - oracle| = {float(np.abs(X - orc.x()).max()):.3e}, max |P - oracle| = {float(np.abs(P - orc.p()).max()):.3e}")
    assert_close("held wide X", X, orc.x(), 4 * X_RTOL[dt], hi.x(), fair=8.0)
    assert_close("held wide P", P, orc.p(), 4 * P_RTOL[dt], hi.p(), fair=8.0)


@pytest.mark.parametrize("N,m", SHAPES, ids=[_sid(*s) for s in SHAPES])
def test_snapshot_rides_in_the_wide_kernel(runs, N, m):
    """Six update_device calls from ONE buffer pair that is rewritten before every call, device-wide waits only in between:
    bitwise the host-pointer filter and the CSLAM_LA_HOLD_WIDE=0 run, and ekf_stage_obs_kernel ran for the first window
    only (every later snapshot was carried by the previous window's wide kernel)."""
    cid, host = f"snapshot-{_sid(N, m)}", f"snapshot_host-{_sid(N, m)}"
    _same(runs, cid)
    _same(runs, cid, other=host, other_hold="1")
    _same(runs, cid, other=host)
    assert int(runs["1"][cid + "/counts"][0]) == 3
    assert int(runs["1"][cid + "/counts"][1]) == 1, "stage kernel launches with the wide launch held"
    assert int(runs["0"][cid + "/counts"][1]) == 3, "stage kernel launches with CSLAM_LA_HOLD_WIDE=0"
    assert int(runs["1"][host + "/counts"][1]) == 0


@pytest.mark.parametrize("case,stage_held", [("tail", 1), ("mixed_hd", 0), ("mixed_dh", 1)])
@pytest.mark.parametrize("N,m", SHAPES, ids=[_sid(*s) for s in SHAPES])
def test_odd_tail_and_mixed_staging(runs, N, m, case, stage_held):
    """Five updates then flush (the last window has one update); windows whose first update is host-staged and whose
    second is device-resident, and the reverse -- against CSLAM_LA_HOLD_WIDE=0 and against the all-host filter."""
    cid = f"{case}-{_sid(N, m)}"
    host = ("tail_host-" if case == "tail" else "snapshot_host-") + _sid(N, m)
    _same(runs, cid)
    _same(runs, cid, other=host)
    assert int(runs["1"][cid + "/counts"][0]) == 3
    assert int(runs["1"][cid + "/counts"][1]) == stage_held


@pytest.mark.parametrize("N,m", SHAPES, ids=[_sid(*s) for s in SHAPES])
def test_buffers_rewritten_after_waiting_for_the_handles_streams_only(runs, N, m):
    """The lifetime rule of cslam_ekf_update_device: after the handle's streams (fetched once) have been synchronised the
    caller rewrites its one buffer pair -- no device-wide wait, so the engine's internal chain stream is not covered.  With
    the wide launch held nothing on the main stream waits for the chain kernel within b's call, so the chain must not
    read b's caller buffers: bitwise the host-pointer filter and the CSLAM_LA_HOLD_WIDE=0 run.  (These shapes have a P-GEMM
    of a few microseconds, so the chain kernel outlives the main stream's work of its call by most of its run time.)"""
    cid, host = f"streams-{_sid(N, m)}", f"streams_host-{_sid(N, m)}"
    _same(runs, cid)
    _same(runs, cid, other=host, other_hold="1")
    _same(runs, cid, other=host)
    assert int(runs["1"][cid + "/counts"][0]) == 4
    assert int(runs["1"][cid + "/counts"][1]) == 1


def test_staging_ring_wraps_under_carried_snapshots(runs):
    """130 windows from one rewritten buffer pair: every slot of the 64-slot ring is rewritten twice by carried copies."""
    cid = f"wrap-{_sid(*WRAP_SHAPE)}"
    _same(runs, cid)
    assert int(runs["1"][cid + "/counts"][0]) == WRAP_UPDATES // 2
    assert int(runs["1"][cid + "/counts"][1]) == 1
    assert int(runs["0"][cid + "/counts"][1]) == WRAP_UPDATES // 2


if __name__ == "__main__":
    _child_main(sys.argv[1])
