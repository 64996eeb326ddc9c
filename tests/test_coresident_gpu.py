"""Several filters alive in one process: cslam_ekf_run_many, and the look-ahead windows' several-engines schedule
(cslam_ekf.hip: g_engines; la_eligible, the `safe` form of la_launch_window, the ev_fb wait of la_launch_held_wide).

The behaviour under test depends on the exact number of live engines (single handles and batched handles share one
counter, cslam_common.hpp: live_engines), so every side of every comparison runs in a fresh child process (this file, run
as a script: `<group> <role> <out.npz>`), closes every handle explicitly and leaves its results in an .npz file; the tests
below only compare files.  A child runs the cases of its group one after another, each from zero live engines.

  A  run_many on three handles of different size against the same three filters run alone through plain calls: bitwise
     on get_state() and trace(), equal lookahead_windows(); one instance per row against the oracle.
  B  CSLAM_LOOKAHEAD=1: a filter alone (in-kernel hand-overs, held wide launches) against the same filter beside an idle
     EKF / an idle EKFBatch (stream events only): bitwise, with the stage-kernel counts la_enqueue implies.
  C  a second handle appears, works and goes away between the calls of a filter that forms windows: bitwise the
     undisturbed filter, with the same counts.
  D  the automatic rule (f32, n >= 7000) at n = 7001: alone, beside a second handle, and a second handle that appears
     while an update is queued.
  E  run_many's argument errors, its no-ops, count == 1, and an out-of-range device index in one instance.

Every case reads factor_status() of every handle: 0, except the instance with the bad index (CSLAM_FACTOR_BAD_IDF).  A
raised CSLAM_FACTOR_INTERNAL (an in-kernel wait that ran into its 0.2 s time-out) fails wherever it appears.

What bites deterministically are the counts: a batched handle that did not count as an engine fails every EKFBatch row of
B (stage launches 1 instead of 4).  The two event edges (ev_raw in front of the safe chain launch, ev_fb in front of a
wide launch held from before) stand in front of in-kernel waits that remain -- the chain kernel reads the blocks
kernel's counters, the wide kernel polls the chain's completion word -- so a run without either edge computes the same
values; its failure mode is a kernel spinning at the head of a hardware queue, which these cases would report as
CSLAM_FACTOR_INTERNAL and did not in the one run made without each edge.

run_many has no per-instance host-side error that leaves the device alone: with device-resident inputs update() checks
only what the instances share (m, R, null pointers -- run_many refuses those up front for every instance), and everything
else it can return is a HIP status.  So the "run_many: instance i: ..." message carried back from a worker thread has no
test here.

f32, TEXTBOOK, sync_mode=False, set_deferred(128) unless stated; device-resident inputs in buffers of their own that stay
alive and are never rewritten.  N = 63 / 64 / 317 landmarks (n = 129: one row past the 128-row tile; 131; 637: a last
row block of 29), m = 9 (general wide kernel), 20, 32 (the k = 64 form); the last landmark and the one that straddles row
128 are always observed.
"""
import hashlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from helpers import OracleState, P_RTOL, X_RTOL, assert_close, make_obs, make_scenario  # noqa: E402

pytestmark = pytest.mark.gpu

TEXTBOOK = 0
F32, F64 = np.float32, np.float64
ERR_BAD_ARG, FACTOR_BAD_IDF, FACTOR_INTERNAL = 1, 8, 16
R0 = np.diag([0.08, 0.0024])
Q0 = np.diag([0.18, 6e-4])
WB, DT = 73.0, 0.01

# group -> (environment of its children, roles, time limit of one child in seconds)
GROUPS = {
    "default": ({}, ("ref", "alt"), 120),
    "la": ({"CSLAM_LOOKAHEAD": "1"}, ("ref", "alt", "alt2"), 180),
    "pipeline": ({"CSLAM_PIPELINE": "1"}, ("ref", "alt"), 120),
    "full": ({"CSLAM_STORAGE": "full"}, ("ref", "alt"), 120),
    "auto": ({}, ("ref", "alt", "alt2"), 180),
}

# A: id -> (group, dtype, landmarks per handle, m, lengths of the run_many calls, P-GEMM workgroup cap)
A_CASES = {
    "A-default": ("default", F32, (63, 64, 317), 32, (4, 2), 0),
    "A-wg3": ("default", F32, (63, 64, 317), 32, (4, 2), 3),
    "A-la-m32": ("la", F32, (63, 64, 317), 32, (4, 2), 0),
    "A-la-m9": ("la", F32, (63, 64, 317), 9, (4, 2), 0),
    "A-la-m20": ("la", F32, (63, 64, 317), 20, (4, 2), 0),
    "A-la-odd": ("la", F32, (63, 64, 317), 32, (4, 3), 0),  # the last call is odd: a window of one, drained by the flush
    "A-la-f64": ("la", F64, (63, 317), 32, (4, 2), 0),
    "A-la-wg3": ("la", F32, (63, 64, 317), 32, (4, 2), 3),
    "A-pipeline": ("pipeline", F32, (63, 64, 317), 32, (4, 2), 0),
    "A-full": ("full", F32, (63, 64, 317), 32, (4, 2), 0),
}
# look-ahead windows per handle (pairs of updates, and the drained last one of an odd run); no windows form by
# themselves at these sizes, and a two-stream (CSLAM_PIPELINE) engine takes none
A_WINDOWS = {"A-default": 0, "A-wg3": 0, "A-la-m32": 3, "A-la-m9": 3, "A-la-m20": 3, "A-la-odd": 4, "A-la-f64": 3,
             "A-la-wg3": 3, "A-pipeline": 0, "A-full": 0}

B_SHAPES = [(N, m) for N in (63, 64, 317) for m in (9, 20, 32)]
B_UPDATES = 8
B_ROLES = {"ref": None, "alt": "ekf", "alt2": "batch"}  # what is alive beside the filter

C_SHAPES = [(317, 32), (63, 9)]
C_UPDATES = 12
C_ENTRIES = ["landmarks", "score", "associate_deferred", "flush"]


def _c_schedules():
    """name -> ops of the disturbed side; the undisturbed side drops open / close / visit"""
    u = ["u"]
    s = {
        "even": u * 4 + ["open"] + u * 8,                      # a wide launch is held: the next call submits it behind ev_fb
        "odd": u * 5 + ["open"] + u * 7,                       # one update is queued: its window launches in the safe form
        "even_back": u * 4 + ["open"] + u * 2 + ["close"] + u * 6,  # ... and back to in-kernel hand-overs and the hold
        "odd_back": u * 5 + ["open"] + u * 2 + ["close"] + u * 5,
        "visit_even": u * 6 + ["visit"] + u * 6,               # created, one predict + update of its own, closed
        "visit_odd": u * 7 + ["visit"] + u * 5,
    }
    for e in C_ENTRIES:
        s[f"{e}_even"] = u * 4 + ["open", "entry:" + e] + u * 8
        s[f"{e}_odd"] = u * 5 + ["open", "entry:" + e] + u * 7
    return s


C_SCHEDULES = _c_schedules()

D_N, D_M, D_UPDATES = 3499, 32, 4  # n = 7001: the smallest size the automatic rule applies to
D_ROLES = {"ref": "alone", "alt": "beside", "alt2": "mixed"}
D_WINDOWS = {"alone": 2, "beside": 0, "mixed": 2}  # mixed: the window of two, and the queued update drained alone

E_NS, E_M, E_STEPS = (63, 64, 317), 20, 4
E_BAD = 1  # the instance of E-badidf that gets the out-of-range index


def _sid(N, m):
    return f"N{N}-m{m}"


def _pick(N, m, rng):
    """m distinct landmarks: the last one and the tile-straddling one (63) always among them"""
    special = list(dict.fromkeys(f for f in (N, 63) if f <= N))
    rest = [int(f) for f in rng.permutation(N) + 1 if f not in special]
    idf = np.array(special + rest[: m - len(special)], dtype=np.int32)
    return idf[rng.permutation(m)]


def _inputs(N, m, steps, dtype=F32, seed=1):
    X0, P0 = make_scenario(N, dtype, seed=500 + N, corr=0.1, pose_scale=1e-4)
    rng = np.random.default_rng(1000 * seed + 10 * N + m)
    idfs = [_pick(N, m, rng) for _ in range(steps)]
    obs = [make_obs(X0, idf, dtype, seed=97 * seed + t) for t, idf in enumerate(idfs)]
    return X0, P0, idfs, obs


def _ctrl(t):
    return 83.33, 0.01 * (t % 5)


def la_counts(ops):
    """(lookahead_windows, stage_launches) of an f32 filter under CSLAM_LOOKAHEAD=1 whose every update is device-resident
    and eligible -- la_enqueue / la_launch_window / la_drain of cslam_ekf.hip reduced to what they count.  The first update
    of a window is snapshotted by the held wide launch of the window before it when there is one, else by
    ekf_stage_obs_kernel (counted); a window's wide launch is held when the window was completed by its second update
    while this engine was the only one alive; every other entry point drains: a queued update becomes a window of one
    (never held), a held launch is submitted."""
    engines, queued, held, windows, stage = 1, 0, False, 0, 0
    for op in list(ops) + ["end"]:
        if op == "open":
            engines += 1
        elif op == "close":
            engines -= 1
        elif op == "visit":
            pass  # (gone again before the filter's next call)
        elif op == "u":
            if queued == 0:
                stage += 0 if held else 1
                held = False
            queued += 1
            if queued == 2:
                queued, windows, held = 0, windows + 1, engines == 1
        else:  # an entry point that drains; "end": the flush of the result
            windows += queued
            queued, held = 0, False
    return windows, stage


# ------------------------------------------------------------------------------------------------ the child's side
class _Filter:
    """One handle and its inputs on the device: one step-major buffer pair, written once."""

    def __init__(self, N, m, steps, dtype=F32, seed=1, wg=0, bad=None):
        import torch

        from conan_slam_amd import EKF

        self.N, self.m, self.dtype, self.t = N, m, np.dtype(dtype), 0
        self.X0, P0, self.idfs, self.obs = _inputs(N, m, steps, dtype, seed)
        self.e = EKF(N + 2, dtype=dtype, quirks=TEXTBOOK, sync_mode=False)
        self.e.set_state(self.X0, P0)
        self.e.set_deferred(128)
        if wg:
            self.e.set_pgemm_workgroups(wg)
        idf = np.concatenate(self.idfs).astype(np.int32)
        if bad is not None:
            idf[bad] = N + 7  # (every kernel clamps the index before it forms an address: ekf_kernels.hpp clamp_idf)
        z = np.concatenate([np.ascontiguousarray(o.reshape(-1, order="F")) for o in self.obs])
        self.dZ, self.dI = torch.from_numpy(z).cuda(), torch.from_numpy(idf).cuda()
        torch.cuda.synchronize()
        self.Q, self.R = Q0.astype(dtype), R0.astype(dtype)

    def zptr(self, t):
        return self.dZ.data_ptr() + t * 2 * self.m * self.dtype.itemsize

    def iptr(self, t):
        return self.dI.data_ptr() + t * self.m * 4

    def step(self):
        self.e.predict(*_ctrl(self.t), self.Q, WB, DT)
        self.e.update_device(self.zptr(self.t), self.m, self.R, self.iptr(self.t), batch=True)
        self.t += 1

    def result(self):
        e = self.e
        e.flush()
        X, P = e.get_state()
        return {"X": X, "P": P, "trace": e.trace(), "windows": e.lookahead_windows(), "stage": e.stage_launches(),
                "status": e.factor_status()}

    def close(self):
        self.e.close()


def _run_many(filters, t0, steps):
    from conan_slam_amd import run_many

    f0 = filters[0]
    ctrl = [_ctrl(t) for t in range(t0, t0 + steps)]
    run_many([f.e for f in filters], steps, [c[0] for c in ctrl], [c[1] for c in ctrl], f0.Q, WB, DT,
             [f.zptr(t0) for f in filters], [f.iptr(t0) for f in filters], f0.m, f0.R, batch=True)
    for f in filters:
        f.t = t0 + steps


def _case_a(role, cid):
    _, dtype, Ns, m, calls, wg = A_CASES[cid]
    steps, out = sum(calls), {}
    if role == "ref":  # each in turn as the only live handle, plain calls
        for i, N in enumerate(Ns):
            f = _Filter(N, m, steps, dtype, wg=wg)
            for _ in range(steps):
                f.step()
            out[str(i)] = f.result()
            f.close()
        return out
    fs = [_Filter(N, m, steps, dtype, wg=wg) for N in Ns]
    t0 = 0
    for c in calls:
        _run_many(fs, t0, c)
        t0 += c
    for i, f in enumerate(fs):
        out[str(i)] = f.result()
    for f in fs:
        f.close()
    return out


def _companion(kind):
    """a small idle handle beside the filter; -> (handle, its factor flags as one word)"""
    from conan_slam_amd import EKF, EKFBatch

    if kind == "batch":
        b = EKFBatch(2, 40, quirks=TEXTBOOK)
        return b, lambda: int(np.bitwise_or.reduce(np.array(b.factor_status(), dtype=np.int64)))
    e = EKF(10, dtype=F32, quirks=TEXTBOOK, sync_mode=False)
    return e, e.factor_status


def _case_b(role, N, m):
    beside = B_ROLES[role]
    comp, comp_status = _companion(beside) if beside else (None, lambda: 0)  # alive from before the filter's first call
    f = _Filter(N, m, B_UPDATES)
    for _ in range(B_UPDATES):
        f.step()
    r = f.result()
    r["status"] |= comp_status()
    f.close()
    if comp is not None:
        comp.close()
    return {"0": r}


def _visit():
    """a second handle that is created, does one predict + update of its own and is closed; -> its factor flags"""
    v = _Filter(20, 9, 1, seed=7)
    v.step()
    v.e.flush()  # (its one update is queued as the first of a window: the flush launches it)
    st = v.e.factor_status()
    v.close()
    return st


def _entry_call(f, entry):
    e = f.e
    if entry == "landmarks":
        return list(e.landmarks())
    if entry == "score":
        e.score(f.X0[:3].astype(np.float64), True)
        return []
    if entry == "associate_deferred":
        idf = _pick(f.N, f.m, np.random.default_rng(41))
        return list(e.associate_deferred(make_obs(f.X0, idf, F32, seed=41), f.R, 4.0, 25.0, with_counts=True))
    if entry == "flush":
        e.flush()
        return []
    raise ValueError(entry)


def _case_c(role, N, m, name):
    ops = C_SCHEDULES[name]
    f = _Filter(N, m, C_UPDATES)
    f.e.score_reset(4)
    f.e.score_set_truth(f.X0[3:].reshape(-1, 2))
    comp, comp_status, extra, ret = None, (lambda: 0), 0, []
    for op in ops:
        if op == "u":
            f.step()
        elif op.startswith("entry:"):
            ret += _entry_call(f, op[6:])
        elif role == "ref":
            continue  # the undisturbed side: alone throughout
        elif op == "open":
            comp, comp_status = _companion("ekf")
        elif op == "close":
            extra |= comp_status()
            comp.close()
            comp, comp_status = None, (lambda: 0)
        elif op == "visit":
            extra |= _visit()
    r = f.result()
    totals, series, track, _ = f.e.scores()
    r["ret"] = ret + [totals, series, track]
    r["status"] |= extra | comp_status()
    f.close()
    if comp is not None:
        comp.close()
    return {"0": r}


def _case_d(role):
    kind = D_ROLES[role]
    comp, comp_status = _companion("ekf") if kind == "beside" else (None, lambda: 0)
    f = _Filter(D_N, D_M, D_UPDATES)
    for t in range(D_UPDATES):
        if kind == "mixed" and t == D_UPDATES - 1:  # one window launched, update 3 queued: now the second handle appears
            comp, comp_status = _companion("ekf")
        f.step()
    r = f.result()
    r["status"] |= comp_status()
    f.close()
    if comp is not None:
        comp.close()
    return {"0": r}


def _error_of(fn):
    from conan_slam_amd import CslamError

    try:
        fn()
    except CslamError as ex:
        return ex.code, str(ex)
    return 0, ""


def _case_e(role, cid):
    from conan_slam_amd import run_many

    out = {}
    if cid in ("E-badidf", "E-badidf-la"):
        bad = {E_BAD: 1 * E_M + 3}  # (instance E_BAD, step 1, observation 3)
        if role == "ref":
            for i, N in enumerate(E_NS):
                f = _Filter(N, E_M, E_STEPS)
                for _ in range(E_STEPS):
                    f.step()
                out[str(i)] = f.result()
                f.close()
            return out
        fs = [_Filter(N, E_M, E_STEPS, bad=bad.get(i)) for i, N in enumerate(E_NS)]
        _run_many(fs, 0, E_STEPS)
        for i, f in enumerate(fs):
            out[str(i)] = f.result()
        for f in fs:
            f.close()
        return out
    N, m = 64, E_M
    if cid == "E-count1":  # one handle: on the calling thread
        f = _Filter(N, m, 6)
        if role == "ref":
            for _ in range(6):
                f.step()
        else:
            _run_many([f], 0, 4)
            _run_many([f], 4, 2)
    elif cid == "E-noop":  # count == 0 and steps == 0 between real steps
        f = _Filter(N, m, 4)
        for _ in range(2):
            f.step()
        if role == "alt":
            ctrl = [_ctrl(t) for t in range(2, 4)]
            run_many([], 2, [c[0] for c in ctrl], [c[1] for c in ctrl], f.Q, WB, DT, [], [], m, f.R)
            run_many([f.e], 0, [], [], f.Q, WB, DT, [f.zptr(2)], [f.iptr(2)], m, f.R)
        for _ in range(2):
            f.step()
    elif cid == "E-null":  # refused before any instance starts: the filters stay as they were set
        f, g = _Filter(N, m, 2), _Filter(63, m, 2)
        msgs = {}
        if role == "alt":
            v, s = [_ctrl(0)[0], _ctrl(1)[0]], [_ctrl(0)[1], _ctrl(1)[1]]
            msgs["handle"] = _error_of(lambda: run_many([f.e, None], 2, v, s, f.Q, WB, DT, [f.zptr(0), g.zptr(0)],
                                                        [f.iptr(0), g.iptr(0)], m, f.R))
            msgs["dz"] = _error_of(lambda: run_many([f.e, g.e], 2, v, s, f.Q, WB, DT, [f.zptr(0), None],
                                                    [f.iptr(0), g.iptr(0)], m, f.R))
        out["1"] = g.result()
        g.close()
        out["0"] = f.result()
        for k, (code, msg) in msgs.items():
            out["0"]["err_" + k] = np.array([code], dtype=np.int64)
            out["0"]["msg_" + k] = np.frombuffer(msg.encode(), np.uint8)
        f.close()
        return out
    else:
        raise ValueError(cid)
    out["0"] = f.result()
    f.close()
    return out


E_CASES = {"E-count1": "default", "E-noop": "default", "E-null": "default", "E-badidf": "default", "E-badidf-la": "la"}


def _all_cases():
    """(id, group, roles, function, arguments)"""
    out = [(cid, c[0], ("ref", "alt"), _case_a, (cid,)) for cid, c in A_CASES.items()]
    for N, m in B_SHAPES:
        out.append((f"B-{_sid(N, m)}", "la", ("ref", "alt", "alt2"), _case_b, (N, m)))
    for N, m in C_SHAPES:
        out += [(f"C-{name}-{_sid(N, m)}", "la", ("ref", "alt"), _case_c, (N, m, name)) for name in C_SCHEDULES]
    out.append(("D", "auto", ("ref", "alt", "alt2"), _case_d, ()))
    out += [(cid, g, ("ref", "alt"), _case_e, (cid,)) for cid, g in E_CASES.items()]
    return out


def _sha(arrays):
    return np.frombuffer(hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).digest(), np.uint8)


def _child_main(group, role, path):
    res = {}
    for cid, g, roles, fn, args in _all_cases():
        if g != group or role not in roles:
            continue
        for inst, r in fn(role, *args).items():
            key = f"{cid}/{inst}/"
            res[key + "X"] = r["X"]
            res[key + "Psha"] = _sha([r["P"]])
            res[key + "trace"] = np.array([r["trace"]], dtype=np.float64)
            res[key + "counts"] = np.array([r["windows"], r["stage"], r["status"]], dtype=np.int64)
            if cid[0] in "AD":
                res[key + "P"] = r["P"]
            if "ret" in r:
                res[key + "ret"] = _sha(r["ret"])
                res[key + "retlen"] = np.array([sum(np.asarray(a).nbytes for a in r["ret"])], dtype=np.int64)
            for k, v in r.items():
                if k.startswith(("err_", "msg_")):
                    res[key + k] = v
    np.savez(path, **res)


# ------------------------------------------------------------------------------------------------ the tests' side
def _run_child(group, role, path):
    extra, _, limit = GROUPS[group]
    env = {k: v for k, v in os.environ.items() if not k.startswith("CSLAM_") or k == "CSLAM_HIP_RUNTIME"}
    env.update(extra)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), group, role, path], env=env, capture_output=True,
                       text=True, timeout=limit)
    print(f"child ({group}, {role}): {time.perf_counter() - t0:.1f} s")
    assert r.returncode == 0, f"child ({group}, {role}) ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _group(name, factory):
    d = factory.mktemp("coresident_" + name)
    return {role: _run_child(name, role, str(d / f"{role}.npz")) for role in GROUPS[name][1]}  # one after another


@pytest.fixture(scope="module")
def runs_default(gpu_required, tmp_path_factory):
    return _group("default", tmp_path_factory)


@pytest.fixture(scope="module")
def runs_la(gpu_required, tmp_path_factory):
    return _group("la", tmp_path_factory)


@pytest.fixture(scope="module")
def runs_pipeline(gpu_required, tmp_path_factory):
    return _group("pipeline", tmp_path_factory)


@pytest.fixture(scope="module")
def runs_full(gpu_required, tmp_path_factory):
    return _group("full", tmp_path_factory)


@pytest.fixture(scope="module")
def runs_auto(gpu_required, tmp_path_factory):
    return _group("auto", tmp_path_factory)


def _status(run, key):
    return int(run[key + "counts"][2])


def _same(runs, cid, inst="0", a="alt", b="ref", status=0):
    """bitwise: X, P and trace(P) of one instance on side a against side b; equal window counts; both sides' flags"""
    ka = kb = f"{cid}/{inst}/"
    A, B = runs[a], runs[b]
    dx = float(np.abs(A[ka + "X"].astype(np.float64) - B[kb + "X"].astype(np.float64)).max())
    print(f"{cid}[{inst}] {a} vs {b}: max |dX| = {dx:.3e}, trace {A[ka + 'trace'][0]!r} / {B[kb + 'trace'][0]!r}, "
          f"(windows, stage launches, flags) {A[ka + 'counts'].tolist()} / {B[kb + 'counts'].tolist()}")
    assert _status(A, ka) == status and _status(B, kb) == 0, "factor_status"
    assert A[ka + "counts"][0] == B[kb + "counts"][0], "lookahead_windows differ"
    assert np.array_equal(A[ka + "X"], B[kb + "X"]), f"X differs: max |dX| = {dx:.3e}"
    assert np.array_equal(A[ka + "Psha"], B[kb + "Psha"]), "P differs"
    assert A[ka + "trace"][0] == B[kb + "trace"][0], "trace differs"


def _oracle(N, m, steps, dtype, fast=False):
    """the plain sequence on the CPU at the filter's precision, and in f64 for the fairness rule (fast: the oracle's
    blocked restatement of the same batch update, slam_oracle_fast.c -- at n = 7001 the plain loops take 15 s an update)"""
    X0, P0, idfs, obs = _inputs(N, m, steps, dtype)
    orc = OracleState(X0, P0, dtype, TEXTBOOK, extra=2)
    hi = OracleState(X0.astype(F64), P0.astype(F64), F64, TEXTBOOK, extra=2)
    for t in range(steps):
        v, swa = _ctrl(t)
        orc.predict(v, swa, Q0.astype(dtype), WB, DT)
        hi.predict(v, swa, Q0, WB, DT)
        assert orc.update(obs[t], R0.astype(dtype), idfs[t], True, fast=fast) == 0
        assert hi.update(obs[t].astype(F64), R0, idfs[t], True, fast=fast) == 0
    return orc, hi


def _close_to_oracle(name, run, key, orc, hi, dtype):
    X, P = run[key + "X"], run[key + "P"]
    print(f"{name}: max |X - oracle| = {float(np.abs(X - orc.x()).max()):.3e}, "
          f"max |P - oracle| = {float(np.abs(P - orc.p()).max()):.3e}")
    assert_close(name + " X", X, orc.x(), X_RTOL[np.dtype(dtype)], hi.x())
    assert_close(name + " P", P, orc.p(), P_RTOL[np.dtype(dtype)], hi.p())


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("cid", list(A_CASES))
def test_run_many_equals_the_handles_run_alone(request, cid):
    """Handles of different size in one run_many call (6 steps as calls of 4 and 2; 7 as 4 and 3 in the odd row) against
    the same filters, each alone in its process' turn, through predict / update_device: bitwise per instance, equal
    window counts, flags 0, the results pairwise different, and one instance against the oracle (f64 as fairness
    reference) so that a fault common to both sides still shows."""
    group, dtype, Ns, m, calls, _ = A_CASES[cid]
    runs = request.getfixturevalue("runs_" + group)
    for i in range(len(Ns)):
        _same(runs, cid, str(i))
        assert int(runs["alt"][f"{cid}/{i}/counts"][0]) == A_WINDOWS[cid]
    lead = [runs["alt"][f"{cid}/{i}/X"][:129] for i in range(len(Ns))]  # (every handle has at least 129 states)
    for i in range(len(Ns)):
        for j in range(i + 1, len(Ns)):
            assert not np.array_equal(lead[i], lead[j]), f"instances {i} and {j} ended with the same state"
    i = list(A_CASES).index(cid) % len(Ns)
    orc, hi = _oracle(Ns[i], m, sum(calls), dtype)
    _close_to_oracle(f"{cid}[{i}]", runs["alt"], f"{cid}/{i}/", orc, hi, dtype)


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("beside,role", [("ekf", "alt"), ("batch", "alt2")])
@pytest.mark.parametrize("N,m", B_SHAPES, ids=[_sid(*s) for s in B_SHAPES])
def test_event_only_windows_equal_the_fast_form(runs_la, N, m, beside, role):
    """8 device-resident updates under CSLAM_LOOKAHEAD=1, alone and beside an idle second handle (a single handle; a
    batched handle, which counts as well): bitwise, 4 windows each.  Alone, every window's wide launch is held and
    carries the next window's snapshot: the stage kernel ran once.  Beside a second engine no launch is held, so it
    ran once per window."""
    cid = f"B-{_sid(N, m)}"
    _same(runs_la, cid, a=role)
    ops = ["u"] * B_UPDATES
    alone, shared = la_counts(ops), la_counts(["open"] + ops)
    assert alone == (4, 1) and shared == (4, 4)
    assert tuple(runs_la["ref"][cid + "/0/counts"][:2]) == alone, "alone"
    assert tuple(runs_la[role][cid + "/0/counts"][:2]) == shared, f"beside an idle {beside} handle"


# ---------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("name", list(C_SCHEDULES))
@pytest.mark.parametrize("N,m", C_SHAPES, ids=[_sid(*s) for s in C_SHAPES])
def test_a_second_engine_comes_and_goes_between_calls(runs_la, N, m, name):
    """12 updates under CSLAM_LOOKAHEAD=1 with a second handle created / closed at the scheduled points, against the
    same calls alone: bitwise (state, and whatever the entry points returned), flags 0 on every handle, and the window and
    stage-kernel counts that la_enqueue implies on either side."""
    cid = f"C-{name}-{_sid(N, m)}"
    _same(runs_la, cid)
    ops = C_SCHEDULES[name]
    for role, o in (("alt", ops), ("ref", [x for x in ops if x not in ("open", "close", "visit")])):
        got = tuple(int(c) for c in runs_la[role][cid + "/0/counts"][:2])
        assert got == la_counts(o), f"{role}: (windows, stage launches) {got}, expected {la_counts(o)}"
    assert int(runs_la["alt"][cid + "/0/retlen"][0]) > 0
    assert np.array_equal(runs_la["alt"][cid + "/0/retlen"], runs_la["ref"][cid + "/0/retlen"])
    assert np.array_equal(runs_la["alt"][cid + "/0/ret"], runs_la["ref"][cid + "/0/ret"]), "what the entry points returned differs"


def test_la_counts_model():
    """the counts the cases above expect, spelled out for the plain schedules (no GPU needed for this one's content)"""
    u = ["u"]
    assert la_counts(u * 12) == (6, 1)
    assert la_counts(C_SCHEDULES["even"]) == (6, 4)        # update 5 rides in the held launch; 7, 9, 11 are staged
    assert la_counts(C_SCHEDULES["odd"]) == (6, 4)         # update 5 rode in the held launch before the handle appeared
    assert la_counts(C_SCHEDULES["even_back"]) == (6, 2)   # only update 7 follows a window that was not held
    assert la_counts(C_SCHEDULES["odd_back"]) == (6, 2)
    assert la_counts(C_SCHEDULES["visit_odd"]) == (6, 1)
    assert la_counts(C_SCHEDULES["flush_odd"]) == (7, 5)   # 2 windows, the drained one, 3 more, the last one drained
    assert la_counts(u * 5 + ["entry:flush"] + u * 7) == (7, 2)


# ---------------------------------------------------------------------------------------------------------------- D
@pytest.fixture(scope="module")
def oracle_d():
    t0 = time.perf_counter()
    o = _oracle(D_N, D_M, D_UPDATES, F32, fast=True)
    print(f"D: oracle in f32 and f64, {time.perf_counter() - t0:.1f} s")
    return o


@pytest.mark.parametrize("role", list(D_ROLES), ids=list(D_ROLES.values()))
def test_automatic_windows_only_while_alone(runs_auto, oracle_d, role):
    """n = 7001, f32, CSLAM_LOOKAHEAD unset, 4 updates: alone 2 windows; a second handle alive from the start: none; a
    second handle that appears while update 3 is queued: the window of two, then update 3 drained as a window of one
    and update 4 on the classic path.  All three against the oracle over the whole state.  (The longest case of the
    file: the three children and the oracle's four updates in f32 and f64, computed once, take 16 s together.)"""
    key = "D/0/"
    run = runs_auto[role]
    print(f"D {D_ROLES[role]}: (windows, stage launches, flags) {run[key + 'counts'].tolist()}")
    assert _status(run, key) == 0
    assert int(run[key + "counts"][0]) == D_WINDOWS[D_ROLES[role]]
    _close_to_oracle("D " + D_ROLES[role], run, key, *oracle_d, F32)


# ---------------------------------------------------------------------------------------------------------------- E
def test_run_many_refuses_null_handles_and_inputs(runs_default):
    alt = runs_default["alt"]
    assert int(alt["E-null/0/err_handle"][0]) == ERR_BAD_ARG
    assert int(alt["E-null/0/err_dz"][0]) == ERR_BAD_ARG
    msg = bytes(alt["E-null/0/msg_dz"]).decode()
    assert "run_many" in msg and "instance 1" in msg, msg
    assert "instance 1" in bytes(alt["E-null/0/msg_handle"]).decode()
    for inst in ("0", "1"):  # nothing ran on either handle
        _same(runs_default, "E-null", inst)


def test_run_many_without_instances_or_steps_changes_nothing(runs_default):
    _same(runs_default, "E-noop")


def test_run_many_of_one_handle_equals_plain_calls(runs_default):
    _same(runs_default, "E-count1")


@pytest.mark.parametrize("cid", ["E-badidf", "E-badidf-la"])
def test_run_many_flags_a_bad_feature_index_in_its_instance_only(request, cid):
    """One instance's device-resident index list holds an out-of-range entry: that handle raises CSLAM_FACTOR_BAD_IDF, the
    others stay at 0 and bitwise equal to their solo runs."""
    runs = request.getfixturevalue("runs_" + E_CASES[cid])
    for i in range(len(E_NS)):
        if i != E_BAD:
            _same(runs, cid, str(i))
    st = _status(runs["alt"], f"{cid}/{E_BAD}/")
    assert st & FACTOR_BAD_IDF and not st & FACTOR_INTERNAL, st
    assert _status(runs["ref"], f"{cid}/{E_BAD}/") == 0


if __name__ == "__main__":
    _child_main(*sys.argv[1:4])
