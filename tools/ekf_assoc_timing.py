#!/usr/bin/env python3
"""Step rate of a single-handle filter that associates every step: cslam_ekf_associate (flushes the pending covariance
downdate, two copies back) against cslam_ekf_associate_deferred (reads the deferred form, leaves the split on the device),
and the known-association loop without any association as the floor.  set_deferred(128), default look-ahead, m
observations of mapped landmarks per step.

    (a) predict + associate          + update(batch) with the association's own host lists
    (b) predict + associate_deferred + update_device from association_device_ptrs()
    (c) predict + update_device with known correspondences (no association)
    (d) predict + associate_deferred_async + update_counted (the count mf read on the device) + association_wait:
        no host round trip between the association's resolve kernel and the update's gather kernel

    (e) predict + associate_update_augment: loop (d), then augment_device on the ZN the association left in HBM, with
        the count association_wait returned -- all new features of the scan in ONE launch
    (f) loop (d) + the host augment(Z[:, kind == 2]): one launch per new feature
Loops (e) and (f) run on a map with a hole around the vehicle: every scan holds --new observations (default 2) inside
the hole, on a fan of 12 bearings x 25 ranges whose neighbours lie beyond gate2 of each other, so each is a new feature;
the capacity is --landmarks, of which 300 slots are left free for them (at most 300 / --new steps in all).  --pair ef
alternates the two on the same scans with CSLAM_LOOKAHEAD=0 and with the default.
--calls times single calls instead: augment against augment_device at q = 1, 8, 32 on n ~ 10 000, with events on the
chain stream around 20 calls, alternated three times.

(a) and (b) -- with --pair bd: (b) and (d), with --pair ef: (e) and (f) -- are alternated --rounds times on fresh handles; every run is timed with events on the handle's chain stream
around --steps steps after --warmup steps, and ends in a synchronise.  Prints one JSON line per run and a summary line.
For the device time of ekf_assoc_pair_kernel run one loop under the profiler,
`rocprofv3 --kernel-trace --stats -- python tools/ekf_assoc_timing.py --only b --rounds 1`, and set it against
`pair_bytes`: the 2 nf kp panel scalars and 25 nf entries of P the kernel has to read.

    python tools/ekf_assoc_timing.py [--landmarks 5000] [--dtype f32] [--m 32] [--steps 200] [--warmup 20] [--rounds 5]
                                     [--pair ab|bd|ef] [--only a|b|c|d|e|f] [--new 2] [--calls]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from conan_slam_amd import EKF, Q_TEXTBOOK  # noqa: E402

GATES = (4.0, 25.0)


def _state(N, dtype, seed):
    rng = np.random.default_rng(seed)
    X = np.concatenate([[0.0, 0.0, 0.1], rng.uniform(-500, 500, 2 * N)]).astype(dtype)
    P = np.eye(3 + 2 * N, dtype=dtype, order="F")
    P[:3, :3] *= 1e-2
    return X, P


def _scans(X, N, m, steps, dtype, seed):
    """per step: (idf [m], Z [2, m]) -- noisy observations of m mapped landmarks from the (standing) true pose"""
    rng = np.random.default_rng(seed)
    out = []
    X = X.astype(np.float64)
    for _ in range(steps):
        idf = np.sort(rng.permutation(N)[:m] + 1).astype(np.int32)
        fx = 3 + 2 * (idf - 1)
        dx, dy = X[fx] - X[0], X[fx + 1] - X[1]
        Z = np.stack([np.hypot(dx, dy) + 0.1 * rng.normal(size=m), np.arctan2(dy, dx) - X[2] + 0.002 * rng.normal(size=m)])
        out.append((idf, np.asfortranarray(Z.astype(dtype))))
    return out


NEW_SLOTS, HOLE = 300, 130.0   # loops (e) / (f): free slots for new features; no mapped landmark this near the vehicle


def _state_with_hole(N, dtype, seed):
    """_state with the landmarks nearer than HOLE to the vehicle pushed out along their bearing"""
    X, P = _state(N, dtype, seed)
    xy = X[3:].astype(np.float64).reshape(N, 2)
    d = np.hypot(xy[:, 0], xy[:, 1])
    near = d < HOLE
    xy[near] *= ((HOLE + d[near]) / np.maximum(d[near], 1e-6))[:, None]
    X[3:] = xy.reshape(-1).astype(dtype)
    return X, P


def _new_columns(X, k0, count):
    """observations k0 .. k0 + count - 1 of the fan of new features: 12 bearings 0.52 rad apart x ranges 10, 14, ... 106 m"""
    k = k0 + np.arange(count)
    assert k.max() < NEW_SLOTS, "more new features than the fan holds: fewer steps or a smaller --new"
    return np.stack([10.0 + 4.0 * (k // 12), -3.0 + 0.52 * (k % 12) - float(X[2])])


def _env(lookahead):
    if lookahead is None:
        os.environ.pop("CSLAM_LOOKAHEAD", None)
    else:
        os.environ["CSLAM_LOOKAHEAD"] = str(lookahead)


def run(loop, N, dtype, m, steps, warmup, seed=1, new=2, lookahead=None):
    import torch

    Q = np.diag([0.18, 6e-4]).astype(dtype)
    R = np.diag([0.08, 0.0024]).astype(dtype)
    grows = loop in ("e", "f")
    if grows:
        N0 = N - NEW_SLOTS
        X, P = _state_with_hole(N0, dtype, 3)
        scans = [(idf, np.asfortranarray(np.concatenate([Z, _new_columns(X, t * new, new).astype(dtype)], axis=1)))
                 for t, (idf, Z) in enumerate(_scans(X, N0, m - new, warmup + steps, dtype, seed))]
    else:
        X, P = _state(N, dtype, 3)
        scans = _scans(X, N, m, warmup + steps, dtype, seed)
    _env(lookahead)
    e = EKF(N, dtype=dtype, quirks=Q_TEXTBOOK, sync_mode=False)
    _env(None)
    e.set_state(X, P)
    e.set_deferred(128)
    stream = torch.cuda.ExternalStream(e.streams()[0])
    dev = [(torch.from_numpy(np.ascontiguousarray(Z.reshape(-1, order="F"))).cuda(), torch.from_numpy(idf).cuda())
           for idf, Z in scans] if loop == "c" else None
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    associated = augmented = 0
    for t, (idf_true, Z) in enumerate(scans):
        if t == warmup:
            e.synchronize()
            t0.record(stream)
        e.predict(0.0, 0.0, Q, 73.0, 0.01)   # (the vehicle stands: the scans stay scans of the estimated map)
        if loop == "a":
            idf, kind = e.associate(Z, R, *GATES)
            sel = kind == 1
            e.update(np.asfortranarray(Z[:, sel]), R, idf[sel], True)
            associated += int(sel.sum()) if t >= warmup else 0
        elif loop == "b":
            idf, kind, counts = e.associate_deferred(Z, R, *GATES, with_counts=True)
            dZF, d_idf, _, _ = e.association_device_ptrs()
            e.update_device(dZF, int(counts[0]), R, d_idf, True)
            associated += int(counts[0]) if t >= warmup else 0
        elif loop == "d":
            idf, kind, counts = e.associate_update_counted(Z, R, *GATES)
            associated += int(counts[0]) if t >= warmup else 0
        elif loop == "e":
            idf, kind, counts = e.associate_update_augment(Z, R, *GATES)
            associated += int(counts[0]) if t >= warmup else 0
            augmented += int(counts[1]) if t >= warmup else 0
        elif loop == "f":
            idf, kind, counts = e.associate_update_counted(Z, R, *GATES)
            e.augment(np.asfortranarray(Z[:, kind == 2]), R)
            associated += int(counts[0]) if t >= warmup else 0
            augmented += int(counts[1]) if t >= warmup else 0
        else:
            dZ, dI = dev[t]
            e.update_device(dZ.data_ptr(), m, R, dI.data_ptr(), True)
            associated += m if t >= warmup else 0
    e.synchronize()
    t1.record(stream)
    t1.synchronize()
    ms = t0.elapsed_time(t1)
    trace = e.trace()
    out = {"loop": loop, "landmarks": N, "dtype": np.dtype(dtype).name, "m": m, "steps": steps, "ms": round(ms, 3),
           "steps_per_s": round(1e3 * steps / ms, 1), "associated": associated, "trace": trace}
    if grows:
        out.update({"lookahead": "default" if lookahead is None else lookahead, "new_per_scan": new, "augmented": augmented,
                    "augment_launches": e.augment_launches(), "n_end": e.n})
    e.close()
    return out


def time_calls(N0, dtype, q, device, reps=20):
    """ms per call of augment (device=False) or augment_device over `reps` calls of q new features from n = 3 + 2 N0"""
    import torch

    R = np.diag([0.08, 0.0024]).astype(dtype)
    X, P = _state(N0, dtype, 3)
    e = EKF(N0 + (reps + 1) * q, dtype=dtype, quirks=Q_TEXTBOOK, sync_mode=False)
    e.set_state(X, P)
    stream = torch.cuda.ExternalStream(e.streams()[0])
    rng = np.random.default_rng(q)
    Zs = [np.asfortranarray(np.stack([rng.uniform(5, 40, q), rng.uniform(-3, 3, q)]).astype(dtype)) for _ in range(reps + 1)]
    dZs = [torch.from_numpy(np.ascontiguousarray(Z.reshape(-1, order="F"))).cuda() for Z in Zs]
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i, (Z, dZ) in enumerate(zip(Zs, dZs)):
        if i == 1:   # (the first call is the warm-up)
            e.synchronize()
            t0.record(stream)
        if device:
            e.augment_device(dZ.data_ptr(), q, R)
        else:
            e.augment(Z, R)
    t1.record(stream)
    t1.synchronize()
    ms = t0.elapsed_time(t1) / reps
    out = {"call": "augment_device" if device else "augment", "q": q, "n_start": 3 + 2 * N0, "n_end": e.n, "reps": reps,
           "dtype": np.dtype(dtype).name, "ms_per_call": round(ms, 5), "launches": e.augment_launches()}
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=5000)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["a", "b", "c", "d", "e", "f"], default=None)
    ap.add_argument("--pair", choices=["ab", "bd", "ef"], default="ab", help="the two loops that are alternated")
    ap.add_argument("--new", type=int, default=2, help="loops (e) / (f): new features per scan")
    ap.add_argument("--calls", action="store_true", help="time augment against augment_device call by call instead")
    args = ap.parse_args()
    dtype = np.float32 if args.dtype == "f32" else np.float64
    if args.calls:
        summary = {"workload": "ekf_augment_calls", "dtype": args.dtype}
        for q in (1, 8, 32):
            ms = {False: [], True: []}
            for _ in range(3):
                for device in (False, True):
                    out = time_calls(4700, dtype, q, device)
                    ms[device].append(out["ms_per_call"])
                    print(json.dumps(out), flush=True)
            summary[f"q{q}"] = {"augment_ms": sorted(ms[False]), "augment_device_ms": sorted(ms[True]),
                                "median_ratio": round(float(np.median(ms[False]) / np.median(ms[True])), 2)}
        print(json.dumps(summary), flush=True)
        return
    if args.pair == "ef" and not args.only:
        summary = {"workload": "ekf_assoc_timing", "pair": "ef", "landmarks": args.landmarks, "dtype": args.dtype,
                   "m": args.m, "new_per_scan": args.new}
        for la in (0, None):
            res = {"e": [], "f": []}
            for r in range(args.rounds):
                for loop in "ef":
                    out = run(loop, args.landmarks, dtype, args.m, args.steps, args.warmup, new=args.new, lookahead=la)
                    res[loop].append(out["steps_per_s"])
                    print(json.dumps(out), flush=True)
            e_, f_ = res["e"], res["f"]
            summary["lookahead_" + ("default" if la is None else str(la))] = {
                "e": {"runs": e_, "median": float(np.median(e_))}, "f": {"runs": f_, "median": float(np.median(f_))},
                "every_e_faster_than_every_f": bool(min(e_) > max(f_)),
                "median_e_over_f": round(float(np.median(e_) / np.median(f_)), 3)}
        print(json.dumps(summary), flush=True)
        return
    res = {"a": [], "b": [], "c": [], "d": [], "e": [], "f": []}
    for r in range(args.rounds):
        for loop in ([args.only] if args.only else list(args.pair) + (["c"] if r in (0, args.rounds - 1) else [])):
            out = run(loop, args.landmarks, dtype, args.m, args.steps, args.warmup, new=args.new)
            res[loop].append(out["steps_per_s"])
            print(json.dumps(out), flush=True)
    size = np.dtype(dtype).itemsize
    summary = {"workload": "ekf_assoc_timing", "landmarks": args.landmarks, "dtype": args.dtype, "m": args.m,
               "pair_bytes": {f"kp{kp}": (2 * args.landmarks * kp + 25 * args.landmarks) * size for kp in (0, 64, 128)}}
    for k, v in res.items():
        if v:
            summary[k] = {"runs": v, "median": float(np.median(v)), "min": min(v), "max": max(v)}
    if res["a"] and res["b"]:
        a, b = res["a"], res["b"]
        summary["every_b_faster_than_every_a"] = bool(min(b) > max(a))
        summary["median_gap_over_range_of_a"] = round((np.median(b) - np.median(a)) / max(max(a) - min(a), 1e-9), 2)
    if res["b"] and res["d"]:
        b, d = res["b"], res["d"]
        summary["every_d_faster_than_every_b"] = bool(min(d) > max(b))
        summary["median_gap_over_range_of_b"] = round((np.median(d) - np.median(b)) / max(max(b) - min(b), 1e-9), 2)
    if res["b"] and res["c"]:
        summary["b_over_c"] = round(float(np.median(res["b"]) / np.median(res["c"])), 3)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
