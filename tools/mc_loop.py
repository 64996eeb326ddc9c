#!/usr/bin/env python3
"""Times the reference's Monte-Carlo unit at its own cadence (test/main.cpp:132-200): one cycle is
6 x (predict + observeHeading), then update (m observations), then augment of one landmark.

Two drivers run the same calls on `instances` filters of N landmarks:
  batch    one EKFBatch: one launch per stage for all instances (cslam_ekf_batch_predict / observe_heading / update /
           augment);
  handles  one EKF handle per filter, one host thread each (the calls release the GIL), each on its own streams.
Prints one JSON line: cycles per second of each driver (a cycle advances every instance by one cycle).

    python tools/mc_loop.py [--instances 8] [--N 2000] [--m 32] [--cycles 50] [--warmup 3]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from conan_slam_amd import EKF, EKFBatch, Q_REF_EXACT  # noqa: E402
from conan_slam_amd.synth import Workload  # noqa: E402

SUB = 6  # control steps per observation step (test/main.cpp:165-174)


def make_inputs(I, N, m, cycles, seed=0):
    """Per instance: its initial state and, per cycle, the observations (2 x m, idf) and the new landmark (2 x 1); the
    controls and headings (common to the instances, as in the reference driver, which observes the true heading)."""
    import torch

    loads = [Workload(N, m, np.float32, seed=seed + i, corr=0.1) for i in range(I)]
    v, wb, dt = loads[0].v, loads[0].wb, loads[0].dt
    pose = np.zeros(3)
    ctrl, phis, poses = [], [], []
    for t in range(cycles * SUB):
        swa = 0.05 * np.sin(0.01 * t)
        pose = pose + [v * dt * np.cos(swa + pose[2]), v * dt * np.sin(swa + pose[2]), v * dt * np.sin(swa) / wb]
        ctrl.append((v, swa))
        phis.append(float(pose[2]))
        if t % SUB == SUB - 1:
            poses.append(pose.copy())
    per = []
    for i, w in enumerate(loads):
        rng = np.random.default_rng(100 + i)
        Zs, ids, Zn = [], [], []
        for c in range(cycles):
            pick = np.sort(rng.permutation(N)[:m])
            dx, dy = w.LM[0, pick] - poses[c][0], w.LM[1, pick] - poses[c][1]
            Z = np.empty((2, m))
            Z[0] = np.hypot(dx, dy) + rng.normal(size=m) * np.sqrt(float(w.R[0, 0]))
            Z[1] = np.arctan2(dy, dx) - poses[c][2] + rng.normal(size=m) * np.sqrt(float(w.R[1, 1]))
            Zs.append(Z.reshape(-1, order="F"))
            ids.append(pick + 1)
            Zn.append([200.0 + 5 * c, 0.3 * np.sin(c + i)])
        per.append(dict(X0=w.X0, P0=w.P0,
                        dZ=torch.from_numpy(np.concatenate(Zs).astype(np.float32)).cuda(),
                        dI=torch.from_numpy(np.concatenate(ids).astype(np.int32)).cuda(),
                        dZn=torch.from_numpy(np.asarray(Zn, np.float32).reshape(-1)).cuda(),
                        Zn=np.asarray(Zn, np.float32)))
    torch.cuda.synchronize()
    return loads[0], ctrl, phis, per


def run_batch(w, ctrl, phis, per, N, m, warm, cycles, quirks):
    I = len(per)
    b = EKFBatch(I, n_landmarks=N, max_landmarks=N + warm + cycles, quirks=quirks)
    for i, p in enumerate(per):
        b.set_state(i, p["X0"], p["P0"])

    def cycle(c):
        for s in range(SUB):
            t = c * SUB + s
            b.predict(ctrl[t][0], ctrl[t][1], w.QE, w.wb, w.dt)
            b.observe_heading(phis[t], True)
        b.update_device([p["dZ"].data_ptr() + c * 2 * m * 4 for p in per], [p["dI"].data_ptr() + c * m * 4 for p in per],
                        m, w.RE)
        b.augment_device([p["dZn"].data_ptr() + c * 2 * 4 for p in per], 1, w.RE)

    for c in range(warm):
        cycle(c)
    b.synchronize()
    t0 = time.perf_counter()
    for c in range(warm, warm + cycles):
        cycle(c)
    b.synchronize()
    el = time.perf_counter() - t0
    flags = b.factor_status()
    b.close()
    return cycles / el, flags


def run_handles(w, ctrl, phis, per, N, m, warm, cycles, quirks):
    I = len(per)
    engs = []
    for p in per:
        e = EKF(N + warm + cycles, dtype=np.float32, quirks=quirks, sync_mode=False)
        e.set_state(p["X0"], p["P0"])
        engs.append(e)

    def cycle(e, p, c):
        for s in range(SUB):
            t = c * SUB + s
            e.predict(ctrl[t][0], ctrl[t][1], w.QE, w.wb, w.dt)
            e.observe_heading(phis[t], True)
        e.update_device(p["dZ"].data_ptr() + c * 2 * m * 4, m, w.RE, p["dI"].data_ptr() + c * m * 4, batch=True)
        e.augment(p["Zn"][c].reshape(2, 1), w.RE)

    for e, p in zip(engs, per):
        for c in range(warm):
            cycle(e, p, c)
        e.synchronize()
    go = threading.Barrier(I + 1)
    errors = []

    def body(e, p):
        try:
            go.wait()
            for c in range(warm, warm + cycles):
                cycle(e, p, c)
            e.synchronize()
        except Exception as ex:  # (reported by the main thread)
            errors.append(ex)

    th = [threading.Thread(target=body, args=(e, p)) for e, p in zip(engs, per)]
    for t in th:
        t.start()
    go.wait()
    t0 = time.perf_counter()
    for t in th:
        t.join()
    el = time.perf_counter() - t0
    if errors:
        raise errors[0]
    flags = [e.factor_status() for e in engs]
    for e in engs:
        e.close()
    return cycles / el, flags


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", type=int, default=8)
    ap.add_argument("--N", type=int, default=2000)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--cycles", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quirks", type=int, default=Q_REF_EXACT)
    a = ap.parse_args()
    w, ctrl, phis, per = make_inputs(a.instances, a.N, a.m, a.warmup + a.cycles)
    args = (w, ctrl, phis, per, a.N, a.m, a.warmup, a.cycles, a.quirks)
    batch, fb = run_batch(*args)
    handles, fh = run_handles(*args)
    print(json.dumps({"tool": "mc_loop", "instances": a.instances, "N": a.N, "m": a.m, "cycles": a.cycles,
                      "steps_per_cycle": f"{SUB} x (predict + heading) + update + augment(1)",
                      "batch_cycles_per_s": round(batch, 2), "handles_cycles_per_s": round(handles, 2),
                      "batch_over_handles": round(batch / handles, 3), "batch_flags": fb, "handle_flags": fh}))


if __name__ == "__main__":
    main()
