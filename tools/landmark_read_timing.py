#!/usr/bin/env python3
"""Wall time of the landmark read (EKFBatch.landmarks / EKF.landmarks) against the get_state route, with window panels
pending: one batch read of I x N landmarks against an I-instance get_state loop (each flushes, mirrors and copies P),
and the single filter at N_single.  Prints one JSON line (medians over --reps).  For the device time of the read
kernels, run it under `rocprofv3 --kernel-trace --stats -- python tools/landmark_read_timing.py`.

    python tools/landmark_read_timing.py [--instances 8] [--landmarks 2000] [--single 5000] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from conan_slam_amd import EKF, EKFBatch, Q_TEXTBOOK  # noqa: E402

Q = np.diag([0.18, 6e-4]).astype(np.float32)
R = np.diag([0.08, 0.0024]).astype(np.float32)


def _state(N, seed):
    rng = np.random.default_rng(seed)
    X = np.concatenate([[0.0, 0.0, 0.1], rng.uniform(-500, 500, 2 * N)]).astype(np.float32)
    P = np.eye(3 + 2 * N, dtype=np.float32, order="F")
    P[:3, :3] *= 1e-2
    return X, P


def _obs(X, idf, rng):
    fx = 3 + 2 * (idf - 1)
    dx, dy = X[fx] - X[0], X[fx + 1] - X[1]
    Z = np.stack([np.hypot(dx, dy) + 0.1 * rng.normal(size=idf.size),
                  np.arctan2(dy, dx) - X[2] + 0.01 * rng.normal(size=idf.size)])
    return np.asfortranarray(Z.astype(np.float32))


def _median_ms(fn, reps):
    fn()  # (first call: allocations)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(ts)), 3)


def batch_case(I, N, reps):
    import torch

    rng = np.random.default_rng(1)
    states = [_state(N, 10 + i) for i in range(I)]
    b = EKFBatch(I, n_landmarks=N, quirks=Q_TEXTBOOK)
    for i, (X, P) in enumerate(states):
        b.set_state(i, X, P)
    keep = []

    def pend():  # one window of one m = 32 update per instance: 64 columns pending
        idf = (rng.permutation(N)[:32] + 1).astype(np.int32)
        dz = [torch.from_numpy(_obs(X, idf, rng).reshape(-1, order="F")).cuda() for X, _ in states]
        di = torch.from_numpy(idf).cuda()
        keep.extend(dz + [di])
        b.predict(83.0, 0.01, Q, 73.0, 0.01)
        b.update_device([t.data_ptr() for t in dz], [di.data_ptr()] * I, 32, R)
        b.synchronize()

    pend()
    t_read = _median_ms(lambda: b.landmarks(), reps)

    def get_state_loop():
        pend()  # (get_state flushes: give every timed loop pending panels again)
        t0 = time.perf_counter()
        for i in range(I):
            b.get_state(i)
        return time.perf_counter() - t0

    get_state_loop()
    t_state = round(1e3 * float(np.median([get_state_loop() for _ in range(max(reps // 4, 3))])), 3)
    b.close()
    return {"instances": I, "landmarks": N, "read_ms": t_read, "get_state_loop_ms": t_state,
            "ratio": round(t_state / t_read, 1)}


def single_case(N, reps):
    rng = np.random.default_rng(2)
    X, P = _state(N, 3)
    e = EKF(N, dtype=np.float32, quirks=Q_TEXTBOOK, sync_mode=False)
    e.set_state(X, P)
    e.set_deferred(128)

    def pend():
        idf = (rng.permutation(N)[:32] + 1).astype(np.int32)
        e.predict(83.0, 0.01, Q, 73.0, 0.01)
        e.update(_obs(X, idf, rng), R, idf, True)
        e.synchronize()

    pend()
    t_read = _median_ms(lambda: e.landmarks(), reps)

    def get_state_once():
        pend()
        t0 = time.perf_counter()
        e.get_state()
        return time.perf_counter() - t0

    get_state_once()
    t_state = round(1e3 * float(np.median([get_state_once() for _ in range(max(reps // 4, 3))])), 3)
    e.close()
    return {"landmarks": N, "read_ms": t_read, "get_state_ms": t_state, "ratio": round(t_state / t_read, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8)
    ap.add_argument("--landmarks", type=int, default=2000)
    ap.add_argument("--single", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    print(json.dumps({"workload": "landmark_read", "batch": batch_case(args.instances, args.landmarks, args.reps),
                      "single": single_case(args.single, args.reps)}))


if __name__ == "__main__":
    main()
