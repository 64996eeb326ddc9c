#!/usr/bin/env python3
"""The score step (EKFBatch.score) beside the landmark read (EKFBatch.landmarks) it replaces, with window panels pending:
I instances of N landmarks, one m = 32 update per instance (64 columns pending), then --reps of each.  Prints one JSON
line: the host time per call (score: enqueue only; landmarks: launch, copy and synchronise) and the time per score call
with the stream kept full (--reps calls, one synchronise).  For the device time of the kernels -- ekf_score_landmarks_batch
and ekf_score_finish_batch beside ekf_landmark_read_batch, which has the same traffic -- run it under
`rocprofv3 --kernel-trace --stats -- python tools/score_timing.py`.

    python tools/score_timing.py [--instances 8] [--landmarks 2000] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from conan_slam_amd import EKFBatch, Q_TEXTBOOK  # noqa: E402
from landmark_read_timing import Q, R, _obs, _state  # noqa: E402


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8)
    ap.add_argument("--landmarks", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    I, N, reps = args.instances, args.landmarks, args.reps
    rng = np.random.default_rng(1)
    states = [_state(N, 10 + i) for i in range(I)]
    b = EKFBatch(I, n_landmarks=N, quirks=Q_TEXTBOOK)
    for i, (X, P) in enumerate(states):
        b.set_state(i, X, P)
    idf = (rng.permutation(N)[:32] + 1).astype(np.int32)
    dz = [torch.from_numpy(_obs(X, idf, rng).reshape(-1, order="F")).cuda() for X, _ in states]
    di = torch.from_numpy(idf).cuda()
    b.predict(83.0, 0.01, Q, 73.0, 0.01)
    b.update_device([t.data_ptr() for t in dz], [di.data_ptr()] * I, 32, R)
    b.score_reset(reps + 1)
    b.score_set_truth(states[0][0][3:].reshape(N, 2) + 0.5)
    xv = np.array([0.1, -0.1, 0.1], np.float32)
    b.score(xv)  # (first call: code objects)
    b.landmarks()
    b.synchronize()
    t_enqueue, t_read = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        b.landmarks()
        t_read.append(time.perf_counter() - t0)
    b.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        t1 = time.perf_counter()
        b.score(xv)
        t_enqueue.append(time.perf_counter() - t1)
    b.synchronize()
    t_stream = (time.perf_counter() - t0) / reps
    totals, series, calls = b.scores()
    b.close()
    print(json.dumps({"workload": "score_timing", "instances": I, "landmarks": N, "pending_columns": 64, "reps": reps,
                      "landmarks_read_ms": round(1e3 * float(np.median(t_read)), 4),
                      "score_enqueue_ms": round(1e3 * float(np.median(t_enqueue)), 4),
                      "score_stream_ms_per_call": round(1e3 * t_stream, 4),
                      "calls": calls, "valid_landmarks_per_call": float(totals[0, 6] / calls)}))


if __name__ == "__main__":
    main()
