"""What scoring on the device costs, and buys, a consistency study of the single EKF handle.

The headline call sequence of bench.py (predict + update_device with m = 32 observations resident in HBM, deferred(128),
asynchronous mode, look-ahead windows), N = 5000 in f32 and N = 1000 in f64.  Four loops over the same inputs, each from
the same state, each ending in one synchronise:
  (a) the unscored run
  (b) score() after every SECOND update -- at the window boundaries, where nothing is queued: no window is split
  (c) score() after EVERY update -- the queued update is launched alone, as a window of one, so the run makes twice the
      windows and P-GEMMs of (a); the printed window counts show it
  (d) the host route after every update: landmarks() + pose() + the numpy scorer (tests/score_ref.py) -- a launch, two
      copies and a synchronise per step, then N 2 x 2 solves on the host; it splits the windows as (c) does
(b) and (c) read their totals with ONE scores() at the end.  One process; a / b / c / d alternated `--rounds` times,
`--steps` steps each; medians and ranges are printed, and one JSON line at the end.  After the first round the totals of
(c) are compared with the host scorer's of (d): counts equal, sums within the restatement's bounds.
Usage (GPU box): python tools/ekf_score_timing.py [--steps 400] [--rounds 5] [--config 5000xf32] [--only b]
For the launch sequence of (b) beside (a): rocprofv3 --kernel-trace --output-format csv -d out -o run -- python3
tools/ekf_score_timing.py --config 5000xf32 --only b --steps 8 --rounds 1, then tools/trace_timeline.py --sequence."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conan_slam_amd import EKF, Q_TEXTBOOK  # noqa: E402
from conan_slam_amd.synth import Workload  # noqa: E402

M_OBS = 32
DTYPES = {"f32": np.float32, "f64": np.float64}


class Bench:
    def __init__(self, N, dtype, steps):
        import torch

        self.N, self.dtype, self.steps = N, np.dtype(dtype), steps
        self.w = w = Workload(N, M_OBS, dtype, seed=0)
        self.ctl, Zh, Ih, self.xv_true = [], [], [], []
        for t in range(steps):
            self.ctl.append(w.controls(t))
            Z, idf = w.observations(t)
            Zh.append(Z.reshape(-1, order="F"))
            Ih.append(idf)
            self.xv_true.append(np.array(w.true_pose_after(t), np.float64))
        self.dZ = torch.from_numpy(np.ascontiguousarray(np.stack(Zh), dtype=dtype)).cuda()
        self.dI = torch.from_numpy(np.ascontiguousarray(np.stack(Ih), dtype=np.int32)).cuda()
        torch.cuda.synchronize()
        self.truth = np.ascontiguousarray(w.LM.T, dtype=np.float64)
        self.e = EKF(N, dtype=dtype, quirks=Q_TEXTBOOK, sync_mode=False)
        self.e.score_set_truth(self.truth)
        self.windows, self.scores, self.ref = {}, None, None

    def run(self, which, steps=None):
        import score_ref

        e, w = self.e, self.w
        steps = self.steps if steps is None else steps
        zs = 2 * M_OBS * self.dtype.itemsize
        e.set_state(w.X0, w.P0)  # every loop starts from the same state
        e.set_deferred(128)
        e.score_reset(0)
        acc = score_ref.Accumulator(1, 0)
        w0 = e.lookahead_windows()
        e.synchronize()
        t0 = time.perf_counter()
        for t in range(steps):
            v, swa = self.ctl[t]
            e.predict(v, swa, w.QE, w.wb, w.dt)
            e.update_device(self.dZ.data_ptr() + t * zs, M_OBS, w.RE, self.dI.data_ptr() + t * 4 * M_OBS, batch=True)
            if which == "c" or (which == "b" and t % 2 == 1):
                e.score(self.xv_true[t])
            elif which == "d":
                xl, pll, _ = e.landmarks()
                x, pvv = e.pose()
                acc.add(x[None], pvv[None], xl[None], pll[None], self.truth, self.xv_true[t])
        scores = e.scores() if which in "bc" else None
        e.flush()
        e.synchronize()
        dt = time.perf_counter() - t0
        self.windows[which] = e.lookahead_windows() - w0
        if which == "c":
            self.scores = scores
        if which == "d":
            self.ref = acc
        return dt / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", action="append", help="landmarks x dtype, e.g. 5000xf32 (may be repeated)")
    ap.add_argument("--only", choices=["a", "b", "c", "d"], help="run this loop alone")
    args = ap.parse_args()
    configs = [(int(c.split("x")[0]), c.split("x")[1]) for c in (args.config or ["5000xf32", "1000xf64"])]
    loops = [args.only] if args.only else ["a", "b", "c", "d"]
    out = {}
    for N, dname in configs:
        b = Bench(N, DTYPES[dname], args.steps)
        for k in loops:  # warm-up: every kernel once, every buffer grown
            b.run(k, min(20, args.steps))
        res = {k: [] for k in loops}
        for r in range(args.rounds):
            for k in loops:
                res[k].append(b.run(k))
            if r == 0 and not args.only:
                totals, series, track, calls = b.scores
                b.ref.check(totals[None], series[:, None, :], calls, f"{N} x {dname}: device totals against the host scorer's")
        print(f"N = {N}, {dname}, m = {M_OBS}, deferred(128), {args.steps} steps per loop, {args.rounds} rounds "
              "(us per step, wall clock, synchronised)")
        for k in loops:
            v = res[k]
            print(f"  ({k}) median {np.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}   windows {b.windows[k]:5d}   runs "
                  + " ".join(f"{x:.2f}" for x in v))
        if not args.only:
            a, bb, c, d = (np.median(res[k]) for k in "abcd")
            print(f"  a score at every window boundary costs (b) - (a) = {bb - a:+.2f} us per step ({2 * (bb - a):+.2f} us per "
                  "score call)")
            print(f"  a score after every update costs (c) - (a) = {c - a:+.2f} us per step: it launches the queued update as a "
                  f"window of one ({b.windows['c']} windows against {b.windows['a']})")
            print(f"  the host route costs (d) - (a) = {d - a:+.2f} us per step; (c) is {'faster' if c < d else 'NOT faster'} "
                  "than (d)")
            print("  device totals of (c) equal the host scorer's of (d) (counts exact, sums within the restatement's bounds): yes")
        out[f"{N}x{dname}"] = {"us_per_step": res, "windows": dict(b.windows)}
        b.e.close()
    print(json.dumps({"tool": "ekf_score_timing", "steps": args.steps, "m": M_OBS, "results": out}))


if __name__ == "__main__":
    main()
