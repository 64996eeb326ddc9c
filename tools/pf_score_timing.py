"""What scoring on the device buys a Monte-Carlo study of the particle filter (m = 8, f32, resample forced on every step).

Three loops over the same observations, each from the same particle set, each ending in one synchronise:
  (a) observation_step_drawn only -- the filter without a score
  (b) observation_step_drawn + estimate() + the numpy scorer (tests/score_ref.py through tests/pf_score_ref.py): what a
      caller who wants a score per step had to do before -- a copy, a synchronise and the host solves per step
  (c) observation_step_drawn + score(), and ONE scores() at the end
One process; a / b / c alternated `--rounds` times, `--steps` steps each; medians and ranges are printed, and one JSON
line at the end.  Configurations: 512 x 1000 (particles x features) and 8192 x 16.  The totals of (b) and (c) are
compared after the first round (counts equal, sums within the restatement's bounds).
Usage (GPU box): python tools/pf_score_timing.py [--steps 1000] [--rounds 5] [--config 512x1000] [--only c]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # (tests/pf_builders.py, which the restatement's helper imports)
from conan_slam_amd.pf import ParticleShard  # noqa: E402
from conan_slam_amd.synth import Workload  # noqa: E402

dtype = np.float32
M_OBS = 8


class Bench:
    def __init__(self, Np, Nf, steps):
        from pf_score_ref import PfScoreRef

        self.Np, self.Nf, self.steps = Np, Nf, steps
        self.w = Workload(Nf, M_OBS, dtype, seed=0, build_p=False)
        self.obs = [self.w.observations(t) for t in range(steps)]
        self.ctl = [self.w.controls(t) for t in range(steps)]
        self.sh = ParticleShard(Np, Nf, dtype=dtype, n_global=Np)
        self.sh.seed_draws(12345)
        XF = np.asfortranarray(np.stack([self.w.X0[3::2], self.w.X0[4::2]]).astype(dtype))
        PF = np.asfortranarray(np.tile(np.array([1, 0, 0, 1], dtype=dtype)[:, None], (1, Nf)))
        Pv = np.diag([0.05, 0.05, 1e-4]).astype(dtype)
        self.first = (1.0 / Np, np.zeros(3, dtype), Pv, XF, PF)
        self.truth = np.ascontiguousarray(XF.T.astype(np.float64))
        self.xv_true = [np.array([1e-3 * t, -1e-3 * t, 1e-4 * t]) for t in range(steps)]
        self.sh.score_set_truth(self.truth)
        self.make_ref = lambda: PfScoreRef(dtype, "mean", 0)
        self.ref, self.scores = None, None
        self.alive, self.calls0, self.res0 = True, 0, 0

    def reset(self):
        """Every loop starts from the same set: the initial particle, gathered into every slot."""
        self.sh.set_particle(0, *self.first)
        self.sh.gather_local(np.zeros(self.Np, np.int32), 1.0 / self.Np)

    def run(self, which, steps=None):
        sh, w, Np = self.sh, self.w, self.Np
        steps = self.steps if steps is None else steps
        self.reset()
        ref = self.make_ref()
        sh.score_reset("mean", 0)
        sh.synchronize()
        t0 = time.perf_counter()
        for t in range(steps):
            (Z, idf), (v, swa) = self.obs[t], self.ctl[t]
            sh.observation_step_drawn(v, swa, w.QE, w.wb, w.dt, Z, idf, w.RE, t, Np + 1, True)
            if which == "b":
                ref.add(sh.estimate(), self.truth, self.xv_true[t])
            elif which == "c":
                sh.score(self.xv_true[t])
        if which == "c":
            self.scores = sh.scores()
        else:
            sh.synchronize()
        dt = time.perf_counter() - t0
        if which == "b":
            self.ref = ref
        self.alive = self.alive and bool(np.all(np.isfinite(sh.get_weights())))
        calls, resamples, neff = sh.resample_stats()
        self.alive = self.alive and np.isfinite(neff) and (calls - self.calls0, resamples - self.res0) == (steps, steps)
        self.calls0, self.res0 = calls, resamples
        return dt / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", action="append", help="particles x features, e.g. 512x1000 (may be repeated)")
    ap.add_argument("--only", choices=["a", "b", "c"], help="run this loop alone")
    args = ap.parse_args()
    configs = [tuple(int(x) for x in c.split("x")) for c in (args.config or ["512x1000", "8192x16"])]
    loops = [args.only] if args.only else ["a", "b", "c"]
    out = {}
    for Np, Nf in configs:
        b = Bench(Np, Nf, args.steps)
        for k in loops:  # warm-up: every kernel once, every buffer grown
            b.run(k, min(50, args.steps))
        copies0 = b.sh.stage_copies()
        res = {k: [] for k in loops}
        for r in range(args.rounds):
            for k in loops:
                res[k].append(b.run(k))
            if r == 0 and not args.only:
                b.ref.check(b.scores, f"{Np}x{Nf}: device totals against the host scorer's")
        print(f"{Np} x {Nf}, m = {M_OBS}, {args.steps} steps per loop, {args.rounds} rounds (us per step, wall clock, synchronised)")
        for k in loops:
            v = res[k]
            print(f"  ({k}) median {np.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}   runs " +
                  " ".join(f"{x:.2f}" for x in v))
        if not args.only:
            a, bb, c = (np.median(res[k]) for k in "abc")
            print(f"  the score costs (c) - (a) = {c - a:+.2f} us per step on the device, (b) - (a) = {bb - a:+.2f} us through the "
                  f"host; (c) is {'faster' if c < bb else 'NOT faster'} than (b)")
            print("  device totals equal the host scorer's (counts exact, sums within the restatement's bounds): yes")
        print(f"  weights finite and every forced resample performed in every loop: {'yes' if b.alive else 'NO'}")
        print(f"  staged copies in the timed loops: {b.sh.stage_copies() - copies0} (none: neither the steps nor the score stage one)")
        out[f"{Np}x{Nf}"] = res
        b.sh.close()
    print(json.dumps({"tool": "pf_score_timing", "steps": args.steps, "us_per_step": out}))


if __name__ == "__main__":
    main()
