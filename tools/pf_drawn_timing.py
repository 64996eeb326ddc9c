"""What the device-side draws buy one FastSLAM-2 observation step (m = 8, f32, resample forced on every step).

Three loops over the same observations, each from the same particle set, each ending in one synchronise:
  (a) observation_step, every normal and stratum drawn with numpy BEFORE the timed loop -- the staged copy alone
  (b) observation_step with the numpy draws inside the loop, as callers run it today
  (c) observation_step_drawn -- launches only
One process; a / b / c alternated `--rounds` times, `--steps` steps each; medians and ranges are printed, and one JSON
line at the end.  Configurations: 512 x 1000 (particles x features) and 8192 x 16, where the per-particle arrays dominate
the inputs.  `--only a|c --rounds 1` runs a single loop (for a kernel trace of its own).
Usage (GPU box): python tools/pf_drawn_timing.py [--steps 2000] [--rounds 5] [--config 512x1000] [--only a]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conan_slam_amd.pf import ParticleShard, stratified_random  # noqa: E402
from conan_slam_amd.synth import Workload, normal, uniform01  # noqa: E402

dtype = np.float32
M_OBS = 8


def host_draws(t, Np):
    """The per-step draws as tools/pf_host_breakdown.py and bench.py make them."""
    nrm = np.ascontiguousarray(normal(500 + t, np.arange(3 * Np, dtype=np.uint64)).reshape(3, Np).astype(dtype))
    sel = stratified_random(Np, uniform01(900 + t, np.arange(Np, dtype=np.uint64)), dtype)
    return nrm, sel


class Bench:
    def __init__(self, Np, Nf, steps):
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
        self.pre = [host_draws(t, Np) for t in range(steps)]
        self.alive, self.calls0, self.res0 = True, 0, 0

    def reset(self):
        """Every loop starts from the same set: the initial particle, gathered into every slot."""
        self.sh.set_particle(0, *self.first)
        self.sh.gather_local(np.zeros(self.Np, np.int32), 1.0 / self.Np)

    def run(self, which, steps=None):
        sh, w, Np = self.sh, self.w, self.Np
        steps = self.steps if steps is None else steps
        self.reset()
        sh.synchronize()
        t0 = time.perf_counter()
        for t in range(steps):
            (Z, idf), (v, swa) = self.obs[t], self.ctl[t]
            if which == "c":
                sh.observation_step_drawn(v, swa, w.QE, w.wb, w.dt, Z, idf, w.RE, t, Np + 1, True)
            else:
                nrm, sel = self.pre[t] if which == "a" else host_draws(t, Np)
                sh.observation_step(v, swa, w.QE, w.wb, w.dt, Z, idf, w.RE, nrm, sel, Np + 1, True)
        sh.synchronize()
        dt = time.perf_counter() - t0
        # a live filter: finite weights, and the forced resample of every step of this loop happened
        self.alive = self.alive and bool(np.all(np.isfinite(sh.get_weights())))
        calls, resamples, neff = sh.resample_stats()
        self.alive = self.alive and np.isfinite(neff) and (calls - self.calls0, resamples - self.res0) == (steps, steps)
        self.calls0, self.res0 = calls, resamples
        return dt / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", action="append", help="particles x features, e.g. 512x1000 (may be repeated)")
    ap.add_argument("--only", choices=["a", "b", "c"], help="run this loop alone")
    args = ap.parse_args()
    configs = [tuple(int(x) for x in c.split("x")) for c in (args.config or ["512x1000", "8192x16"])]
    loops = [args.only] if args.only else ["a", "b", "c"]
    out = {}
    for Np, Nf in configs:
        b = Bench(Np, Nf, args.steps)
        for k in loops:  # warm-up: every kernel and both staging paths once
            b.run(k, min(50, args.steps))
        copies0 = b.sh.stage_copies()
        res = {k: [] for k in loops}
        for _ in range(args.rounds):
            for k in loops:
                res[k].append(b.run(k))
        print(f"{Np} x {Nf}, m = {M_OBS}, {args.steps} steps per loop, {args.rounds} rounds (us per step, wall clock, synchronised)")
        for k in loops:
            v = res[k]
            print(f"  ({k}) median {np.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}   runs " +
                  " ".join(f"{x:.2f}" for x in v))
        if not args.only:
            a, c = np.median(res["a"]), np.median(res["c"])
            print(f"  (c) - (a) = {c - a:+.2f} us; the spread of (a)'s own runs is {max(res['a']) - min(res['a']):.2f} us; "
                  f"(b) - (a) = {np.median(res['b']) - a:+.2f} us of numpy on the host")
        print(f"  weights finite and every forced resample performed in every loop: {'yes' if b.alive else 'NO'}")
        print(f"  staged copies in the timed loops: {b.sh.stage_copies() - copies0} "
              f"(one per step of (a) and (b), none for (c))")
        out[f"{Np}x{Nf}"] = res
        b.sh.close()
    print(json.dumps({"tool": "pf_drawn_timing", "steps": args.steps, "us_per_step": out}))


if __name__ == "__main__":
    main()
