"""What the fused new-feature scan costs per call, against the separate calls and against the host round trip (f32, q = 2).

Three loops, each from the same particle set (every particle a copy of one, Nf mapped features), each ending in one
synchronise.  One iteration is one scan that observes only new features (test/main.cpp:314-328) behind its predict:
  (a) new_feature_step_drawn                          -- the draw launch + one launch for predict, sample, Pv = 0, add
  (b) predict + sample_pose_drawn + add_features      -- the same work as separate calls (four launches, one staged copy)
  (c) get_particle x np (pose and Pv only), the sample with numpy on the host, set_particle x np, add_features -- the only
      route without the pose-sample call: one stream drain per particle and direction
The store has room for Nf + q * iters features, so a loop of `--iters` scans runs between two synchronisations without
filling it; every loop starts again from Nf.  After the first scan Pv = 0, so every later scan samples from the rank-2
covariance one predict adds: the Jacobi branch of the factorisation, which is what a first scan from P = 0 meets too.
(a) and (b) alternate `--rounds` times with `--iters` scans each; (c) runs `--host-iters` scans per round.  Medians and
ranges are printed, and one JSON line at the end.
`--only a|b --rounds 1` runs a single loop (for a kernel trace of its own).
Usage (GPU box): python tools/pf_new_feature_timing.py [--iters 1000] [--rounds 5] [--host-iters 2] [--config 512x1000]
                 [--only a]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conan_slam_amd.pf import ParticleShard  # noqa: E402
from conan_slam_amd.synth import Workload  # noqa: E402

dtype = np.float32
Q_NEW = 2


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Bench:
    def __init__(self, Np, Nf, iters):
        self.Np, self.Nf, self.iters = Np, Nf, iters
        self.w = Workload(Nf, 8, dtype, seed=0, build_p=False)
        self.v, self.swa = self.w.controls(0)
        self.sh = ParticleShard(Np, Nf + Q_NEW * iters, dtype=dtype, n_global=Np)
        self.sh.seed_draws(12345)
        XF = np.asfortranarray(np.stack([self.w.X0[3::2], self.w.X0[4::2]]).astype(dtype))
        PF = np.asfortranarray(np.tile(np.array([1, 0, 0, 1], dtype=dtype)[:, None], (1, Nf)))
        Pv = np.diag([0.05, 0.05, 1e-4]).astype(dtype)
        self.first = (1.0 / Np, np.zeros(3, dtype), Pv, XF, PF)
        self.Z = np.asfortranarray(np.array([[25.0, 40.0], [0.4, -0.9]], dtype=dtype))
        self.alive = True

    def reset(self):
        """Every loop starts from the same set: the initial particle, gathered into every slot; Nf features."""
        self.sh.set_particle(0, *self.first)
        self.sh.gather_local(np.zeros(self.Np, np.int32), 1.0 / self.Np)

    def host_scan(self, t):
        """(c): the poses come to the host one particle at a time, are sampled there and go back the same way."""
        sh, L, h, Np = self.sh, self.sh._L, self.sh._h, self.Np
        X, P = np.zeros(3, dtype), np.zeros((3, 3), dtype, order="F")
        z = np.random.default_rng(t).normal(size=(Np, 3)).astype(dtype)
        nf = C.c_int(sh.n_features)
        for i in range(Np):
            L.cslam_pf_get_particle(h, C.c_int(i), None, _vp(X), _vp(P), None, None)
            try:
                F = np.linalg.cholesky(P.astype(np.float64))
            except np.linalg.LinAlgError:
                ev, V = np.linalg.eigh(P.astype(np.float64))
                F = V * np.sqrt(np.maximum(ev, 0.0))
            X[:] = (F @ z[i] + X).astype(dtype)
            P[:] = 0
            L.cslam_pf_set_particle(h, C.c_int(i), None, _vp(X), _vp(P), None, None, nf)

    def run(self, which, iters):
        sh, w = self.sh, self.w
        self.reset()
        sh.synchronize()
        t0 = time.perf_counter()
        for t in range(iters):
            if which == "a":
                sh.new_feature_step_drawn(self.v, self.swa, w.QE, w.wb, w.dt, self.Z, w.RE, t)
            elif which == "b":
                sh.predict(self.v, self.swa, w.QE, w.wb, w.dt)
                sh.sample_pose_drawn(t)
                sh.add_features(self.Z, w.RE)
            else:
                sh.predict(self.v, self.swa, w.QE, w.wb, w.dt)
                self.host_scan(t)
                sh.add_features(self.Z, w.RE)
        sh.synchronize()
        dt = time.perf_counter() - t0
        # a live set: the features were counted, the first and the last particle are finite and their Pv is zero
        ok = sh.n_features == self.Nf + Q_NEW * iters
        for i in (0, self.Np - 1):
            _, Xv, Pv, XF, PF = sh.get_particle(i)
            ok = ok and bool(np.all(np.isfinite(Xv)) and np.all(Pv == 0) and np.all(np.isfinite(XF)) and np.all(np.isfinite(PF)))
        self.alive = self.alive and ok
        return dt / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--config", action="append", help="particles x features, e.g. 512x1000 (may be repeated)")
    ap.add_argument("--only", choices=["a", "b", "c"], help="run this loop alone (for a kernel trace of its own)")
    args = ap.parse_args()
    loops = [args.only] if args.only else ["a", "b", "c"]
    configs = [tuple(int(x) for x in c.split("x")) for c in (args.config or ["512x1000", "8192x16"])]
    out = {}
    for Np, Nf in configs:
        b = Bench(Np, Nf, args.iters)
        for k in loops:  # warm-up: every kernel and the staging path once
            if k != "c":
                b.run(k, min(50, args.iters))
        res = {k: [] for k in loops}
        copies = {}
        for _ in range(args.rounds):
            for k in loops:
                c0 = b.sh.stage_copies()
                res[k].append(b.run(k, args.host_iters if k == "c" else args.iters))
                copies[k] = b.sh.stage_copies() - c0
        print(f"{Np} x {Nf}, q = {Q_NEW}, {args.iters} scans per loop of (a) and (b), {args.host_iters} of (c), "
              f"{args.rounds} rounds (us per scan, wall clock, synchronised)")
        for k in loops:
            v = res[k]
            print(f"  ({k}) median {np.median(v):10.2f}   min {min(v):10.2f}   max {max(v):10.2f}   runs " +
                  " ".join(f"{x:.2f}" for x in v))
        if not args.only:
            print(f"  (a) worst {max(res['a']):.2f} vs (b) best {min(res['b']):.2f}; (b) worst {max(res['b']):.2f}; "
                  f"(c) / (a) = {np.median(res['c']) / np.median(res['a']):.0f}x")
        print("  staged copies per loop: " + ", ".join(f"({k}) {copies[k]}" for k in loops))
        print(f"  every loop counted its features and left finite particles with Pv = 0: {'yes' if b.alive else 'NO'}")
        out[f"{Np}x{Nf}"] = res
        b.sh.close()
    print(json.dumps({"tool": "pf_new_feature_timing", "iters": args.iters, "host_iters": args.host_iters, "q": Q_NEW,
                      "us_per_scan": out}))


if __name__ == "__main__":
    main()
