#!/usr/bin/env python3
"""What one iteration block of the FastSLAM-1 loop costs: k = 6 heading-known control steps with per-particle control
noise and one scan of m = 8 known features (f32, resample forced on every scan), three ways:
  (a)  fs1_cycle_drawn: the whole block in one C call
  (b)  the separate new calls: control_run_sampled, likelihood_update (features updated, Pv zeroed),
       resample_local_drawn with nothing returned
  (c)  cycle_drawn: the FastSLAM-2 block on the same inputs, for context (another filter: its end state is not compared)
One process; the forms are alternated `--rounds` times in batches of `--batch` blocks, every batch from the same particle
set (restored, untimed, before it).  Per batch: device events on the handle's own stream around the whole batch and a
host clock around the same blocks ending in the event's synchronise.  Medians and every run are printed, and one JSON
line at the end.  No time is fixed in advance.
Usage (GPU box): python tools/pf_fs1_timing.py [--batch 50] [--rounds 7] [--config 512x1000] [--config 8192x16]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conan_slam_amd import _capi  # noqa: E402
from conan_slam_amd.pf import ParticleShard  # noqa: E402
from conan_slam_amd.synth import Workload  # noqa: E402

dtype = np.float32
M_OBS, K = 8, 6
PATHS = ("a", "b", "c")


class Bench:
    def __init__(self, Np, Nf, batch):
        import torch

        self.torch, self.Np, self.Nf, self.batch = torch, Np, Nf, batch
        self.w = w = Workload(Nf, M_OBS, dtype, seed=0, build_p=False)
        self.blocks = []
        for c in range(batch):  # K control steps (the compass reads the true heading after each), then the scan
            steps = range(c * K, (c + 1) * K)
            ctl = [w.controls(t) for t in steps]
            phi = [float(w.true_pose_after(t)[2]) for t in steps]
            Z, idf = w.observations(steps[-1])
            self.blocks.append((np.array([x[0] for x in ctl]), np.array([x[1] for x in ctl]), np.array(phi), Z, idf))
        self.none = np.zeros((2, 0), dtype)
        self.sh = ParticleShard(Np, Nf, dtype=dtype, n_global=Np)
        self.sh.seed_draws(12345)
        self.stream = torch.cuda.ExternalStream(self.sh.stream_ptr())
        XF = np.asfortranarray(np.stack([w.X0[3::2], w.X0[4::2]]).astype(dtype))
        PF = np.asfortranarray(np.tile(np.array([1, 0, 0, 1], dtype=dtype)[:, None], (1, Nf)))
        Pv = np.diag([0.05, 0.05, 1e-4]).astype(dtype)
        self.first = (1.0 / Np, np.zeros(3, dtype), Pv, XF, PF)
        self.alive, self.ends = True, {}

    def reset(self):
        """Every batch starts from the same set: the initial particle (Nf features), gathered into every slot."""
        self.sh.set_particle(0, *self.first)
        self.sh.gather_local(np.zeros(self.Np, np.int32), 1.0 / self.Np)

    def block(self, which, c):
        sh, w, Np = self.sh, self.w, self.Np
        v, swa, phi, Z, idf = self.blocks[c]
        if which == "a":
            sh.fs1_cycle_drawn(v, swa, w.QE, w.wb, w.dt, c * K, Z, idf, self.none, w.RE, c, Np + 1, True, phi=phi,
                               use_heading=True)
        elif which == "b":
            sh.control_run_sampled(v, swa, w.QE, w.wb, w.dt, c * K, phi=phi, use_heading=True)
            sh.likelihood_update(Z, idf, w.RE, True, True)
            sh.resample_local_drawn(c, Np + 1, True, want_result=False)
        else:
            sh.cycle_drawn(v, swa, w.QE, w.wb, w.dt, Z, idf, self.none, w.RE, c, Np + 1, True, phi=phi, use_heading=True)

    def run(self, which, blocks=None):
        """-> (us per block by device events, us per block by the host clock)"""
        torch, sh = self.torch, self.sh
        blocks = self.batch if blocks is None else blocks
        self.reset()
        sh.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        t0 = time.perf_counter()
        for c in range(blocks):
            self.block(which, c)
        e1.record(self.stream)
        e1.synchronize()
        host = (time.perf_counter() - t0) * 1e6 / blocks
        dev = e0.elapsed_time(e1) * 1e3 / blocks
        # a live filter that did what was asked: finite weights, and the two FastSLAM-1 forms end with the same best
        # particle, bit for bit
        wts = sh.get_weights()
        best = sh.best_particle()
        end = (wts.tobytes(), best.Xv.tobytes(), best.Pv.tobytes())
        family = ("fs1" if which in "ab" else "fs2", blocks)
        self.alive = self.alive and bool(np.all(np.isfinite(wts))) and self.ends.setdefault(family, end) == end
        return dev, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--config", action="append", help="particles x features, e.g. 512x1000 (may be repeated)")
    args = ap.parse_args()
    if _capi.device_count() == 0:
        raise SystemExit("pf_fs1_timing: no HIP device (there is nothing to time without one)")
    configs = [tuple(int(x) for x in c.split("x")) for c in (args.config or ["512x1000", "8192x16"])]
    out = {}
    for Np, Nf in configs:
        b = Bench(Np, Nf, args.batch)
        for k in PATHS:  # warm-up: every kernel and every staging path once
            b.run(k, min(10, args.batch))
        dev, host = {k: [] for k in PATHS}, {k: [] for k in PATHS}
        for _ in range(args.rounds):
            for k in PATHS:
                d, h = b.run(k)
                dev[k].append(d)
                host[k].append(h)
        print(f"{Np} x {Nf}, m = {M_OBS}, k = {K}, f32, {args.batch} blocks per batch, {args.rounds} rounds (us per block)")
        for name, res in (("device events", dev), ("host clock   ", host)):
            for k in PATHS:
                v = res[k]
                print(f"  {name} ({k}) median {np.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}   runs " +
                      " ".join(f"{x:.2f}" for x in v))
        no_slower = bool(np.median(host["a"]) <= np.median(host["b"]) and np.median(dev["a"]) <= np.median(dev["b"]))
        print(f"  the one-call form (a) no slower than the separate calls (b), medians of both clocks: "
              f"{'yes' if no_slower else 'NO'}")
        print(f"  finite weights in every batch, and the same best particle at the end of (a) and (b): "
              f"{'yes' if b.alive else 'NO'}")
        out[f"{Np}x{Nf}"] = dict(device_us=dev, host_us=host, alive=bool(b.alive), a_no_slower_than_b=no_slower)
        b.sh.close()
    print(json.dumps({"tool": "pf_fs1_timing", "batch": args.batch, "rounds": args.rounds, "k": K, "us_per_block": out}))


if __name__ == "__main__":
    main()
