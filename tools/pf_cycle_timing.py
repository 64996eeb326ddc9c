#!/usr/bin/env python3
"""What the control run and the whole-cycle call buy one iteration block of the reference's FastSLAM-2 loop: k = 6
control steps and one scan of m = 8 known features (f32, resample forced on every scan).

With the heading known (mSwitchHeadingKnown = true, the reference's default) three ways to run the same block:
  (a)  6 x (predict, observe_heading), then sample_proposal_drawn, feature_update, resample_local_drawn with nothing
       returned: what a heading-known caller runs with the calls that existed before the control run -- THE YARDSTICK
  (b)  control_run, then the same separate scan calls
  (c)  cycle_drawn: the whole block in one C call
and with the heading not observed the pair that shows what giving up the riding predict costs:
  (d)  5 x predict, then observation_step_drawn (the sixth predict rides in its proposal kernel)
  (e)  cycle_drawn with use_heading off (the run does all six predicts, the proposal none)
One process; the paths are alternated `--rounds` times in batches of `--batch` blocks, every batch from the same particle
set (restored, untimed, before it).  Per batch: device events on the handle's own stream around the whole batch and a
host clock around the same blocks ending in the event's synchronise.  Medians and every run are printed, and one JSON
line at the end.  No time is fixed in advance.
Usage (GPU box): python tools/pf_cycle_timing.py [--batch 50] [--rounds 7] [--config 512x1000] [--config 8192x16]"""
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
PATHS = ("a", "b", "c", "d", "e")


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

    def scan(self, c, Z, idf):
        sh, w = self.sh, self.w
        sh.sample_proposal_drawn(Z, idf, w.RE, c)
        sh.feature_update(Z, idf, w.RE)
        sh.resample_local_drawn(c, self.Np + 1, True, want_result=False)

    def block(self, which, c):
        sh, w, Np = self.sh, self.w, self.Np
        v, swa, phi, Z, idf = self.blocks[c]
        if which == "a":
            for j in range(K):
                sh.predict(v[j], swa[j], w.QE, w.wb, w.dt)
                sh.observe_heading(phi[j], True)
            self.scan(c, Z, idf)
        elif which == "b":
            sh.control_run(v, swa, w.QE, w.wb, w.dt, phi=phi, use_heading=True)
            self.scan(c, Z, idf)
        elif which == "c":
            sh.cycle_drawn(v, swa, w.QE, w.wb, w.dt, Z, idf, self.none, w.RE, c, Np + 1, True, phi=phi, use_heading=True)
        elif which == "d":
            for j in range(K - 1):
                sh.predict(v[j], swa[j], w.QE, w.wb, w.dt)
            sh.observation_step_drawn(v[K - 1], swa[K - 1], w.QE, w.wb, w.dt, Z, idf, w.RE, c, Np + 1, True)
        else:
            sh.cycle_drawn(v, swa, w.QE, w.wb, w.dt, Z, idf, self.none, w.RE, c, Np + 1, True)

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
        # a live filter that did what was asked: finite weights, and the paths that run the same filter (a, b, c with the
        # heading; d, e without) end with the same best particle, bit for bit
        wts = sh.get_weights()
        best = sh.best_particle()
        end = (wts.tobytes(), best.Xv.tobytes(), best.Pv.tobytes())
        family = ("heading" if which in "abc" else "plain", blocks)
        self.alive = self.alive and bool(np.all(np.isfinite(wts))) and self.ends.setdefault(family, end) == end
        return dev, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--config", action="append", help="particles x features, e.g. 512x1000 (may be repeated)")
    args = ap.parse_args()
    if _capi.device_count() == 0:
        raise SystemExit("pf_cycle_timing: no HIP device (there is nothing to time without one)")
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
        beats = {}
        for new, old in (("c", "a"), ("b", "a"), ("e", "d")):
            beats[f"{new}_beats_every_{old}"] = bool(max(host[new]) < min(host[old]) and max(dev[new]) < min(dev[old]))
            print(f"  every run of ({new}) beats every run of ({old}), by both clocks: "
                  f"{'yes' if beats[f'{new}_beats_every_{old}'] else 'NO'}")
        print(f"  finite weights in every batch, and the same best particle at the end of (a), (b), (c) and of (d), (e): "
              f"{'yes' if b.alive else 'NO'}")
        out[f"{Np}x{Nf}"] = dict(device_us=dev, host_us=host, alive=bool(b.alive), **beats)
        b.sh.close()
    print(json.dumps({"tool": "pf_cycle_timing", "batch": args.batch, "rounds": args.rounds, "k": K, "us_per_block": out}))


if __name__ == "__main__":
    main()
