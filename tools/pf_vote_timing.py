#!/usr/bin/env python3
"""What the vote on new features kept on the device buys one FastSLAM-2 scan with unknown correspondences (m = 8, f32,
resample forced on every scan).

Every scan observes seven mapped landmarks and one far from all of them, which the vote declares new, so each scan adds
at least one feature (the store has room for all eight; how many a batch added is printed, and must be the same for
every path: they run the same filter on the same draws).  Four ways to run the same scan, each behind a predict:
  (a)  the host-policy sequence of tests/test_pf_drive_gpu.py::test_unknown_correspondences: pf.data_associate (associate,
       synchronise, summary to the host, numpy vote), sample_proposal_assoc_drawn(use), resample_local_drawn with its
       result read back, add_features(ZN)
  (a') the same without reading the resample's result (the one round trip left is the vote's)
  (b)  the separate voted calls: associate_vote, sample_proposal_voted_drawn, resample_local_drawn(want_result=False),
       add_features_voted
  (c)  assoc_scan_step_drawn: the same in one C call
One process; the paths are alternated `--rounds` times in batches of `--batch` scans, every batch from the same particle
set (restored, untimed, before it).  Per batch: device events on the handle's own stream around the whole batch (the
stream's idle gaps while the host decides are inside them) and a host clock around the same scans ending in the event's
synchronise.  Medians and every run are printed, and one JSON line at the end.  No time is fixed in advance.
Usage (GPU box): python tools/pf_vote_timing.py [--batch 50] [--rounds 7] [--config 512x1000] [--config 8192x16]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conan_slam_amd import _capi, pf  # noqa: E402
from conan_slam_amd.pf import ParticleShard  # noqa: E402
from conan_slam_amd.synth import Workload  # noqa: E402

dtype = np.float32
M_OBS = 8
GATES = (4.0, 25.0)
NEW_FRACTION, MISS = 0.5, 0.01
PATHS = ("a", "a'", "b", "c")


class Bench:
    def __init__(self, Np, Nf, batch):
        import torch

        self.torch, self.Np, self.Nf, self.batch = torch, Np, Nf, batch
        self.w = Workload(Nf, M_OBS - 1, dtype, seed=0, build_p=False)
        self.ctl = [self.w.controls(t) for t in range(batch)]
        self.Z = []
        for t in range(batch):  # seven mapped landmarks and one 2 km out: new for every particle
            Zk, _ = self.w.observations(t)
            far = np.array([[2000.0 + 25.0 * t], [0.3]], dtype)
            self.Z.append(np.asfortranarray(np.concatenate([np.asarray(Zk, dtype).reshape(2, -1, order="F"), far], axis=1)))
        self.sh = ParticleShard(Np, Nf + batch * M_OBS, dtype=dtype, n_global=Np)
        self.sh.seed_draws(12345)
        self.stream = torch.cuda.ExternalStream(self.sh.stream_ptr())
        XF = np.asfortranarray(np.stack([self.w.X0[3::2], self.w.X0[4::2]]).astype(dtype))
        PF = np.asfortranarray(np.tile(np.array([1, 0, 0, 1], dtype=dtype)[:, None], (1, Nf)))
        Pv = np.diag([0.05, 0.05, 1e-4]).astype(dtype)
        self.first = (1.0 / Np, np.zeros(3, dtype), Pv, XF, PF)
        self.alive, self.added = True, {}

    def reset(self):
        """Every batch starts from the same set: the initial particle (Nf features), gathered into every slot."""
        self.sh.set_particle(0, *self.first)
        self.sh.gather_local(np.zeros(self.Np, np.int32), 1.0 / self.Np)

    def scan(self, which, t):
        sh, w, Np, Z = self.sh, self.w, self.Np, self.Z[t]
        v, swa = self.ctl[t]
        if which == "c":
            return sh.assoc_scan_step_drawn(v, swa, w.QE, w.wb, w.dt, Z, w.RE, *GATES, t, Np + 1, True, NEW_FRACTION, MISS)
        sh.predict(v, swa, w.QE, w.wb, w.dt)
        if which == "b":
            sh.associate_vote(Z, w.RE, *GATES, NEW_FRACTION)
            sh.sample_proposal_voted_drawn(Z, w.RE, t, MISS)
            sh.resample_local_drawn(t, Np + 1, True, want_result=False)
            return sh.add_features_voted(w.RE)
        use, ZN = pf.data_associate(sh, Z, w.RE, *GATES, NEW_FRACTION)
        sh.sample_proposal_assoc_drawn(Z, w.RE, t, use, MISS)
        sh.resample_local_drawn(t, Np + 1, True, want_result=(which == "a"))
        if ZN.shape[1]:
            sh.add_features(ZN, w.RE)
        return ZN.shape[1]

    def run(self, which, scans=None):
        """-> (us per scan by device events, us per scan by the host clock)"""
        torch, sh = self.torch, self.sh
        scans = self.batch if scans is None else scans
        self.reset()
        sh.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        t0 = time.perf_counter()
        added = sum(self.scan(which, t) for t in range(scans))
        e1.record(self.stream)
        e1.synchronize()
        host = (time.perf_counter() - t0) * 1e6 / scans
        dev = e0.elapsed_time(e1) * 1e3 / scans
        # a live filter that did what was asked: at least the far observation of every scan added, the same count on
        # every path, finite weights
        self.alive = self.alive and added >= scans and sh.n_features == self.Nf + added
        self.alive = self.alive and self.added.setdefault(scans, added) == added
        self.alive = self.alive and bool(np.all(np.isfinite(sh.get_weights())))
        return dev, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--config", action="append", help="particles x features, e.g. 512x1000 (may be repeated)")
    args = ap.parse_args()
    if _capi.device_count() == 0:
        raise SystemExit("pf_vote_timing: no HIP device (there is nothing to time without one)")
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
        print(f"{Np} x {Nf}, m = {M_OBS}, f32, {args.batch} scans per batch, {args.rounds} rounds (us per scan)")
        for name, res in (("device events", dev), ("host clock   ", host)):
            for k in PATHS:
                v = res[k]
                print(f"  {name} ({k:2s}) median {np.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}   runs " +
                      " ".join(f"{x:.2f}" for x in v))
        every = max(host["c"]) < min(min(host["a"]), min(host["a'"])) and max(dev["c"]) < min(min(dev["a"]), min(dev["a'"]))
        print(f"  every run of (c) beats every run of (a) and (a'), by both clocks: {'yes' if every else 'NO'}")
        print(f"  features added per batch: {b.added.get(args.batch)}; the same on every path, finite weights in every batch: "
              f"{'yes' if b.alive else 'NO'}")
        out[f"{Np}x{Nf}"] = {"device_us": dev, "host_us": host, "c_beats_every_a": bool(every), "alive": bool(b.alive),
                              "features_added_per_batch": b.added.get(args.batch)}
        b.sh.close()
    print(json.dumps({"tool": "pf_vote_timing", "batch": args.batch, "rounds": args.rounds, "us_per_scan": out}))


if __name__ == "__main__":
    main()
