#!/usr/bin/env python3
"""Time of ParticleShard.associate (cslam_pf_associate: scan + merge + resolve + summary and its one staged copy) on the
particle set of bench.py's FastSLAM-2 workload, next to cslam_pf_observation_step at the same size in the same process.

Every timed associate call gets observations that differ from the previous call's, as in a running filter, so each pays
its staged host-to-device copy (as every observation_step does).
Device events on the shard's own stream (torch.cuda.ExternalStream over cslam_pf_get_stream), after a warm-up:
  us_per_call     events around a batch of --batch back-to-back calls, divided by the batch; median over --reps batches
                  (the stream stays busy: what a driver that queues steps sees)
  us_single_call  events around ONE call; median over --reps calls (includes the host's enqueue gaps between the copy and
                  the four launches)
  host_enqueue_us_per_call  a host clock around the same batch's calls alone (they return before the device finishes)
and from them pairs/s (np * nf * m innovations per call) and the achieved rate on the bytes the scan must read,
np * nf * 6 * sizeof(T) * ceil(m / obs_chunk) (every chunk of observations streams the whole map once).
One JSON line per shape.  For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/...`.

    python tools/pf_assoc_probe.py [--shapes 512x1000x32xf32,512x1000x8xf32,512x1000x32xf64] [--reps 50] [--batch 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from conan_slam_amd import _capi  # noqa: E402
from conan_slam_amd.pf import ParticleShard, stratified_random  # noqa: E402
from conan_slam_amd.synth import Workload, normal, uniform01  # noqa: E402

GATES = (4.0, 25.0)


def _fill(sh, w, npart, dtype):
    """bench.py's particle set: map estimate = truth + N(0, 1), PF = I, poses at the origin with a small covariance."""
    nf = w.N
    XF = np.asfortranarray(np.stack([w.X0[3::2], w.X0[4::2]]).astype(dtype))
    PF = np.asfortranarray(np.tile(np.array([1, 0, 0, 1], dtype=dtype)[:, None], (1, nf)))
    Pv = np.diag([0.05, 0.05, 1e-4]).astype(dtype)
    for i in range(npart):
        pose = np.array([0.05 * normal(77, 3 * i), 0.05 * normal(77, 3 * i + 1), 0.002 * normal(77, 3 * i + 2)], dtype=dtype)
        sh.set_particle(i, 1.0 / npart, pose, Pv, XF, PF)


def _timed(torch, stream, fn, reps, batch, warmup=5):
    for _ in range(warmup):
        fn()
    stream.synchronize()
    out, host = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        for _ in range(batch):
            fn()
        host.append((time.perf_counter() - t0) * 1e6 / batch)   # the host's share: the calls return before the device ends
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / batch)
    _timed.host_us = float(np.median(host))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def case(npart, nf, m, dtype, reps, batch):
    import torch

    dtype = np.dtype(dtype).type
    w = Workload(nf, m, dtype, seed=0, build_p=False)
    sh = ParticleShard(npart, nf, dtype=dtype)
    _fill(sh, w, npart, dtype)
    stream = torch.cuda.ExternalStream(sh.stream_ptr())
    Z, idf = w.observations(0)
    R = w.RE
    # A filter sees new observations every step, and a call whose Z is byte-identical to the last one staged skips its
    # host-to-device copy.  So every timed call gets its own Z: step 0's scan with 1e-3 (m, rad) of jitter, 64 variants
    # in rotation (the association itself does not change: the jitter is a thousandth of a sigma).
    jit = np.random.default_rng(1)
    Zs = [np.asfortranarray((Z.astype(np.float64) + 1e-3 * jit.normal(size=Z.shape)).astype(dtype)) for _ in range(64)]
    calls = [0]

    def assoc():
        sh.associate(Zs[calls[0] % len(Zs)], R, *GATES)
        calls[0] += 1

    a_med, a_min, a_max = _timed(torch, stream, assoc, reps, batch)
    a_host = _timed.host_us
    s_med, _, _ = _timed(torch, stream, assoc, reps, 1)
    sh.associate(Z, R, *GATES)
    idf_t, kind, summary = sh.association()
    pairs = npart * nf * m
    chunks = -(-m // _capi.PF_ASSOC_OBS_CHUNK)
    must_read = npart * nf * 6 * np.dtype(dtype).itemsize * chunks
    out = {"workload": "pf_associate", "particles": npart, "features": nf, "m": m, "dtype": np.dtype(dtype).name,
           "reps": reps, "batch": batch,
           "associate_us_per_call": round(a_med, 2), "associate_us_min": round(a_min, 2), "associate_us_max": round(a_max, 2),
           "associate_us_single_call": round(s_med, 2), "associate_host_enqueue_us_per_call": round(a_host, 2),
           "pairs_per_call": pairs, "pairs_per_s": round(pairs / (a_med * 1e-6), 0),
           "bytes_scan_must_read": must_read, "scan_read_GBps": round(must_read / (a_med * 1e-6) / 1e9, 1),
           "matched_fraction": round(float((kind == 1).mean()), 4),
           "table_agrees_with_known_idf": round(float((idf_t == np.asarray(idf)[:, None]).mean()), 4)}
    # the yardstick: the known-association step at the same size, bench.py's loop (state evolves step by step)
    steps = 5 + reps * batch + reps
    inputs = []
    for t in range(steps):
        Zt, idft = w.observations(t)
        nrm = normal(500 + t, np.arange(3 * npart, dtype=np.uint64)).reshape(3, npart).astype(dtype)
        inputs.append((w.controls(t), Zt, idft, np.ascontiguousarray(nrm),
                       stratified_random(npart, uniform01(900 + t, np.arange(npart, dtype=np.uint64)), dtype)))
    it = iter(inputs)

    def step():
        (v, swa), Zt, idft, nrm, sel = next(it)
        sh.observation_step(v, swa, w.QE, w.wb, w.dt, Zt, idft, R, nrm, sel, int(0.75 * npart), True)

    o_med, _, _ = _timed(torch, stream, step, reps, batch)
    out["observation_step_host_enqueue_us_per_call"] = round(_timed.host_us, 2)
    o_single, _, _ = _timed(torch, stream, step, reps, 1, warmup=0)
    out["observation_step_us_per_call"] = round(o_med, 2)
    out["observation_step_us_single_call"] = round(o_single, 2)
    out["associate_over_step"] = round(a_med / o_med, 2)
    sh.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x1000x32xf32,512x1000x8xf32,512x1000x32xf64")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=10)
    args = ap.parse_args()
    if _capi.device_count() == 0:
        raise SystemExit("pf_assoc_probe: no HIP device (there is nothing to time without one)")
    for shape in args.shapes.split(","):
        npart, nf, m, dt = shape.split("x")
        print(json.dumps(case(int(npart), int(nf), int(m), {"f32": np.float32, "f64": np.float64}[dt], args.reps, args.batch)),
              flush=True)


if __name__ == "__main__":
    main()
