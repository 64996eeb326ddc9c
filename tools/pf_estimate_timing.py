#!/usr/bin/env python3
"""Wall time of the particle filter's read path (ParticleShard.estimate / best_particle / all_features) against the only
route there was before it: one get_particle per particle plus the moments in numpy (tests/pf_estimate_ref.py).  Host
clock around calls that end in their own synchronise, after a warm-up; medians over --reps.  Prints one JSON line per
shape.  For the device time of the kernels and the launch / copy counts run it under
`rocprofv3 --kernel-trace --stats -- python tools/pf_estimate_timing.py --reps 50 --skip-download`.

    python tools/pf_estimate_timing.py [--shapes 512x1000,20000x1] [--reps 50] [--download-reps 3] [--skip-download]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from conan_slam_amd.pf import ParticleShard  # noqa: E402


def _median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(ts)), 4)


def _fill(sh, npart, nf, rng):
    """A converged set around a common map, written through the packed-record upload (one copy, not np of them)."""
    import torch

    base = rng.uniform(-300, 300, size=(2, nf))
    rec = np.zeros((npart, 13 + 6 * nf), dtype=np.float32)
    rec[:, 0] = rng.uniform(0.5, 1.5, npart) / npart
    rec[:, 1:3] = rng.normal(0, 0.3, (npart, 2))
    rec[:, 3] = rng.normal(0.2, 0.006, npart)
    rec[:, 4:13] = (np.diag([0.05, 0.05, 1e-4]).reshape(-1))[None]
    rec[:, 13:13 + 2 * nf] = (base.reshape(-1, order="F")[None] + rng.normal(0, 0.3, (npart, 2 * nf)))
    rec[:, 13 + 2 * nf:] = np.tile(np.array([0.2, 0.0, 0.0, 0.2], dtype=np.float32), nf)[None]
    # the store's feature count is set by set_particle; the records then overwrite every particle
    sh.set_particle(0, rec[0, 0], rec[0, 1:4], rec[0, 4:13].reshape(3, 3, order="F"),
                    rec[0, 13:13 + 2 * nf].reshape(2, nf, order="F"), rec[0, 13 + 2 * nf:].reshape(4, nf, order="F"))
    buf = torch.from_numpy(rec).cuda()
    torch.cuda.synchronize()
    sh.unpack_from(np.arange(npart, dtype=np.int32), buf.data_ptr())
    sh.synchronize()


def case(npart, nf, reps, download_reps):
    from pf_estimate_ref import download, estimate_ref

    rng = np.random.default_rng(npart + nf)
    sh = ParticleShard(npart, nf, dtype=np.float32)
    _fill(sh, npart, nf, rng)
    out = {"particles": npart, "features": nf,
           "estimate_ms": _median_ms(lambda: sh.estimate(), reps),
           "estimate_pose_only_ms": _median_ms(lambda: sh.estimate(want_map=False), reps),
           "best_particle_ms": _median_ms(lambda: sh.best_particle(), reps),
           "all_features_ms": _median_ms(lambda: sh.all_features(), reps)}
    map_bytes = npart * (1 + 6 * nf) * 4
    out["map_bytes"] = map_bytes
    out["estimate_GBps_wall"] = round(map_bytes / (out["estimate_ms"] * 1e-3) / 1e9, 2)
    if download_reps > 0:
        est = sh.estimate()
        arrs = [None]

        def dl():
            arrs[0] = download(sh)

        out["download_all_ms"] = _median_ms(dl, download_reps, warmup=1)
        out["numpy_moments_ms"] = _median_ms(lambda: estimate_ref(*arrs[0]), download_reps, warmup=1)
        out["old_route_ms"] = round(out["download_all_ms"] + out["numpy_moments_ms"], 3)
        out["speedup_estimate"] = round(out["old_route_ms"] / out["estimate_ms"], 1)
        out["speedup_best_particle"] = round(out["download_all_ms"] / out["best_particle_ms"], 1)
        out["speedup_all_features"] = round(out["download_all_ms"] / out["all_features_ms"], 1)
        ref = estimate_ref(*arrs[0])
        out["max_abs_map_mean_diff"] = float(np.abs(est.XF.astype(np.float64) - ref.XF).max())
    sh.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x1000,20000x1")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--download-reps", type=int, default=3)
    ap.add_argument("--skip-download", action="store_true")
    args = ap.parse_args()
    for shape in args.shapes.split(","):
        npart, nf = (int(v) for v in shape.split("x"))
        print(json.dumps({"workload": "pf_estimate",
                          **case(npart, nf, args.reps, 0 if args.skip_download else args.download_reps)}), flush=True)


if __name__ == "__main__":
    main()
