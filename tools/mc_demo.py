#!/usr/bin/env python3
"""A Monte-Carlo study of the bundled demo (test/main.cpp:24-200, the map in tests/golden/demo_map.json) through the
batched engine: I seeded noisy runs (control noise slam.h:149-159, sensor noise slam.h:168-178, the counter-based
generator of conan_slam_amd/synth.py) share one true trajectory, hence the visible tags, the table association, m and
the new features at every step; only the numbers differ.

The calls of every run are taken from the harness (oracle/sim_driver.run_demo with a recording back-end: the truth,
the sensor and the association table are test-side helpers, not product code), then driven two ways:
  batch    one EKFBatch(I, n_landmarks=0, max_landmarks=64): predict_each / observe_heading / update_device /
           augment_device, one launch per stage for all instances;
  handles  I EKF handles, one host thread each (as tools/mc_loop.py).
Prints one JSON line: control steps per second of each driver (a step advances every instance by one control step),
and per instance the pose RMSE and mean NEES against the truth at the observation steps, from EKFBatch.poses(), and the
map RMSE and mean landmark NEES (e^T P_jj^-1 e per landmark, averaged over landmarks and steps) from
EKFBatch.landmarks(), which reads without applying the pending covariance downdate: scoring does not perturb the runs.
The true landmark of each state feature is the demo map's landmark the association table gave it.

--generator device needs none of the recorded filter runs for its inputs: the truth (poses, steering, observation
steps) still comes from the harness helpers, the noisy controls from synth.control_noise, the scans from one
BatchSimulator for all instances, consumed with EKFBatch.update_scan / augment_scan.  --placement says when the scan of
an observation step is made: `late` right before it is consumed, `early` right after the previous scan was consumed
(the table depends only on the sequence of scans), while that window is still running.

--score says who scores.  `host` (the default): the separate accuracy pass described above, poses() and landmarks() after
every observation step and numpy on the host.  `device`: EKFBatch.score (tape) / score_scan (generator) at the same
points INSIDE a timed pass -- the totals and the series stay on the device until the pass ends -- and the same four
summary keys from them (pose_rmse_m, mean_nees, map_rmse_m from the totals; mean_landmark_nees keeps its meaning, the
mean over observation steps of the step's mean, from the series; pooled_landmark_nees is LM_NEES / LM_N), plus the
fraction inside each 95 % gate and per observation step the run-averaged pose NEES.  `both`: both, with the largest
relative difference of the four numbers between them (the host scorer is then given the f32 truth the device holds).
scored_steps_per_s is the rate of the pass that scores, for either scorer.

    python tools/mc_demo.py [--instances 8] [--steps 2400] [--seed 1000] [--quirks textbook|ref_exact]
                            [--generator tape|device] [--placement late|early|both] [--score host|device|both]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from conan_slam_amd import EKF, EKFBatch, Q_REF_EXACT, Q_TEXTBOOK  # noqa: E402


class Recorder:
    """run_demo back-end: forwards to the f32 CPU oracle (which supplies n for the association) and keeps every call."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    @property
    def n(self):
        return self.inner.n

    def predict(self, v, swa, Q, wb, dt):
        self.calls.append(("P", float(v), float(swa), np.array(Q, np.float32), float(wb), float(dt)))
        self.inner.predict(v, swa, Q, wb, dt)

    def observe_heading(self, phi, use):
        self.calls.append(("H", float(phi), bool(use)))
        self.inner.observe_heading(phi, use)

    def update(self, Z, R, idf, batch):
        if Z.size and Z.shape[1]:
            self.calls.append(("U", np.array(Z, np.float32, order="F"), np.array(idf, np.int32), np.array(R, np.float32)))
        return self.inner.update(Z, R, idf, batch)

    def augment(self, Z, R):
        if Z.size and Z.shape[1]:
            self.calls.append(("A", np.array(Z, np.float32, order="F"), np.array(R, np.float32)))
        self.inner.augment(Z, R)

    def get_x(self):
        return self.inner.get_x()

    def get_p(self):
        return self.inner.get_p()


def truth_poses(LM, WP, steps):
    """The true pose after every control step: run_demo's vehicle and steering, through the same harness helpers."""
    from pyoracle import Oracle
    from sim_driver import SlamConfig

    cfg = SlamConfig()
    sim = Oracle(np.float32)
    f = np.float32
    XTrue = np.zeros(3, dtype=np.float32)
    WPd = WP.astype(np.float32, order="F")
    iwp, swa, loops, out = 1, f(0.0), float(cfg.number_loops), []
    while 0 < iwp <= WP.shape[1] and len(out) < steps:
        iwp, swa = sim.compute_swa(XTrue, WPd, iwp, cfg.at_waypoint, swa, cfg.rate_swa, cfg.max_swa, f(cfg.dt_controls), True)
        if iwp == 0 and loops > 1:
            iwp, loops = 1, loops - 1
        sim.vehicle_model(XTrue, cfg.velocity, swa, cfg.wheel_base, f(cfg.dt_controls))
        out.append(XTrue.astype(np.float64).copy())
    return out


class _MapTable:
    """run_demo back-end without a filter, noise off: the demo map landmark behind every state feature, in augment
    order (the table association appends new features in the order data_associate_table returns them)."""

    def __init__(self, LM, truth):
        self.LM, self.truth, self.step, self.nf, self.lm = LM, truth, 0, 0, []

    @property
    def n(self):
        return 3 + 2 * self.nf

    def predict(self, *a):
        self.step += 1

    def observe_heading(self, *a):
        pass

    def update(self, *a):
        return 0

    def augment(self, Z, R):
        x = self.truth[self.step - 1]
        for c in range(Z.shape[1] if Z.size else 0):
            r, b = float(Z[0, c]), float(Z[1, c])
            p = np.array([x[0] + r * np.cos(b + x[2]), x[1] + r * np.sin(b + x[2])])
            d = np.hypot(self.LM[0] - p[0], self.LM[1] - p[1])
            assert d.min() < 1e-2 * r + 1e-3, "a noise-free observation must land on its landmark"
            self.lm.append(int(np.argmin(d)))
            self.nf += 1

    def get_x(self):
        return np.zeros(self.n, np.float32)

    def get_p(self):
        return np.zeros((self.n, self.n), np.float32)


def map_truth(steps):
    """[N, 2]: the true position of state feature j + 1, from a noise-free run of the same demo."""
    from sim_driver import load_demo_map, run_demo

    LM, WP = load_demo_map()
    t = _MapTable(LM.astype(np.float64), truth_poses(LM, WP, steps))
    run_demo(t, LM, WP, noise_seed=None, max_steps=steps)
    return LM.astype(np.float64)[:, t.lm].T


def record(I, seed, steps, quirks):
    from sim_driver import OracleBackend, load_demo_map, run_demo

    LM, WP = load_demo_map()
    recs = []
    for i in range(I):
        r = Recorder(OracleBackend(np.float32, quirks))
        run_demo(r, LM, WP, noise_seed=seed + i, max_steps=steps)
        recs.append(r.calls)
    for rec in recs[1:]:
        assert [c[0] for c in rec] == [c[0] for c in recs[0]], "the runs must share their call structure"
    return recs, truth_poses(LM, WP, steps)


def pack(recs):
    import torch

    zs = [np.concatenate([c[1].reshape(-1, order="F") for c in rec if c[0] in "UA"] + [np.zeros(1, np.float32)])
          for rec in recs]
    ids = np.concatenate([c[2] for c in recs[0] if c[0] == "U"] + [np.zeros(1, np.int32)])
    return ([torch.from_numpy(np.ascontiguousarray(z)).cuda() for z in zs],
            torch.from_numpy(np.ascontiguousarray(ids)).cuda())


class HostScorer:
    """score(step, b) on the host: pose error and NEES from poses(), map error and landmark NEES from landmarks()."""

    def __init__(self, I, truth, lm_true):
        self.I, self.truth, self.lm_true = I, truth, lm_true
        self.err2, self.nees = [[] for _ in range(I)], [[] for _ in range(I)]
        self.merr2, self.mnees = [[] for _ in range(I)], [[] for _ in range(I)]

    def __call__(self, step, b):
        I = self.I
        x, pvv = b.poses()
        xt = self.truth[step - 1]
        for i in range(I):
            e = x[i].astype(np.float64) - xt
            e[2] = (e[2] + np.pi) % (2 * np.pi) - np.pi
            self.err2[i].append(float(e[0] ** 2 + e[1] ** 2))
            try:
                self.nees[i].append(float(e @ np.linalg.solve(pvv[i].astype(np.float64), e)))
            except np.linalg.LinAlgError:
                self.nees[i].append(float("nan"))
        xl, pll, _ = b.landmarks()
        e = xl.astype(np.float64) - self.lm_true[None, : xl.shape[1]]
        for i in range(I):
            self.merr2[i].extend((e[i] ** 2).sum(axis=1).tolist())
            try:
                self.mnees[i].append(float(np.mean(np.einsum("ja,ja->j", e[i], np.linalg.solve(
                    pll[i].astype(np.float64), e[i][:, :, None])[:, :, 0]))))
            except np.linalg.LinAlgError:
                self.mnees[i].append(float("nan"))

    def summary(self):
        return {"pose_rmse_m": [float(np.sqrt(np.mean(e))) for e in self.err2],
                "mean_nees": [float(np.nanmean(v)) for v in self.nees],
                "map_rmse_m": [float(np.sqrt(np.mean(e))) for e in self.merr2],
                "mean_landmark_nees": [float(np.nanmean(v)) for v in self.mnees]}


SUMMARY_DIGITS = {"pose_rmse_m": 4, "mean_nees": 3, "map_rmse_m": 4, "mean_landmark_nees": 3}


def rounded(summary):
    return {k: [round(v, SUMMARY_DIGITS[k]) for v in summary[k]] for k in SUMMARY_DIGITS}


def device_summary(totals, series):
    """The four summary keys and the consistency figures from EKFBatch.scores()."""
    from conan_slam_amd import _capi as c

    with np.errstate(invalid="ignore", divide="ignore"):
        T = totals
        four = {"pose_rmse_m": np.sqrt(T[:, c.SCORE_POSE_ERR2] / T[:, c.SCORE_POSE_N]).tolist(),
                "mean_nees": (T[:, c.SCORE_POSE_NEES] / T[:, c.SCORE_POSE_N]).tolist(),
                "map_rmse_m": np.sqrt(T[:, c.SCORE_LM_ERR2] / T[:, c.SCORE_LM_N]).tolist(),
                "mean_landmark_nees": np.nanmean(series[:, :, 3].astype(np.float64), axis=0).tolist()}
        more = {"pooled_landmark_nees": [round(float(v), 3) for v in T[:, c.SCORE_LM_NEES] / T[:, c.SCORE_LM_N]],
                "pose_in_gate": [round(float(v), 4) for v in T[:, c.SCORE_POSE_IN] / T[:, c.SCORE_POSE_N]],
                "landmark_in_gate": [round(float(v), 4) for v in T[:, c.SCORE_LM_IN] / T[:, c.SCORE_LM_N]],
                "bad_blocks": [int(v) for v in T[:, c.SCORE_POSE_BAD] + T[:, c.SCORE_LM_BAD]],
                "pose_nees_by_step": [round(float(v), 3) for v in np.nanmean(series[:, :, 1].astype(np.float64), axis=1)]}
    return four, more


def max_rel_diff(dev, host):
    return {k: float(max(abs(d - h) / abs(h) for d, h in zip(dev[k], host[k]))) for k in SUMMARY_DIGITS}


def drive_batch(b, recs, dz, di, score=None):
    """The recorded calls through one EKFBatch.  score(step, b): called after every observation step."""
    I = len(recs)
    zo = io = step = 0
    for k, c in enumerate(recs[0]):
        if c[0] == "P":
            b.predict_each([r[k][1] for r in recs], [r[k][2] for r in recs], c[3], c[4], c[5])
            step += 1
        elif c[0] == "H":
            b.observe_heading(c[1], c[2])
        elif c[0] == "U":
            m = c[1].shape[1]
            b.update_device([t.data_ptr() + 4 * zo for t in dz], [di.data_ptr() + 4 * io] * I, m, c[3])
            zo, io = zo + 2 * m, io + m
        else:
            q = c[1].shape[1]
            b.augment_device([t.data_ptr() + 4 * zo for t in dz], q, c[2])
            zo += 2 * q
            if score is not None:
                score(step, b)
    b.synchronize()


def truth_script(LM, WP, steps):
    """Per control step (true pose f32, steering angle, observes?): run_demo's truth side through the harness helpers."""
    from pyoracle import Oracle
    from sim_driver import SlamConfig

    cfg = SlamConfig()
    sim = Oracle(np.float32)
    f = np.float32
    XTrue = np.zeros(3, dtype=np.float32)
    WPd = WP.astype(np.float32, order="F")
    dt = cfg.dt_controls
    iwp, swa, loops, dtsum, out = 1, f(0.0), float(cfg.number_loops), 0.0, []
    while 0 < iwp <= WP.shape[1] and len(out) < steps:
        iwp, swa = sim.compute_swa(XTrue, WPd, iwp, cfg.at_waypoint, swa, cfg.rate_swa, cfg.max_swa, f(dt), True)
        if iwp == 0 and loops > 1:
            iwp, loops = 1, loops - 1
        sim.vehicle_model(XTrue, cfg.velocity, swa, cfg.wheel_base, f(dt))
        dtsum += dt
        observe = dtsum >= cfg.dt_observe
        if observe:
            dtsum = 0.0
        out.append((XTrue.copy(), f(swa), observe))
    return cfg, out


def drive_device(b, gen, cfg, script, vn, swan, QE, R, RE, early=False, score=None):
    """The demo loop with device-generated scans: predict_each / observe_heading per control step, scan -> update_scan ->
    augment_scan per observation step.  early: the scan of the NEXT observation step is made right after this one's was
    consumed.  Returns (observation steps, updates, largest scan)."""
    wb, dt, rmax = float(cfg.wheel_base), float(np.float32(cfg.dt_controls)), float(cfg.max_range)
    obs = [k for k, s in enumerate(script) if s[2]]
    nxt = {a: c for a, c in zip(obs, obs[1:])}
    made = None
    n_obs = updates = max_m = 0
    for k, (xv, swa, observe) in enumerate(script):
        b.predict_each(vn[k], swan[k], QE, wb, dt)
        b.observe_heading(float(xv[2]), True)
        if not observe:
            continue
        m, mf, mn = made if made is not None else gen.scan(xv, rmax, R, k + 1)
        made = None
        b.update_scan(gen, RE)
        b.augment_scan(gen, RE)
        n_obs, updates, max_m = n_obs + 1, updates + (mf > 0), max(max_m, mf)
        if score is not None and mn:
            score(k + 1, b)
        if early and k in nxt:
            made = gen.scan(script[nxt[k]][0], rmax, R, nxt[k] + 1)
    b.synchronize()
    return n_obs, updates, max_m


def drive_handles(hs, recs, dz, di):
    """Instance i's calls through handle i, one host thread per handle (the calls release the GIL)."""

    def one(i):
        h, rec, zo, io = hs[i], recs[i], 0, 0
        for c in rec:
            if c[0] == "P":
                h.predict(c[1], c[2], c[3], c[4], c[5])
            elif c[0] == "H":
                h.observe_heading(c[1], c[2])
            elif c[0] == "U":
                m = c[1].shape[1]
                h.update_device(dz[i].data_ptr() + 4 * zo, m, c[3], di.data_ptr() + 4 * io, batch=True)
                zo, io = zo + 2 * m, io + m
            else:
                q = c[1].shape[1]
                h.augment(c[1], c[2])
                zo += 2 * q
        h.synchronize()

    ts = [threading.Thread(target=one, args=(i,)) for i in range(len(hs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8)
    ap.add_argument("--steps", type=int, default=2400)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--quirks", choices=["textbook", "ref_exact"], default="textbook")
    ap.add_argument("--generator", choices=["tape", "device"], default="tape")
    ap.add_argument("--placement", choices=["late", "early", "both"], default="both")
    ap.add_argument("--score", choices=["host", "device", "both"], default="host")
    args = ap.parse_args()
    quirks = Q_TEXTBOOK if args.quirks == "textbook" else Q_REF_EXACT
    I = args.instances
    if args.generator == "device":
        return main_device(args, quirks)
    recs, truth = record(I, args.seed, args.steps, quirks)
    steps = sum(1 for c in recs[0] if c[0] == "P")
    dz, di = pack(recs)

    # batch: one untimed pass (code objects, allocations), then the timed pass
    for timed in (False, True):
        b = EKFBatch(I, n_landmarks=0, max_landmarks=64, quirks=quirks)
        t0 = time.perf_counter()
        drive_batch(b, recs, dz, di)
        t_batch = time.perf_counter() - t0
        flags = b.factor_status()
        b.close()
    for timed in (False, True):
        hs = [EKF(64, dtype=np.float32, quirks=quirks) for _ in range(I)]
        t0 = time.perf_counter()
        drive_handles(hs, recs, dz, di)
        t_handles = time.perf_counter() - t0
        for h in hs:
            h.close()

    # accuracy: pose error and NEES at every observation step, map error and landmark NEES of the features seen so far
    # (truth through the association table)
    lm_true = map_truth(args.steps)
    out, dev, host = {}, None, None
    if args.score in ("device", "both"):
        lm32 = lm_true.astype(np.float32)
        n_calls = sum(1 for c in recs[0] if c[0] == "A")
        for timed in (False, True):
            b = EKFBatch(I, n_landmarks=0, max_landmarks=64, quirks=quirks)
            b.score_reset(n_calls)
            b.score_set_truth(lm32)
            t0 = time.perf_counter()
            drive_batch(b, recs, dz, di, lambda step, b: b.score(truth[step - 1]))
            t_scored = time.perf_counter() - t0
            totals, series, _ = b.scores()
            b.close()
        dev, more = device_summary(totals, series)
        out.update(more)
        if args.score == "both":
            lm_true = lm32.astype(np.float64)
    if args.score in ("host", "both"):
        score = HostScorer(I, truth, lm_true)
        b = EKFBatch(I, n_landmarks=0, max_landmarks=64, quirks=quirks)
        t0 = time.perf_counter()
        drive_batch(b, recs, dz, di, score)
        t_host = time.perf_counter() - t0
        b.close()
        host = score.summary()
    if args.score == "both":
        out["host_scored_steps_per_s"] = round(steps / t_host, 1)
        out["host_summary"] = rounded(host)
        out["score_max_rel_diff"] = max_rel_diff(dev, host)
    out["scored_steps_per_s"] = round(steps / (t_host if args.score == "host" else t_scored), 1)
    print(json.dumps({
        "workload": "mc_demo", "generator": "tape", "instances": I, "steps": steps, "quirks": args.quirks,
        "updates": sum(1 for c in recs[0] if c[0] == "U"),
        "max_m": max((c[1].shape[1] for c in recs[0] if c[0] == "U"), default=0),
        "batch_steps_per_s": round(steps / t_batch, 1),
        "handles_steps_per_s": round(steps / t_handles, 1),
        "speedup": round(t_handles / t_batch, 3),
        **rounded(host if args.score == "host" else dev),
        "factor_status": flags, "score": args.score, **out,
    }))


def main_device(args, quirks):
    from sim_driver import load_demo_map

    from conan_slam_amd import BatchSimulator
    from conan_slam_amd.synth import control_noise, noise_matrices

    I = args.instances
    seeds = [args.seed + i for i in range(I)]
    LM, WP = load_demo_map()
    cfg, script = truth_script(LM, WP, args.steps)
    steps = len(script)
    Q, R, QE, RE = noise_matrices(np.float32)
    vn, swan = control_noise(seeds, np.arange(1, steps + 1), cfg.velocity, np.array([s[1] for s in script], np.float32), Q)
    vn, swan = vn.astype(np.float64), swan.astype(np.float64)

    truth = [s[0].astype(np.float64) for s in script]
    scores = {}

    def run(early, score=None, device_score=False):
        gen = BatchSimulator(LM, I, seeds)
        b = EKFBatch(I, n_landmarks=0, max_landmarks=64, quirks=quirks)
        if device_score:
            b.score_reset(sum(1 for s in script if s[2]))
            score = lambda step, b: b.score_scan(gen, truth[step - 1])  # noqa: E731
        t0 = time.perf_counter()
        counts = drive_device(b, gen, cfg, script, vn, swan, QE, R, RE, early, score)
        t = time.perf_counter() - t0
        if device_score:
            scores["device"] = b.scores()
        flags = b.factor_status()
        b.close()
        gen.close()
        return t, counts, flags

    # one untimed pass (code objects, allocations), then the timed passes, alternated
    run(False)
    times = {"late": [], "early": []}
    for _ in range(3):
        for p in (("late", "early") if args.placement == "both" else (args.placement,)):
            t, counts, flags = run(p == "early")
            times[p].append(t)
    best = {p: min(v) for p, v in times.items() if v}
    place = min(best, key=best.get)

    lm_true = map_truth(args.steps)
    out, dev, host = {}, None, None
    if args.score in ("device", "both"):
        run(place == "early", device_score=True)  # (untimed: the score kernels' code objects and buffers)
        t_scored, counts, flags = run(place == "early", device_score=True)
        dev, more = device_summary(scores["device"][0], scores["device"][1])
        out.update(more)
        if args.score == "both":
            lm_true = lm_true.astype(np.float32).astype(np.float64)
    if args.score in ("host", "both"):
        score = HostScorer(I, truth, lm_true)
        t_host, counts, flags = run(place == "early", score)
        host = score.summary()
    if args.score == "both":
        out["host_scored_steps_per_s"] = round(steps / t_host, 1)
        out["host_summary"] = rounded(host)
        out["score_max_rel_diff"] = max_rel_diff(dev, host)
    out["scored_steps_per_s"] = round(steps / (t_host if args.score == "host" else t_scored), 1)
    print(json.dumps({
        "workload": "mc_demo", "generator": "device", "instances": I, "steps": steps, "quirks": args.quirks,
        "updates": int(counts[1]), "max_m": int(counts[2]), "scans": int(counts[0]),
        "batch_steps_per_s": round(steps / best[place], 1), "placement": place,
        "steps_per_s_by_placement": {p: round(steps / t, 1) for p, t in best.items()},
        **rounded(host if args.score == "host" else dev),
        "factor_status": flags, "score": args.score, **out,
    }))


if __name__ == "__main__":
    main()
