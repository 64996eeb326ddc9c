"""bench.py's command line, without a GPU: --full is an option of its own, off by default, and leaves the others alone."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse_args()


def test_full_is_off_by_default(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and (a.gpus, a.steps, a.warmup) == (1, 20, 5)
    assert a.workload == "ekf" and a.dump_outputs is None


def test_full_switches_on_and_keeps_the_trimming_options(monkeypatch):
    a = _parse(monkeypatch, ["--full", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-extras"])
    assert a.full is True and a.no_cpu_baseline is True and a.no_extras is True and (a.steps, a.warmup) == (20, 5)
