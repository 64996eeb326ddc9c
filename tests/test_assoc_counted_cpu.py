"""The cap that keeps the loop of test_assoc_counted_gpu.py honest, proven on the CPU oracle alone: every observation of
every step of assoc_counted_loop.get_loop is decisive by assoc_builders' margin rule (every comparison that fixes its
(idf, kind) has an f64 margin of at least tau = 64 x the C oracle's own error), none is left out, and the scans have the
counts the GPU test relies on."""
import numpy as np
import pytest

from assoc_counted_loop import KINDS, STEPS, get_loop


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("shape", ["all", "split", "split32"])
def test_every_observation_of_every_step_is_decisive(shape, dtype):
    steps = get_loop(shape, dtype)
    assert len(steps) == STEPS
    want = [KINDS[shape].count(k) for k in (1, 2, 0)]
    for t, s in enumerate(steps):
        assert s["Z"].shape == (2, len(KINDS[shape])) and s["Z"].dtype == np.dtype(dtype)
        assert s["margin"] >= s["tau"] > 0, (t, s["margin"], s["tau"])
        assert [int((s["kind"] == k).sum()) for k in (1, 2, 0)] == want, (t, s["kind"])
        assert np.all(s["idf"][s["kind"] == 1] > 0) and np.all(s["idf"][s["kind"] != 1] == 0)
        assert len(set(s["idf"][s["kind"] == 1])) == want[0]  # (distinct landmarks: a batch update of each once)
    # the scans differ from step to step (the pose moves and the noise is drawn anew)
    assert not np.array_equal(steps[0]["Z"], steps[1]["Z"])
