"""A numpy restatement of pf_assoc_vote_kernel (conan_slam_amd/csrc/pf_vote_kernels.hpp): the rule, the ordered
compaction and the counts -- written the way the kernel computes them (a sequential three-term sum per row, tiles of 256
with a running base), NOT by calling pf.new_feature_votes, against which tests/test_pf_vote_cpu.py holds it."""
from collections import namedtuple

import numpy as np

TILE = 256  # kPfVoteLanes
Vote = namedtuple("Vote", "use new_idx ZN q count")

# The edge rows of the rule with the answers of pf.new_feature_votes, per new_fraction: (row, {fraction: new?})
EDGE_ROWS = (
    ((0.5, 0.5, 0.0), {0.5: True, 0.0: True, 1.0: False, 1.5: False}),     # equality
    ((0.75, 0.25, 0.0), {0.5: False, 0.0: True, 1.0: False, 1.5: False}),
    ((0.0, 0.0, 0.0), {0.5: False, 0.0: False, 1.0: False, 1.5: False}),   # no mass
    ((0.0, 0.0, 1.0), {0.5: False, 0.0: False, 1.0: False, 1.5: False}),   # all ambiguous
    ((0.0, 1.0, 0.0), {0.5: True, 0.0: True, 1.0: True, 1.5: False}),      # all new
)
FRACTIONS = (0.0, 0.5, 1.0, 1.5)


def is_new(summary, new_fraction):
    """total = (s0 + s1) + s2 in float64, in this order; new when total > 0, s1 > 0 and s1 >= new_fraction * total."""
    s = np.asarray(summary, dtype=np.float64).reshape(-1, 4)
    f = np.float64(new_fraction)
    out = np.zeros(s.shape[0], bool)
    for j in range(s.shape[0]):
        total = np.float64(np.float64(s[j, 0] + s[j, 1]) + s[j, 2])
        out[j] = bool(total > 0.0) and bool(s[j, 1] > 0.0) and bool(s[j, 1] >= f * total)
    return out


def vote(summary, Z, new_fraction):
    """-> Vote(use [m] int32, new_idx [q] int32, ZN [2 x q] in Z's dtype, q, count = (q, m)): tile by tile, a lane's slot
    is the running base plus the number of new lanes below it in the tile."""
    Z = np.asarray(Z)
    Z = Z.reshape(2, -1, order="F") if Z.size else np.zeros((2, 0), Z.dtype)
    m = Z.shape[1]
    new = is_new(summary, new_fraction)
    assert new.shape[0] == m
    use = np.where(new, 0, 1).astype(np.int32)
    new_idx = np.full(m, -1, np.int32)  # (entries from q on are never written)
    ZN = np.zeros((2, m), Z.dtype, order="F")
    base = 0
    for t0 in range(0, m, TILE):
        flags = new[t0:t0 + TILE]
        rank = np.cumsum(flags) - flags  # new lanes below
        for lane in np.nonzero(flags)[0]:
            k = base + int(rank[lane])
            new_idx[k] = t0 + lane
            ZN[:, k] = Z[:, t0 + lane]
        base += int(flags.sum())
    q = base
    return Vote(use, new_idx[:q].copy(), np.asfortranarray(ZN[:, :q]), q, (q, m))


def host_policy(summary, Z, new_fraction):
    """What pf.data_associate derives from the same summary -> Vote (the reference the device vote is held against)."""
    from conan_slam_amd.pf import new_feature_votes

    Z = np.asarray(Z)
    Z = Z.reshape(2, -1, order="F") if Z.size else np.zeros((2, 0), Z.dtype)
    s = np.asarray(summary, dtype=np.float64).reshape(-1, 4)
    new = new_feature_votes(s, new_fraction) if s.shape[0] else np.zeros(0, bool)
    idx = np.nonzero(new)[0].astype(np.int32)
    return Vote(np.where(new, 0, 1).astype(np.int32), idx, np.asfortranarray(Z[:, new]), int(idx.shape[0]),
                (int(idx.shape[0]), Z.shape[1]))


def same(a, b):
    """Two Votes, bit for bit."""
    return (a.q == b.q and a.count == b.count and a.use.dtype == b.use.dtype and np.array_equal(a.use, b.use)
            and np.array_equal(a.new_idx, b.new_idx) and a.ZN.dtype == b.ZN.dtype and a.ZN.shape == b.ZN.shape
            and a.ZN.tobytes(order="F") == b.ZN.tobytes(order="F"))


def random_summaries(rng, m):
    """Rows that exercise the rule: ordinary masses, exact ties at common fractions, zero rows, rows nobody calls new."""
    s = np.zeros((m, 4))
    s[:, :3] = rng.random((m, 3)) * rng.choice([1.0, 1e-300, 1e300, 1.0 / 3.0], (m, 1))
    kind = rng.integers(0, 8, m)
    s[kind == 0, 1] = 0.0                       # nobody calls it new
    s[kind == 1, :3] = 0.0                      # no mass
    s[kind == 2, 0] = s[kind == 2, 1]           # half and half ...
    s[kind == 2, 2] = 0.0                       # ... exactly
    s[kind == 3, 0] = s[kind == 3, 2] = 0.0     # all new
    s[kind == 4, :2] = 0.0                      # all ambiguous
    s[:, 3] = rng.integers(0, 100, m)
    return s
