"""cslam_ekf_associate_deferred without a GPU: the decomposed rule of its two kernels equals the reference's sequential
loop, the deferred 2 x 2 block equals the true one, and the pending-state builder of test_assoc_deferred_gpu.py keeps its
promises (every observation decisive under the true P; the flips flip under the stale blocks)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from assoc_builders import CASE_KEYS, GATES, case_id, decide, get_case
from assoc_deferred_ref import (BLOCK, NEG_N, PENDING_SEEDS, SIG2_HEADING, check_pending, decide_blocks, deferred_block,
                                get_pending, panels_of, search_seed_pending, split_scan)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAULTS = ("last_block_tie", "outer_ungated_only", "partial_nis_gated_only")


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("key", CASE_KEYS, ids=case_id)
def test_decomposed_rule_equals_the_sequential_rule(key):
    case = get_case(key)
    nis, nd = case.ref()[:2]
    for gates in GATES:
        assert _same(decide_blocks(nis, nd, *gates), decide(nis, nd, *gates)[:2]), (case, gates)
        # ... at every block size, the wave's included
        for block in (1, 64, 100):
            assert _same(decide_blocks(nis, nd, *gates, block=block), decide(nis, nd, *gates)[:2]), (case, gates, block)


def hand_rows():
    """nis / nd [7, 320] with gate1 = 4, gate2 = 25: everything far (nis = 100, nd = 50) except what the row is about."""
    nis, nd = np.full((7, 320), 100.0), np.full((7, 320), 50.0)
    nis[0, 5], nd[0, 5] = 1.0, np.nan                      # a NaN nd inside gate1: no record, feeds outer -> dropped
    nis[1, 7], nd[1, 7] = 2.0, np.inf                      # nd = +inf inside gate1: never below the initial best
    nis[2, [10, 20]], nd[2, [10, 20]] = (1.0, 2.0), 3.0    # an exact tie within a block
    nis[3, [10, 300]], nd[3, [10, 300]] = (1.0, 2.0), 3.0  # ... across a block boundary
    nis[4, 300], nd[4, 300] = 1.0, -np.inf                 # log det = -inf
    nis[5, 12], nd[5, 12] = 10.0, 1.0                      # nothing gated, the smallest nis between the gates -> dropped
    nis[6, 3], nd[6, 3] = np.nan, np.nan                   # a NaN nis takes part in nothing
    nis[6, 299], nd[6, 299] = 3.0, 7.0
    return nis, nd


def test_decomposed_rule_on_hand_made_rows():
    nis, nd = hand_rows()
    idf, kind = decide_blocks(nis, nd, 4.0, 25.0)
    assert _same((idf, kind), decide(nis, nd, 4.0, 25.0)[:2])
    assert list(idf) == [0, 0, 11, 11, 301, 0, 300] and list(kind) == [0, 0, 1, 1, 1, 0, 1]
    for nf in (0, 1):
        e = np.zeros((3, nf))
        assert _same(decide_blocks(e, e, 4.0, 25.0), decide(e, e, 4.0, 25.0)[:2])
    assert list(decide_blocks(np.zeros((3, 0)), np.zeros((3, 0)), 4.0, 25.0)[1]) == [2, 2, 2]


def test_negative_controls_of_the_decomposed_rule_change_decisions():
    """Each fault changes at least one decision, on the hand-made rows and on a builder case."""
    nis, nd = hand_rows()
    good = decide_blocks(nis, nd, 4.0, 25.0)
    bad = decide_blocks(nis, nd, 4.0, 25.0, fault="last_block_tie")
    assert bad[0][3] == 301 and bad[0][2] == 11 and not _same(good, bad)      # only the tie across the boundary moves
    assert decide_blocks(nis, nd, 4.0, 25.0, fault="outer_ungated_only")[1][0] == 2 != good[1][0]
    assert decide_blocks(nis, nd, 4.0, 25.0, fault="partial_nis_gated_only")[1][5] == 2
    per_case = {"last_block_tie": ("B", 0, "float32"), "outer_ungated_only": ("F", "lone", "float32"),
                "partial_nis_gated_only": ("D", 0, "float32")}
    for fault, key in per_case.items():
        case = get_case(key)
        cn, cd = case.ref()[:2]
        assert any(not _same(decide_blocks(cn, cd, *g, fault=fault), decide(cn, cd, *g)[:2]) for g in case.gates), fault
    assert BLOCK == 256


PENDING_KEYS = sorted(PENDING_SEEDS)


@pytest.mark.parametrize("key", PENDING_KEYS, ids=lambda k: f"nf{k[0]}-{k[1]}-{k[2]}")
def test_pending_builder_is_decisive_and_its_flips_flip(key):
    nf, dt, variant = key
    p = get_pending(nf, np.dtype(dt).type, variant)
    c = check_pending(p)
    assert c.m == p.Z.shape[1] == len(p.own) + len(p.far) + len(p.flips)
    if variant == "neg":
        assert len(p.flips) >= 1 and len(p.steps) == 1
    else:
        assert len(p.flips) >= 4 and len(p.steps) == 3
        assert [st[0] for st in p.steps].count("heading") == (1 if variant == "pos" else 0)


@pytest.mark.parametrize("variant", ["pos", "la", "neg"])
def test_deferred_block_equals_the_true_block(variant):
    """Ps - sum s_c w w^T over the panels of the builder's steps is the oracle's f64 block; without the panels, or with the
    sign dropped, it is not."""
    negative = variant == "neg"
    nf = NEG_N if negative else 65
    p = get_pending(nf, np.float64, variant)
    Wp, s, P_np = panels_of(p.steps, p.X0, p.P0, p.R, SIG2_HEADING)
    assert Wp.shape[1] == {"pos": 33, "la": 72, "neg": 1}[variant] and (s < 0).sum() == (1 if negative else 0)
    worst, moved, sign = 0.0, 0.0, 0.0
    for f in range(nf):
        fx = 3 + 2 * f
        true = p.P1[fx:fx + 2, fx:fx + 2].astype(np.float64)
        got = deferred_block(p.P0.astype(np.float64), Wp, s, f)
        scale = np.abs(true).max()
        worst = max(worst, np.abs(got - true).max() / scale)
        moved = max(moved, np.abs(p.P0[fx:fx + 2, fx:fx + 2] - true).max() / scale)
        sign = max(sign, np.abs(deferred_block(p.P0.astype(np.float64), Wp, np.abs(s), f) - true).max() / scale)
    assert worst < 1e-9, worst
    assert moved > 1e-2, moved
    if negative:
        assert sign > 1e-2, sign


@pytest.mark.parametrize("key", PENDING_KEYS, ids=lambda k: f"nf{k[0]}-{k[1]}-{k[2]}")
def test_committed_seed_is_what_the_search_finds(key):
    nf, dt, variant = key
    assert search_seed_pending(nf, np.dtype(dt).type, variant) == PENDING_SEEDS[key]


def test_split_scan_has_all_three_kinds_and_is_decisive():
    case = split_scan()
    kind = case.decisions(GATES[0])[1]
    assert [int((kind == k).sum()) for k in (1, 2, 0)] == [30, 5, 5]
    assert np.all(case.margins(GATES[0]) >= case.tau()[0])


def test_adapter_program_compiles_and_links(tmp_path):
    """tests/adapter/adapter_assoc_deferred.cpp (run on the GPU by tests/test_adapter_assoc_deferred_gpu.py) against the
    stand-in: HipEKF::setDeferredAssociation and the new entry point behind Slam::dataAssociate."""
    from conan_slam_amd import _capi

    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    libdir = os.path.dirname(os.path.abspath(_capi.LIB_PATH))
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "tests", "adapter"),
                        os.path.join(ROOT, "tests", "adapter", "adapter_assoc_deferred.cpp"), "-L" + libdir, "-lcslam_hip",
                        "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined", "-o",
                        str(tmp_path / "adapter_assoc_deferred")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_prototypes_are_declared_and_bound():
    from conan_slam_amd import EKF, _capi

    names = _capi.declared_symbols()
    for s in _capi.EKF_ASSOC_DEFERRED_SYMBOLS:
        assert s in names and s in _capi._PROTOTYPES, s
    for meth in ("associate_deferred", "data_associate_deferred", "association_device_ptrs"):
        assert callable(getattr(EKF, meth))
