"""CPU side of the control run and the whole-cycle calls: the host parts (the split of k steps into launches of 16, the
refusal rule) as a stand-alone program, plain and under the address and undefined-behaviour sanitizers; the constant of
the f64 device-against-oracle check of a 6-step run, measured on the CPU oracle (tests/pf_control_ref.py says how);
and the new entry points declared, cited, bound, exported and mirrored.  Run with -s to see the measured figures."""
import ctypes
import os

import numpy as np

import pf_control_ref as CR
from test_host_parts_cpu import build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEED = ("cslam_pf_control_run", "cslam_pf_control_launches", "cslam_pf_cycle_drawn", "cslam_pf_assoc_cycle_drawn")


def test_control_check_builds_and_passes(tmp_path):
    build_and_run("pf_control_check", tmp_path)


def test_the_control_sequence_differs_per_step():
    v, swa, phi = CR.controls(33, seed=5)
    for a in (v, swa, phi):
        assert len(set(np.asarray(a, np.float32).tolist())) == 33  # (distinct after the cast to f32 as well)


def test_c_control_is_four_times_the_measured_constant():
    """The CPU oracle over the heading-known run of the GPU oracle test, in f32 and in f64 from the same inputs: the
    difference in units of u32 * magnitude is the amplification of the chain; C_CONTROL is 4 x it -- no less, and not
    idly more -- and bounds the f64 device run in units of u64 * magnitude."""
    parts, v, swa, phi = CR.oracle_run_case()
    assert len(v) == CR.ORACLE_K == 6 and len(parts) == CR.ORACLE_NP
    lo = CR.oracle_chain(parts, v, swa, phi, np.float32)
    hi = CR.oracle_chain(parts, v, swa, phi, np.float64)
    ex, ep = CR.units(lo, hi, CR.U[CR.F32])
    c = max(ex, ep)
    print(f"f32 against f64 oracle over k = {CR.ORACLE_K}, np = {CR.ORACLE_NP}: Xv {ex:.2f}, Pv {ep:.2f} units of u32 * "
          f"magnitude; C_CONTROL {CR.C_CONTROL}")
    assert 4.0 * c <= CR.C_CONTROL <= 4.0 * c + 1.0, (ex, ep, CR.C_CONTROL)
    # the heading is what makes the chain hard: without it the same run needs a far smaller constant
    lo0 = CR.oracle_chain(parts, v, swa, phi, np.float32, use_heading=False)
    hi0 = CR.oracle_chain(parts, v, swa, phi, np.float64, use_heading=False)
    ex0, ep0 = CR.units(lo0, hi0, CR.U[CR.F32])
    print(f"the same run without the heading: Xv {ex0:.2f}, Pv {ep0:.2f}")
    assert max(ex0, ep0) <= c
    # ... and the f64 oracle passes its own bound (it is the reference: zero units)
    assert max(CR.units(hi, hi, CR.U[CR.F64])) == 0.0


def test_entry_points_declared_cited_bound_and_exported():
    from conan_slam_amd import _capi

    names = _capi.declared_symbols()
    assert _capi.PF_CONTROL_SYMBOLS == NEED
    for n in NEED:
        assert n in names and n in _capi._PROTOTYPES, n
    assert _capi.PF_CONTROL_MAX == 16
    text = open(os.path.join(ROOT, "include", "cslam.h")).read()
    block = text[text.index("---- a run of control steps in one launch"):text.index("int cslam_pf_assoc_cycle_drawn")]
    for cite in ("test/main.cpp:249-334", "test/main.cpp:279-286", "slam.h:69-77", "slam.h:99", "PF.cpp:419-471",
                 "PF.cpp:382-417", "slam.h:700-725", "test/main.cpp:294-328", "PF.cpp:502-544", "PF.cpp:222-277",
                 "PF.cpp:473-500", "PF.cpp:9-60", "test/main.cpp:314-328", "EKF.cpp:131-144"):
        assert cite in block, cite
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for n in NEED:
        assert hasattr(lib, n), n
    # the kernel's constant, the host parts' and the Python mirror agree
    csrc = os.path.join(ROOT, "conan_slam_amd", "csrc")
    assert "constexpr int kPfControlMax = 16;" in open(os.path.join(csrc, "pf_control_kernels.hpp")).read()
    assert "constexpr int kPfControlChunk = 16;" in open(os.path.join(csrc, "pf_host_parts.hpp")).read()


def test_python_layer_has_the_methods():
    from conan_slam_amd.pf import ParticleShard

    for n in ("control_run", "control_launches", "cycle_drawn", "assoc_cycle_drawn"):
        assert callable(getattr(ParticleShard, n)), n


def test_controls_are_broadcast():
    """_controls: scalars or sequences of equal length for v and swa, a scalar phi for every step"""
    from conan_slam_amd.pf import ParticleShard

    sh = object.__new__(ParticleShard)  # (no handle: _controls needs the dtype alone)
    sh.dtype = np.dtype(np.float32)
    keep, args = ParticleShard._controls(sh, [1.0, 2.0, 3.0], 0.5, np.eye(2), 2.0, 0.1, 0.25, True)
    assert args[0].value == 3 and keep[0].tolist() == [1.0, 2.0, 3.0] and keep[1].tolist() == [0.5] * 3
    assert keep[2].tolist() == [0.25] * 3 and args[7].value == 1 and keep[3].dtype == np.float32
    keep, args = ParticleShard._controls(sh, 4.0, 0.5, np.eye(2), 2.0, 0.1, None, False)
    assert args[0].value == 1 and keep[2] is None and args[6] is None
    keep, args = ParticleShard._controls(sh, [], [], None, 2.0, 0.1, None, False)
    assert args[0].value == 0 and args[3] is None
    sh._h = None  # (so that __del__ has nothing to close)
