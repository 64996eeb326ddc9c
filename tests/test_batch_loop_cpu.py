"""CPU checks of the batched engine's reference-loop surface (cslam_ekf_batch_predict / observe_heading / update /
augment, create_capacity): declared in include/cslam.h, exported by the library, reachable from EKFBatch."""
import ctypes
import os
import re

from conan_slam_amd import EKFBatch, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cslam_ekf_batch_create_capacity", "cslam_ekf_batch_predict", "cslam_ekf_batch_observe_heading",
       "cslam_ekf_batch_update", "cslam_ekf_batch_augment")


def test_header_declares_the_batch_loop_entry_points():
    names = _capi.declared_symbols()
    for s in NEW:
        assert s in names, s
    text = open(os.path.join(ROOT, "include", "cslam.h")).read()
    m = re.search(r"#define\s+CSLAM_FACTOR_HEADING_SKIPPED\s+(\d+)", text)
    assert m and int(m.group(1)) == 32 == _capi.FACTOR_HEADING_SKIPPED
    # every new declaration cites the reference interface it replaces
    for cite in ("slam.h:841-847", "slam.h:788", "slam.h:938-943", "slam.h:190-191", "test/main.cpp:107-108"):
        assert cite in text, cite


def test_library_exports_the_batch_loop_entry_points():
    assert os.path.exists(_capi.LIB_PATH), "build the engine first: python -m conan_slam_amd.build"
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s


def test_ekfbatch_has_the_reference_loop_methods():
    for name in ("predict", "observe_heading", "update_device", "augment_device"):
        assert callable(getattr(EKFBatch, name, None)), name
    assert isinstance(EKFBatch.__dict__.get("n"), property)
