"""CPU checks of the landmark reads (cslam_ekf_get_landmarks, cslam_ekf_batch_get_landmarks): declared and documented in
include/cslam.h, exported by the library, reachable from EKF / EKFBatch."""
import ctypes
import os

from conan_slam_amd import EKF, EKFBatch, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cslam_ekf_get_landmarks", "cslam_ekf_batch_get_landmarks")


def test_header_declares_and_documents_the_landmark_reads():
    names = _capi.declared_symbols()
    for s in NEW:
        assert s in names, s
    assert set(NEW) == set(_capi.LANDMARK_SYMBOLS)
    text = open(os.path.join(ROOT, "include", "cslam.h")).read()
    i = text.index("int cslam_ekf_get_landmarks(")
    doc = text[text.rindex("/*", 0, i): i]
    for cite in ("test/main.cpp:107-108", "EKF.cpp:131-144"):
        assert cite in doc, cite
    assert "NEVER applies the pending" in doc
    assert "int cslam_ekf_batch_get_landmarks(cslam_ekf_batch_t h, int first, int count, float* x, float* pll, float* pvl);" in text


def test_library_exports_the_landmark_reads():
    assert os.path.exists(_capi.LIB_PATH), "build the engine first: python -m conan_slam_amd.build"
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s
    # the loaded binding carries their prototypes
    L = _capi.lib()
    for s in NEW:
        assert getattr(L, s).restype is ctypes.c_int and len(getattr(L, s).argtypes) == 6, s


def test_python_classes_have_landmarks():
    assert callable(getattr(EKF, "landmarks", None))
    assert callable(getattr(EKFBatch, "landmarks", None))
