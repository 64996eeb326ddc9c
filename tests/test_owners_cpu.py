"""The owning types of conan_slam_amd/csrc/device_owners.hpp (DevBuf, PinnedBuf, Event, Stream): a host-only C++ check,
built and run here.  Without a GPU it covers the empty state and the failure path (CSLAM_ERR_HIP, owner left empty, error
text set); with one it allocates a few KB and checks zero fill, moves, reset and the all-or-nothing growth sequence."""
import os
import subprocess

from conan_slam_amd import build as cbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_check_builds_and_passes(tmp_path):
    src = os.path.join(ROOT, "tests", "owners", "owners_check.cpp")
    exe = str(tmp_path / "owners_check")
    r = subprocess.run([cbuild._hipcc(), "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "conan_slam_amd", "csrc"),
                        src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
