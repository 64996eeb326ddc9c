"""The host-only parts of the EKF engine (conan_slam_amd/csrc/ekf_options.hpp: the engine switches and their parsing;
ekf_pending_store.hpp: the bookkeeping of the pending W1 store): a C++ check with its own main, built with plain g++ and
run here -- once as it is, once as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "host_parts_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "conan_slam_amd", "csrc")]
# (the sanitizer runtimes are linked statically: the program is self-contained)
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_host_parts_check_builds_and_passes(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    env = {k: v for k, v in os.environ.items() if not k.startswith("CSLAM_")}
    for name, extra in (("plain", []), ("sanitized", SANITIZE)):
        exe = str(tmp_path / f"host_parts_check_{name}")
        r = subprocess.run([gxx] + FLAGS + extra + [SRC, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, name + ": " + r.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
        print(name, r.stdout)
        assert r.returncode == 0, name + ": " + r.stdout + r.stderr
        assert "0 failed" in r.stdout, name
