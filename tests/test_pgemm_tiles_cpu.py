"""The work list of the f32 P-GEMM's tail phase (conan_slam_amd/csrc/ekf_pgemm_tiles.hpp: whole tiles, then 32-row strips;
the rule for how many tiles are split) and its switch CSLAM_PGEMM_TAIL (ekf_options.hpp): a C++ check with its own main,
built with plain g++ and run here -- once as it is, once as a stand-alone program under the address and
undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "conan_slam_amd", "csrc")]
# (the sanitizer runtimes are linked statically: the program is self-contained)
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_pgemm_tiles_check_builds_and_passes(tmp_path):
    src = os.path.join(HOST, "pgemm_tiles_check.cpp")
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    env = {k: v for k, v in os.environ.items() if not k.startswith("CSLAM_")}
    for name, extra in (("plain", []), ("sanitized", SANITIZE)):
        exe = str(tmp_path / f"pgemm_tiles_check_{name}")
        r = subprocess.run([gxx] + FLAGS + extra + [src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, name + ": " + r.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
        print(name, r.stdout)
        assert r.returncode == 0, name + ": " + r.stdout + r.stderr
        assert "0 failed" in r.stdout, name
