"""The host-only parts of the engines -- the EKF's (conan_slam_amd/csrc/ekf_options.hpp: the engine switches and their
parsing; ekf_pending_store.hpp: the bookkeeping of the pending W1 store) and the particle handle's (pf_host_parts.hpp:
staging layout, staged and association memos, exchange bookkeeping, strata): C++ checks with their own main, built with
plain g++ and run here -- once as they are, once as stand-alone programs under the address and undefined-behaviour
sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "conan_slam_amd", "csrc")]
# (the sanitizer runtimes are linked statically: the program is self-contained)
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def build_and_run(stem, tmp_path):
    src = os.path.join(HOST, stem + ".cpp")
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    env = {k: v for k, v in os.environ.items() if not k.startswith("CSLAM_")}
    for name, extra in (("plain", []), ("sanitized", SANITIZE)):
        exe = str(tmp_path / f"{stem}_{name}")
        r = subprocess.run([gxx] + FLAGS + extra + [src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, name + ": " + r.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
        print(name, r.stdout)
        assert r.returncode == 0, name + ": " + r.stdout + r.stderr
        assert "0 failed" in r.stdout, name


def test_host_parts_check_builds_and_passes(tmp_path):
    build_and_run("host_parts_check", tmp_path)


def test_pf_host_parts_check_builds_and_passes(tmp_path):
    build_and_run("pf_host_parts_check", tmp_path)
