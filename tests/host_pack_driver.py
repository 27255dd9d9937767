"""The sanitized host driver of the C ABI's packing code (tests/host_pack/host_pack_driver.cpp), shared by tests/test_host_pack.py
and tests/test_batch_pack.py: how it is built, how it is run, and the line format of its `checks` input."""
import os
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "flow-sim_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "host_pack", "host_pack_driver.cpp")


def build_driver(out_dir, include_dirs):
    exe = os.path.join(str(out_dir), "host_pack_driver")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer"]
    for d in include_dirs:
        cmd += ["-I", str(d)]
    r = subprocess.run(cmd + ["-o", exe, DRIVER], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_driver(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def line(what, *fields):
    return what + " " + " ".join(float(v).hex() if isinstance(v, (float, np.floating)) else str(int(v)) for v in fields)
