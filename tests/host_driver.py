"""The sanitized host drivers of the tests (tests/*/*_driver.cpp: plain C++ of flow-sim_amd/csrc built by the system compiler with its
own main): the one compile line, the one way to run them and refuse any sanitizer report, and the line format of the `checks` input of
tests/host_pack/host_pack_driver.cpp (PACK_DRIVER: tests/test_host_pack.py, tests/test_batch_pack.py)."""
import os
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "flow-sim_amd", "csrc")
PACK_DRIVER = os.path.join(ROOT, "tests", "host_pack", "host_pack_driver.cpp")


def build(source, out_dir, include_dirs=(CSRC,), extra_flags=()):
    """the program of one driver source under AddressSanitizer and UBSan, warnings as errors; named after the source"""
    exe = os.path.join(str(out_dir), os.path.splitext(os.path.basename(source))[0])
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra_flags, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    for d in include_dirs:
        cmd += ["-I", str(d)]
    r = subprocess.run(cmd + ["-o", exe, str(source)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe, args, env_extra=None, drop_env=(), timeout=60):
    """its standard output; a sanitizer report or another exit status than 0 fails the test"""
    env = {k: v for k, v in os.environ.items() if k not in drop_env}
    env.update(env_extra or {}, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def line(what, *fields):
    return what + " " + " ".join(float(v).hex() if isinstance(v, (float, np.floating)) else str(int(v)) for v in fields)
