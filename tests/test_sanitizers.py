"""AddressSanitizer + UndefinedBehaviorSanitizer over the C pieces, in the build container (GPU sanitizers
and XNACK are not available on this pool, so the device code is covered by the bitwise batch- / shard-invariance tests
instead):

  * oracle/preissmann_oracle.c - the C restatement with its banded LU - `make -C oracle SAN=1`, loaded into a python that
    was started with the gcc sanitizer runtimes preloaded, and run through tests/test_oracle_c.py (every reference-generated
    fixture of the trapezoid family + fresh 700-node inputs);
  * the host side of the C ABI (flow-sim_amd/csrc/fs_abi.hip: descriptor validation, kernel dispatch table, error texts,
    NULL handles) - a host-only clang build of the same source with -fsanitize=address,undefined - driven by two plain-C
    programs: tests/c_abi/host_paths.c and tests/c_abi/smoke.c (which on a box without a GPU ends in "no HIP device").  What
    that side computes without a device (fs_host_pack.hpp: pack_polylines, extend_table, the boundary checks) has its own
    sanitized build: tests/test_host_pack.py."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "flow-sim_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang"
HIPCC = "/opt/rocm/bin/hipcc"


def gcc_runtime(name):
    p = subprocess.run(["gcc", f"-print-file-name={name}"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def test_c_oracle_under_asan_and_ubsan():
    asan, ubsan = gcc_runtime("libasan.so"), gcc_runtime("libubsan.so")
    if shutil.which("gcc") is None or asan is None or ubsan is None:
        pytest.skip("no gcc sanitizer runtimes")
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "SAN=1"], check=True, capture_output=True)
    env = dict(os.environ, LD_PRELOAD=f"{asan}:{ubsan}", FS_ORACLE_SAN="1",
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_oracle_c.py"), "-x", "-q", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert " passed" in r.stdout
    # the sanitized library is the one that ran
    probe = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from oracle import c_oracle as C; C.lib(); print(C._SO)" % ROOT],
                           env=env, capture_output=True, text=True)
    assert probe.stdout.strip().endswith("liboracle_c_san.so"), probe.stdout + probe.stderr


@pytest.fixture(scope="module")
def host_sanitized_library(tmp_path_factory):
    if not (os.path.exists(CLANG) and os.path.exists(HIPCC)):
        pytest.skip("no ROCm clang")
    d = tmp_path_factory.mktemp("hostsan")
    lib = str(d / "libflowsim_hip.so")
    # host code only (--cuda-host-only: no device code is compiled or embedded; nothing here launches a kernel)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    obj = str(d / "fs_abi.o")
    r = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-host-only", *san, "-Wno-unused-result",
                        "-DFS_MINIMAL=1", "-c", "-o", obj, os.path.join(CSRC, "fs_abi.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    # the host object still refers to the device image it would normally embed (__hip_fatbin_<hash>): an empty stand-in - it is
    # only ever looked at when a kernel is launched, which nothing here does
    und = [ln.split()[-1] for ln in subprocess.run(["nm", "-u", obj], capture_output=True, text=True).stdout.splitlines() if "__hip_fatbin" in ln]
    stub, sobj = str(d / "fatbin_stub.c"), str(d / "fatbin_stub.o")
    open(stub, "w").write("".join(f"const char {u}[8] = {{0}};\n" for u in und) or "int fs_no_stub;\n")
    subprocess.run([CLANG, "-fPIC", "-c", stub, "-o", sobj], check=True)
    r = subprocess.run([HIPCC, "-shared", *san, "-o", lib, obj, sobj, "-L/opt/rocm/lib", "-lrocprofiler-sdk-roctx", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(d), lib


@pytest.mark.parametrize("program, want_rc, want_text", [("host_paths.c", 0, "host paths answered"), ("smoke.c", None, None)])
def test_host_side_of_the_abi_under_asan_and_ubsan(host_sanitized_library, program, want_rc, want_text, tmp_path):
    libdir, _ = host_sanitized_library
    exe = str(tmp_path / program[:-2])
    cmd = [CLANG, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi", program), "-L", libdir, "-lflowsim_hip", "-lm",
           "-Wl,-rpath," + libdir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    if want_rc is None:                       # smoke.c: 2 without a GPU ("no HIP device"), and a host-only library cannot launch anyway
        from flowsim_amd import _abi as A
        if A.device_count() > 0:
            pytest.skip("host-only build: meant for the box without a GPU")
        assert r.returncode == 2 and "no HIP device" in r.stdout, (r.returncode, out[-2000:])
    else:
        assert r.returncode == want_rc and want_text in r.stdout, (r.returncode, out[-2000:])
