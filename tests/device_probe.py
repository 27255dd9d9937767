"""ctypes front of tests/device_probe/libfs_probe.so (probe.hip: thin kernels around the __device__ functions of fs_device.hpp; built by
`make -C flow-sim_amd/csrc probe`, which __graft_entry__.build() runs).  TEST INFRASTRUCTURE: the product never loads it.  Arrays go
in and come out as numpy arrays of the device type (float64 / float32); a HIP error raises."""
import ctypes
import os

import numpy as np

import helper_reference as HR

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_probe", "libfs_probe.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"probe library not built: {LIB_PATH} (make -C flow-sim_amd/csrc probe)")
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.fsp_error_string.restype = ctypes.c_char_p
    return _lib


def _suffix(a):
    return {np.dtype(np.float64): "f64", np.dtype(np.float32): "f32"}[a.dtype]


def _call(name, like, *args):
    """args: numpy arrays go as pointers (they must be contiguous and of the type of `like`, int32 for flags), Python ints as int,
    numpy scalars of the device type by value"""
    l = lib()
    fn = getattr(l, f"{name}_{_suffix(like)}")
    real = ctypes.c_double if like.dtype == np.float64 else ctypes.c_float
    conv = []
    for a in args:
        if isinstance(a, np.ndarray):
            assert a.flags["C_CONTIGUOUS"] and a.dtype in (like.dtype, np.dtype(np.int32)), (name, a.dtype)
            conv.append(a.ctypes.data_as(ctypes.c_void_p))
        elif isinstance(a, (int, np.integer)):
            conv.append(ctypes.c_int(int(a)))
        else:
            conv.append(real(float(a)))
    fn.restype = ctypes.c_int
    e = fn(*conv)
    if e != 0:
        raise RuntimeError(f"{name}: HIP error {e}: {l.fsp_error_string(e).decode()}")


def _in(a, D):
    a = np.ascontiguousarray(a)
    assert a.dtype == D, (a.dtype, D)
    return a


def unary(code, x):
    x = _in(x, x.dtype)
    y = np.empty_like(x)
    _call("fsp_unary", x, code, x, y, len(x))
    return y


def power(which, a, b):
    """which 0: pow_pos, 1: pow_"""
    a, b = _in(a, a.dtype), _in(b, a.dtype)
    y = np.empty_like(a)
    _call("fsp_pow", a, which, a, b, y, len(a))
    return y


def k15(A, P, n15):
    A, P, n15 = _in(A, A.dtype), _in(P, A.dtype), _in(n15, A.dtype)
    y = np.empty_like(A)
    _call("fsp_k15", A, A, P, n15, y, len(A))
    return y


def node_terms(form, sec, h, Q):
    """form 0 node_terms_rect, 1 node_terms_trap, 2 node_terms_general; the seven NodeTerms fields as written (eQh, not eQ)"""
    D = h.dtype.type
    s, h, Q = HR.sec_array(sec, D), _in(h, D), _in(Q, D)
    out = np.empty((7, len(h)), dtype=D)
    _call("fsp_node_terms", h, form, s, h, Q, out, len(h))
    return dict(zip(("A", "T", "Se", "eAT", "eQh", "v", "rT"), out))


def general_props(sec, h):
    D = h.dtype.type
    s, h = HR.sec_array(sec, D), _in(h, D)
    out = np.empty((13, len(h)), dtype=D)
    _call("fsp_general_props", h, s, h, out, len(h))
    return dict(zip(HR.PROP_FIELDS, out))


def sec_derive(secs, D):
    s = np.ascontiguousarray(np.stack([HR.sec_array(sec, D) for sec in secs]))
    out = np.empty((9, len(secs)), dtype=D)
    _call("fsp_sec_derive", s, s, out, len(secs))
    return dict(zip(HR.DERIVE_FIELDS, out))


def rating_blend(rcp, p, z):
    """rating_blend<true> (rcp != 0) or rating_blend<false>; p: s0, buf, l0, l1, l2, h0, h1, h2"""
    z = _in(z, z.dtype)
    p = _in(np.asarray(p, dtype=z.dtype), z.dtype)
    assert len(p) == 8
    y = np.empty_like(z)
    _call("fsp_rating_blend", z, int(bool(rcp)), p, z, y, len(z))
    return y


def bc(form, kind, params, sec, level, dt, h, Q, Qold, Yprev, tgt):
    """form 0 bc_eval<false>, 1 bc_eval_rect; returns res, dh, dq, Ynew, flag"""
    D = h.dtype.type
    arrays = [_in(a, D) for a in (h, Q, Qold, Yprev, tgt)]
    p = _in(np.asarray(params, dtype=D), D)
    assert len(p) == 10
    out = np.empty((4, len(h)), dtype=D)
    flag = np.full(len(h), -1, dtype=np.int32)
    _call("fsp_bc", arrays[0], form, kind, p, HR.sec_array(sec, D), level, D(dt), *arrays, out, flag, len(h))
    return dict(res=out[0], dh=out[1], dq=out[2], Ynew=out[3], flag=flag)
