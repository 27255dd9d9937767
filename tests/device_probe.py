"""ctypes front of tests/device_probe/libfs_probe.so (probe.hip: thin kernels around the __device__ functions of fs_device.hpp;
probe_reduce.hip: the launchers of the post-processing kernels of fs_reduce.hpp / fs_envelope.hpp, linked with the library's own
objects; built by `make -C flow-sim_amd/csrc probe`, which __graft_entry__.build() runs).  TEST INFRASTRUCTURE: the product never
loads it.  Arrays go in and come out as numpy arrays of the device type (float64 / float32); a HIP error raises."""
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


STORAGE_OPS = dict(area_at=0, net_vol=1, outflow=2, storage_root=3)


def storage_parts(op, params, dt, a, b=None):
    """one part of the general reservoir row on a shared FS_BC_STORAGE_CURVE parameter block: area_at(a), net_vol(a, b, step),
    outflow(a) or storage_root(Yold = a, vol_in = b, dt, step); returns (value, flag)"""
    D = a.dtype.type
    a = _in(a, D)
    b = np.zeros_like(a) if b is None else _in(b, D)
    p = _in(params, D)
    out = np.empty((2, len(a)), dtype=D)
    _call("fsp_storage_parts", a, STORAGE_OPS[op], p, len(p), D(dt), a, b, out, len(a))
    return out[0], out[1].astype(np.int32)


def bc_general(kind, params, sec, level, dt, h, Q, Qold, Yprev):
    """bc_eval<true> for FS_BC_STORAGE_CURVE / FS_BC_HOST_ROW with the parameters in global memory; params 1-d: shared by all
    elements (stride 0), 2-d [n_params][n]: element i reads column i (stride 1).  Returns res, dh, dq, Ynew, flag"""
    D = h.dtype.type
    arrays = [_in(a, D) for a in (h, Q, Qold, Yprev)]
    p = _in(params, D)
    assert p.ndim == 1 or p.shape[1] == len(h)
    out = np.empty((4, len(h)), dtype=D)
    flag = np.full(len(h), -1, dtype=np.int32)
    _call("fsp_bc_general", arrays[0], kind, p, p.shape[0], p.ndim - 1, HR.sec_array(sec, D), level, D(dt), *arrays, out, flag, len(h))
    return dict(res=out[0], dh=out[1], dq=out[2], Ynew=out[3], flag=flag)


# ---- probe_reduce.hip: the launchers of the post-processing kernels on arrays of the caller's choice ---------------------------
def _ptr(a, dtype):
    if a is None:
        return None
    assert isinstance(a, np.ndarray) and a.flags["C_CONTIGUOUS"] and a.dtype == dtype, (a.dtype, dtype)
    return a.ctypes.data_as(ctypes.c_void_p)


def _run(name, *args):
    """args: (array or None, dtype) pairs go as pointers, Python ints as int"""
    l = lib()
    fn = getattr(l, name)
    fn.restype = ctypes.c_int
    e = fn(*[_ptr(*a) if isinstance(a, tuple) else ctypes.c_int(int(a)) for a in args])
    if e != 0:
        raise RuntimeError(f"{name}: HIP error {e}: {l.fsp_error_string(e).decode()}")


F64, I32 = np.dtype(np.float64), np.dtype(np.int32)


def _block(hydro, status, iters, level, first, n):
    """hydro[levels][4][B] in the device type, status[B], iters[levels][B]; rows 0 .. level exist, the range is [first, first + n)"""
    levels, four, B = hydro.shape
    assert four == 4 and status.shape == (B,) and iters.shape == (levels, B) and 0 <= first and n >= 1 and first + n <= level + 1 <= levels
    return [(hydro, hydro.dtype), (status, I32), (iters, I32), B, levels, level, first, n]


def bands(hydro, status, iters, level, first, n, q):
    """fs::launch_bands: min, max, mean, std [n][4][4], quantiles [n][4][n_q], n_members [n]"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    mom, qu, nm = np.full((n, 4, 4), -7.0), np.full((n, 4, len(q)), -7.0), np.full(n, -7, dtype=np.int32)
    _run(f"fsp_bands_{_suffix(hydro)}", *_block(hydro, status, iters, level, first, n), (q if len(q) else None, F64), len(q), (mom, F64),
         (qu if len(q) else None, F64), (nm, I32))
    return dict(moments=mom, quantiles=qu, n_members=nm)


def profile_bands(x, count, status, levels, reach_nodes, q):
    """fs::launch_profile_bands on x[N][B]: moments [N][4], quantiles [N][n_q], exceed [N], n_members [N]"""
    N, B = x.shape
    q = np.ascontiguousarray(q, dtype=np.float64)
    assert status.shape == (B,) and levels.shape == (B,) and (count is None or count.shape == (N, B)) and (reach_nodes is None or reach_nodes.shape == (B,))
    mom, qu, ex, nm = np.full((N, 4), -7.0), np.full((N, len(q)), -7.0), np.full(N, -7.0), np.full(N, -7, dtype=np.int32)
    _run("fsp_profile_bands", (x, F64), (count, F64), (status, I32), (levels, I32), (reach_nodes, I32), B, N, (q if len(q) else None, F64), len(q),
         (mom, F64), (qu if len(q) else None, F64), (ex if count is not None else None, F64), (nm, I32))
    return dict(moments=mom, quantiles=qu, exceed=ex if count is not None else None, n_members=nm)


def transpose_rows(rows):
    """fs::launch_transpose_rows: one or two [B][N] rows -> [z][N][B]"""
    B, N = rows[0].shape
    assert 1 <= len(rows) <= 2 and all(r.shape == (B, N) for r in rows)
    out = np.full((len(rows), N, B), -7.0)
    _run("fsp_transpose_rows", (rows[0], F64), (rows[1] if len(rows) == 2 else None, F64), len(rows), B, N, (out, F64))
    return out


def summarize(hydro, status, iters, level, first, n):
    """fs::launch_summarize: out[FS_SUM_NROWS][B] (row 0: the rows of the range each reach completed)"""
    out = np.full((14, hydro.shape[2]), -7.0)
    _run(f"fsp_summarize_{_suffix(hydro)}", *_block(hydro, status, iters, level, first, n), (out, F64))
    return out


def lookup(hydro, status, iters, level, first, n, x_row, y_row, xq, y_offset=None, target=None):
    """fs::launch_lookup: values [n_q][B], rmse [B] (with a target), info [B] (bit 0: the abscissae descend somewhere)"""
    B = hydro.shape[2]
    xq = np.ascontiguousarray(xq, dtype=np.float64)
    val, rm, info = np.full((len(xq), B), -7.0), np.full(B, -7.0), np.full(B, -7, dtype=np.int32)
    _run(f"fsp_lookup_{_suffix(hydro)}", *_block(hydro, status, iters, level, first, n), x_row, y_row, (y_offset, F64), (xq, F64), len(xq),
         (target, F64), (val, F64), (rm if target is not None else None, F64), (info, I32))
    return dict(values=val, rmse=rm if target is not None else None, info=info)
