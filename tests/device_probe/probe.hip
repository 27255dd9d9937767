// probe.hip - TEST INFRASTRUCTURE ONLY: thin kernels around the __device__ functions of flow-sim_amd/csrc/fs_device.hpp, so that
// tests/test_gpu_device_helpers.py can run each of them on the device with known inputs.  Not part of libflowsim_hip.so: built as
// tests/device_probe/libfs_probe.so by its own Makefile target, with the library's flags (-ffp-contract=on: the helpers' arithmetic
// follows the source, as it does inside the step kernels).
//
// Every kernel: one thread per element, a bounds check, no data-dependent loop - except the two kernels of the general reservoir row
// (k_storage_parts, k_bc_general), whose functions carry their own: the binary search of area_at over the n_curve breakpoints, the
// trapezoid of net_vol with (int)(|Y2 - Y1| / step) points, and the Brent loop of storage_root, which evaluates the balance at most
// 102 times (two bracket ends and 100 iterations), each evaluation a trapezoid of at most (Y_max - Y_min) / step points when Yold is
// inside the bracket.  The recipes (tests/helper_recipes.py) keep that quotient <= 64; the host wrappers refuse a parameter block
// whose curve does not fit its n_params and a stage that would make a trapezoid of more than kMaxTrapezoid points.
// Every host wrapper takes HOST pointers, allocates, copies in, launches, synchronises, copies out, frees, and returns the first HIP
// error (0 = hipSuccess).  Arrays with several fields per element are field-major: out[f * n + i].
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <type_traits>
#include <vector>
#include "../../flow-sim_amd/csrc/fs_device.hpp"
#include "probe_call.hpp"

namespace {
using namespace fs;
using fsp::Call;
using fsp::kBadArg;

constexpr int kBlock = 256;

// ---- kernels -------------------------------------------------------------------------------------------------------------
enum { OP_FRCP = 0, OP_FRSQ, OP_RCBRT, OP_RCBRT2, OP_FSQRT, OP_P23, OP_P32, OP_PM15, OP_LOG, OP_EXP, OP_COUNT };

template <typename R> __global__ void k_unary(int op, const R *x, R *y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const R v = x[i];
  R r = R(0);
  switch (op) {
    case OP_FRCP: r = frcp(v); break;
    case OP_FRSQ: r = frsq(v); break;
    case OP_RCBRT: r = rcbrt_pos(v); break;
    case OP_RCBRT2: r = rcbrt2_pos(v); break;
    case OP_FSQRT: r = fsqrt_pos(v); break;
    case OP_P23: r = p23_(v); break;
    case OP_P32: r = p32_(v); break;
    case OP_PM15: r = pm15_(v); break;
    default:
      if constexpr (std::is_same<R, double>::value) {
        if (op == OP_LOG) r = log_pos(v);
        else if (op == OP_EXP) r = exp_short(v);
      }
      break;
  }
  y[i] = r;
}

template <typename R> __global__ void k_pow(int op, const R *a, const R *b, R *y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = op == 0 ? pow_pos(a[i], b[i]) : pow_(a[i], b[i]);
}

template <typename R> __global__ void k_k15(const R *A, const R *P, const R *n15, R *y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = k15_(A[i], P[i], n15[i]);
}

// the twelve caller-side section parameters, in the order of the FS_GEO_* rows (z_bed, b_main, m_main, n_main, n_left, n_right,
// is_compound, h_bf, b_fp_l, b_fp_r, m_fp, curvature); the derived members as a single section gets them (sec_derive)
template <typename R> __device__ __forceinline__ SecParams<R> section_from(const R *p) {
  SecParams<R> s;
  s.z = p[0]; s.b = p[1]; s.m = p[2]; s.nm = p[3]; s.nl = p[4]; s.nr = p[5]; s.compound = p[6] > R(0.5);
  s.hbf = p[7]; s.bl = p[8]; s.br = p[9]; s.mfp = p[10]; s.curv = p[11];
  sec_derive(s);
  return s;
}

// form 0: node_terms_rect (b, 1/b, n as Geometry<FS_SEC_RECT_UNIFORM>::init makes them), 1: node_terms_trap (sm2 as
// Geometry<FS_SEC_TRAP_UNIFORM>::init), 2: node_terms_general.  out: A, T, Se, eAT, eQh, v, rT
template <typename R> __global__ void k_node_terms(int form, const R *sec, const R *h, const R *Q, R *out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  NodeTerms<R> t;
  if (form == 0) {
    const R b = sec[1];
    t = node_terms_rect(b, R(1) / b, sec[3], h[i], Q[i]);
  } else if (form == 1) {
    const R m = sec[2];
    t = node_terms_trap(sec[1], m, R(2) * sqrt_(R(1) + m * m), sec[3], h[i], Q[i]);
  } else {
    t = node_terms_general(section_from(sec), h[i], Q[i]);
  }
  const size_t N = (size_t)n;
  out[i] = t.A; out[N + i] = t.T; out[2 * N + i] = t.Se; out[3 * N + i] = t.eAT; out[4 * N + i] = t.eQh; out[5 * N + i] = t.v;
  out[6 * N + i] = t.rT;
}

// out: A, rA, P, Rh, T, rT, K, rK, neq, dRdA, dKdA, dKdA_K, y13
template <typename R> __global__ void k_general_props(const R *sec, const R *h, R *out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const GeneralProps<R> g = general_props(section_from(sec), h[i]);
  const size_t N = (size_t)n;
  out[i] = g.A; out[N + i] = g.rA; out[2 * N + i] = g.P; out[3 * N + i] = g.Rh; out[4 * N + i] = g.T; out[5 * N + i] = g.rT;
  out[6 * N + i] = g.K; out[7 * N + i] = g.rK; out[8 * N + i] = g.neq; out[9 * N + i] = g.dRdA; out[10 * N + i] = g.dKdA;
  out[11 * N + i] = g.dKdA_K; out[12 * N + i] = g.y13;
}

// sec: [n][12] (one section per element); out: sm, sfp, Tb, Am, Pm, rnm, km15, kl15, kr15
template <typename R> __global__ void k_sec_derive(const R *sec, R *out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const SecParams<R> s = section_from(sec + (size_t)i * 12);
  const size_t N = (size_t)n;
  out[i] = s.sm; out[N + i] = s.sfp; out[2 * N + i] = s.Tb; out[3 * N + i] = s.Am; out[4 * N + i] = s.Pm; out[5 * N + i] = s.rnm;
  out[6 * N + i] = s.km15; out[7 * N + i] = s.kl15; out[8 * N + i] = s.kr15;
}

// p: s0, buf, l0, l1, l2, h0, h1, h2
template <typename R> __global__ void k_rating_blend(int rcp, const R *p, const R *z, R *y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = rcp ? rating_blend<true>(z[i], p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7])
             : rating_blend<false>(z[i], p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
}

// form 0: bc_eval<false> on the section `sec`, 1: bc_eval_rect on (b, n, z) of it.  The fixed-size parameters are staged in LDS
// and slot 2 of a normal-depth boundary is derived as the prologue of preissmann_step_kernel does (fs_kernel.hpp): the rows read
// them through an LDS-typed pointer.  out: res, dh, dq, Ynew; flag starts from FS_OK per element
template <typename R>
__global__ void k_bc(int form, int kind, const R *params, const R *sec, int level, R dt, const R *h, const R *Q, const R *Qold,
                     const R *Yprev, const R *tgt, R *out, int *flag, int n) {
  __shared__ R bcp[FS_BC_MAX_PARAMS];
  const int t = threadIdx.x;
  if (t < FS_BC_MAX_PARAMS) {
    bcp[t] = t < bc_param_count(kind) ? params[t] : R(0);
    if (kind == FS_BC_NORMAL_DEPTH && t == 2) {
      const R S0 = params[0];
      bcp[2] = (S0 < R(0) ? R(-1) : R(1)) * sqrt_(fabs_(S0));
    }
  }
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + t;
  if (i >= n) return;
  BCDesc<R> bc;
  bc.kind = kind; bc.stride = 0; bc.params = &bcp[0]; bc.target = nullptr; bc.tgt = tgt[i];
  R Ynew = R(0);
  int fl = FS_OK;
  BCRow<R> r;
  if (form == 0) r = bc_eval<false>(bc, 0, 1, level, section_from(sec), h[i], Q[i], Qold[i], dt, Yprev[i], &Ynew, &fl);
  else r = bc_eval_rect(bc, (LdsParams<R>)bc.params, level, sec[1], sec[3], sec[0], h[i], Q[i], Qold[i], dt, Yprev[i], &Ynew, &fl);
  const size_t N = (size_t)n;
  out[i] = r.res; out[N + i] = r.dh; out[2 * N + i] = r.dq; out[3 * N + i] = Ynew;
  flag[i] = fl;
}

// the smallest gap of the area curve's stages, as bc_storage_curve computes it (1 without a curve)
template <typename R> __device__ __forceinline__ R storage_step(const StorageCurve<R> &sc) {
  R step = R(1);
  for (int j = 0; j + 1 < sc.nc; ++j) {
    const R d = fabs_(sc.xs(j + 1) - sc.xs(j));
    step = j == 0 ? d : (d < step ? d : step);
  }
  return step;
}

// the parts of the general reservoir row on one shared parameter block in global memory (stride 0).  out: value, flag
enum { SOP_AREA = 0, SOP_NET_VOL, SOP_OUTFLOW, SOP_ROOT, SOP_COUNT };

template <typename R> __global__ void k_storage_parts(int op, const R *params, R dt, const R *a, const R *b, R *out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  BCDesc<R> bc;
  bc.kind = FS_BC_STORAGE_CURVE; bc.stride = 0; bc.params = params; bc.target = nullptr; bc.tgt = R(0);
  StorageCurve<R> sc{bc, 0, 1, 0};
  sc.nc = (int)sc.p(FS_SC_N_CURVE);
  int fl = FS_OK;
  R r = R(0);
  switch (op) {
    case SOP_AREA: r = sc.area_at(a[i]); break;
    case SOP_NET_VOL: r = sc.net_vol(a[i], b[i], storage_step(sc)); break;
    case SOP_OUTFLOW: r = sc.outflow(a[i]); break;
    default: r = storage_root(sc, a[i], b[i], dt, storage_step(sc), &fl); break;
  }
  out[i] = r; out[(size_t)n + i] = R(fl);
}

// bc_eval<true> for FS_BC_STORAGE_CURVE and FS_BC_HOST_ROW, parameters in global memory as the step kernels of boundary class -1
// read them: stride 0 (one block, reach 0, B 1) or stride 1 (params[n_params][n], element i reads column i).  out: res, dh, dq, Ynew
template <typename R>
__global__ void k_bc_general(int kind, const R *params, int stride, const R *sec, int level, R dt, const R *h, const R *Q,
                             const R *Qold, const R *Yprev, R *out, int *flag, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  BCDesc<R> bc;
  bc.kind = kind; bc.stride = stride; bc.params = params; bc.target = nullptr; bc.tgt = R(0);
  R Ynew = R(0);
  int fl = FS_OK;
  const BCRow<R> r = bc_eval<true>(bc, stride ? i : 0, stride ? n : 1, level, section_from(sec), h[i], Q[i], Qold[i], dt, Yprev[i], &Ynew, &fl);
  const size_t N = (size_t)n;
  out[i] = r.res; out[N + i] = r.dh; out[2 * N + i] = r.dq; out[3 * N + i] = Ynew;
  flag[i] = fl;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
inline dim3 grid_for(int n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

template <typename R> int unary(int op, const R *x, R *y, int n) {
  if (n <= 0 || op < 0 || op >= OP_COUNT || (!std::is_same<R, double>::value && op >= OP_LOG)) return kBadArg;
  Call c;
  const R *dx = c.in(x, n); R *dy = c.out(y, n);
  if (c.ok()) hipLaunchKernelGGL(k_unary<R>, grid_for(n), dim3(kBlock), 0, 0, op, dx, dy, n);
  return c.finish();
}
template <typename R> int pow2(int op, const R *a, const R *b, R *y, int n) {
  if (n <= 0 || op < 0 || op > 1) return kBadArg;
  Call c;
  const R *da = c.in(a, n), *db = c.in(b, n); R *dy = c.out(y, n);
  if (c.ok()) hipLaunchKernelGGL(k_pow<R>, grid_for(n), dim3(kBlock), 0, 0, op, da, db, dy, n);
  return c.finish();
}
template <typename R> int k15(const R *A, const R *P, const R *n15, R *y, int n) {
  if (n <= 0) return kBadArg;
  Call c;
  const R *dA = c.in(A, n), *dP = c.in(P, n), *dn = c.in(n15, n); R *dy = c.out(y, n);
  if (c.ok()) hipLaunchKernelGGL(k_k15<R>, grid_for(n), dim3(kBlock), 0, 0, dA, dP, dn, dy, n);
  return c.finish();
}
template <typename R> int node_terms(int form, const R *sec, const R *h, const R *Q, R *out, int n) {
  if (n <= 0 || form < 0 || form > 2) return kBadArg;
  Call c;
  const R *ds = c.in(sec, 12), *dh = c.in(h, n), *dQ = c.in(Q, n); R *dout = c.out(out, (size_t)7 * n);
  if (c.ok()) hipLaunchKernelGGL(k_node_terms<R>, grid_for(n), dim3(kBlock), 0, 0, form, ds, dh, dQ, dout, n);
  return c.finish();
}
template <typename R> int props(const R *sec, const R *h, R *out, int n) {
  if (n <= 0) return kBadArg;
  Call c;
  const R *ds = c.in(sec, 12), *dh = c.in(h, n); R *dout = c.out(out, (size_t)13 * n);
  if (c.ok()) hipLaunchKernelGGL(k_general_props<R>, grid_for(n), dim3(kBlock), 0, 0, ds, dh, dout, n);
  return c.finish();
}
template <typename R> int derive(const R *sec, R *out, int n) {
  if (n <= 0) return kBadArg;
  Call c;
  const R *ds = c.in(sec, (size_t)12 * n); R *dout = c.out(out, (size_t)9 * n);
  if (c.ok()) hipLaunchKernelGGL(k_sec_derive<R>, grid_for(n), dim3(kBlock), 0, 0, ds, dout, n);
  return c.finish();
}
template <typename R> int blend(int rcp, const R *p, const R *z, R *y, int n) {
  if (n <= 0) return kBadArg;
  Call c;
  const R *dp = c.in(p, 8), *dz = c.in(z, n); R *dy = c.out(y, n);
  if (c.ok()) hipLaunchKernelGGL(k_rating_blend<R>, grid_for(n), dim3(kBlock), 0, 0, rcp, dp, dz, dy, n);
  return c.finish();
}
template <typename R>
int bc_rows(int form, int kind, const R *params, const R *sec, int level, R dt, const R *h, const R *Q, const R *Qold, const R *Yprev,
            const R *tgt, R *out, int *flag, int n) {
  // the closed-form kinds only, their parameters in LDS: the Brent row and the host row read theirs from global memory and go
  // through bc_general below; bc_eval_rect has no power rating row
  if (n <= 0 || form < 0 || form > 1 || kind < FS_BC_FLOW_HYDROGRAPH || kind > FS_BC_STORAGE) return kBadArg;
  if (form == 1 && kind == FS_BC_RATING_POWER) return kBadArg;
  Call c;
  const R *dp = c.in(params, FS_BC_MAX_PARAMS), *ds = c.in(sec, 12);
  const R *dh = c.in(h, n), *dQ = c.in(Q, n), *dQo = c.in(Qold, n), *dY = c.in(Yprev, n), *dt_ = c.in(tgt, n);
  R *dout = c.out(out, (size_t)4 * n); int *dflag = c.out(flag, n);
  if (c.ok()) hipLaunchKernelGGL(k_bc<R>, grid_for(n), dim3(kBlock), 0, 0, form, kind, dp, ds, level, dt, dh, dQ, dQo, dY, dt_, dout, dflag, n);
  return c.finish();
}

// Host-side guard of the two kernels with data-dependent loops: column `col` of the block holds a curve that fits n_params, with
// ascending finite stages, and a trapezoid from `y` to either bracket end has at most kMaxTrapezoid points (a NaN stage gives n = 0
// on the device and passes).
constexpr int kMaxTrapezoid = 4096;
template <typename R> bool storage_block_ok(const R *params, int n_params, int stride, int B, int col, const R *ys, int n_y) {
  auto p = [&](int i) { return stride ? params[(size_t)i * B + col] : params[i]; };
  if (n_params < FS_SC_NFIXED) return false;
  const R ncr = p(FS_SC_N_CURVE);
  if (!(ncr >= R(0) && ncr <= R(1024))) return false;
  const int nc = (int)ncr;
  if (FS_SC_NFIXED + 2 * nc > n_params) return false;
  R step = R(1);
  for (int j = 0; j + 1 < nc; ++j) {
    const R d = p(FS_SC_NFIXED + j + 1) - p(FS_SC_NFIXED + j);
    if (!(d > R(0))) return false;
    step = j == 0 ? d : (d < step ? d : step);
  }
  if (nc == 0) return true;
  const R lo = p(FS_SC_Y_MIN), hi = p(FS_SC_Y_MAX);
  if (!(hi - lo >= R(0)) || !((hi - lo) / step <= R(kMaxTrapezoid))) return false;
  for (int k = 0; k < n_y; ++k) {
    const R y = ys[k];
    if (y != y) continue;
    if (!(std::fabs(y - lo) / step <= R(kMaxTrapezoid)) || !(std::fabs(y - hi) / step <= R(kMaxTrapezoid))) return false;
  }
  return true;
}

template <typename R> int storage_parts(int op, const R *params, int n_params, R dt, const R *a, const R *b, R *out, int n) {
  if (n <= 0 || op < 0 || op >= SOP_COUNT) return kBadArg;
  if (!storage_block_ok<R>(params, n_params, 0, 1, 0, a, n)) return kBadArg;
  if (op == SOP_NET_VOL && !storage_block_ok<R>(params, n_params, 0, 1, 0, b, n)) return kBadArg;
  Call c;
  const R *dp = c.in(params, n_params), *da = c.in(a, n), *db = c.in(b, n); R *dout = c.out(out, (size_t)2 * n);
  if (c.ok()) hipLaunchKernelGGL(k_storage_parts<R>, grid_for(n), dim3(kBlock), 0, 0, op, dp, dt, da, db, dout, n);
  return c.finish();
}

// stride 0: params[n_params]; stride 1: params[n_params][n]
template <typename R>
int bc_general(int kind, const R *params, int n_params, int stride, const R *sec, int level, R dt, const R *h, const R *Q, const R *Qold,
               const R *Yprev, R *out, int *flag, int n) {
  if (n <= 0 || (kind != FS_BC_STORAGE_CURVE && kind != FS_BC_HOST_ROW) || stride < 0 || stride > 1) return kBadArg;
  if (kind == FS_BC_HOST_ROW && n_params < 3) return kBadArg;
  if (kind == FS_BC_STORAGE_CURVE) {
    for (int i = 0; i < n; ++i) {
      const int col = stride ? i : 0, B = stride ? n : 1;
      if (!storage_block_ok<R>(params, n_params, stride, B, col, nullptr, 0)) return kBadArg;
      const R bed = stride ? params[(size_t)FS_SC_BED_LEVEL * B + col] : params[FS_SC_BED_LEVEL];
      const R yold = level == 1 ? h[i] + bed : Yprev[i];
      if (!storage_block_ok<R>(params, n_params, stride, B, col, &yold, 1)) return kBadArg;
    }
  }
  Call c;
  const R *dp = c.in(params, (size_t)n_params * (stride ? n : 1)), *ds = c.in(sec, 12);
  const R *dh = c.in(h, n), *dQ = c.in(Q, n), *dQo = c.in(Qold, n), *dY = c.in(Yprev, n);
  R *dout = c.out(out, (size_t)4 * n); int *dflag = c.out(flag, n);
  if (c.ok()) hipLaunchKernelGGL(k_bc_general<R>, grid_for(n), dim3(kBlock), 0, 0, kind, dp, stride, ds, level, dt, dh, dQ, dQo, dY, dout, dflag, n);
  return c.finish();
}
}  // namespace

extern "C" {
int fsp_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }
const char *fsp_error_string(int e) { return hipGetErrorString((hipError_t)e); }

#define FSP_BOTH(T, S)                                                                                                          \
  int fsp_unary_##S(int op, const T *x, T *y, int n) { return unary<T>(op, x, y, n); }                                          \
  int fsp_pow_##S(int op, const T *a, const T *b, T *y, int n) { return pow2<T>(op, a, b, y, n); }                              \
  int fsp_k15_##S(const T *A, const T *P, const T *n15, T *y, int n) { return k15<T>(A, P, n15, y, n); }                        \
  int fsp_node_terms_##S(int form, const T *sec, const T *h, const T *Q, T *out, int n) { return node_terms<T>(form, sec, h, Q, out, n); } \
  int fsp_general_props_##S(const T *sec, const T *h, T *out, int n) { return props<T>(sec, h, out, n); }                       \
  int fsp_sec_derive_##S(const T *sec, T *out, int n) { return derive<T>(sec, out, n); }                                        \
  int fsp_rating_blend_##S(int rcp, const T *p, const T *z, T *y, int n) { return blend<T>(rcp, p, z, y, n); }                  \
  int fsp_bc_##S(int form, int kind, const T *params, const T *sec, int level, T dt, const T *h, const T *Q, const T *Qold,     \
                 const T *Yprev, const T *tgt, T *out, int *flag, int n) {                                                      \
    return bc_rows<T>(form, kind, params, sec, level, dt, h, Q, Qold, Yprev, tgt, out, flag, n);                                \
  }                                                                                                                             \
  int fsp_storage_parts_##S(int op, const T *params, int n_params, T dt, const T *a, const T *b, T *out, int n) {               \
    return storage_parts<T>(op, params, n_params, dt, a, b, out, n);                                                            \
  }                                                                                                                             \
  int fsp_bc_general_##S(int kind, const T *params, int n_params, int stride, const T *sec, int level, T dt, const T *h,        \
                         const T *Q, const T *Qold, const T *Yprev, T *out, int *flag, int n) {                                 \
    return bc_general<T>(kind, params, n_params, stride, sec, level, dt, h, Q, Qold, Yprev, out, flag, n);                      \
  }
FSP_BOTH(double, f64)
FSP_BOTH(float, f32)
#undef FSP_BOTH
}
