// fs_init_state.hpp - initial conditions on the device: what Channel.initialize_conditions (channel.py:107-138) builds per channel on
// the host - 'linear', 'GVF_equation' (backwater march), 'steady-state' (normal depth) - for every reach of a batch at once, on the
// geometry the batch already holds.  Sections are evaluated through Geometry<R, SEC> (fs_kernel.hpp), as the step kernels do.
//
// The first part (brent_root) is plain C++: tests/test_init_state_host.py compiles it with the system compiler and holds it to
// scipy.optimize.brentq evaluation by evaluation.  The kernels follow under __HIPCC__; they are instantiated in fs_part_init.hip.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FS_IC_HD __host__ __device__ __forceinline__
#else
#define FS_IC_HD inline
#endif

namespace fs {

// scipy.optimize.brentq with its defaults (xtol 2e-12, rtol 4 eps, 100 iterations; Brent 1973 as arranged in
// scipy/optimize/Zeros/brentq.c: bisection-guarded secant / inverse quadratic extrapolation on a bracketing triple), generic over the
// function.  The caller brings f at both ends - brentq evaluates them first, and an end whose value is known by definition then
// costs nothing.  *bracketed = false: f(xa) and f(xb) have the same sign (brentq's ValueError; also for a NaN) and xb comes
// back.  *evals (optional) counts the evaluations as brentq's full_output does, the two ends included.
template <typename R, typename F>
FS_IC_HD R brent_root(F &&f, R xa, R fa, R xb, R fb, bool *bracketed, int *evals = nullptr) {
  const R xtol = R(2e-12), rtol = R(4) * (sizeof(R) == 8 ? R(2.220446049250313e-16) : R(1.1920929e-7));
  auto mag = [](R v) __attribute__((always_inline)) { return v < R(0) ? -v : v; };
  R xpre = xa, xcur = xb, xblk = R(0);
  R fpre = fa, fcur = fb, fblk = R(0), spre = R(0), scur = R(0);
  int calls = 2;
  *bracketed = true;
  if (evals) *evals = calls;
  if (fpre == R(0)) return xpre;
  if (fcur == R(0)) return xcur;
  if ((fpre < R(0)) == (fcur < R(0)) || !(fpre == fpre) || !(fcur == fcur)) { *bracketed = false; return xb; }
  for (int it = 0; it < 100; ++it) {
    if (fpre != R(0) && fcur != R(0) && ((fpre < R(0)) != (fcur < R(0)))) {
      xblk = xpre; fblk = fpre;
      spre = scur = xcur - xpre;
    }
    if (mag(fblk) < mag(fcur)) {
      xpre = xcur; xcur = xblk; xblk = xpre;
      fpre = fcur; fcur = fblk; fblk = fpre;
    }
    const R delta = (xtol + rtol * mag(xcur)) / R(2);
    const R sbis = (xblk - xcur) / R(2);
    if (fcur == R(0) || mag(sbis) < delta) break;
    if (mag(spre) > delta && mag(fcur) < mag(fpre)) {
      R stry;
      if (xpre == xblk) {
        stry = -fcur * (xcur - xpre) / (fcur - fpre);                                   // secant
      } else {
        const R dpre = (fpre - fcur) / (xpre - xcur), dblk = (fblk - fcur) / (xblk - xcur);
        stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre));     // inverse quadratic
      }
      const R a = mag(spre), c = R(3) * mag(sbis) - delta;
      if (R(2) * mag(stry) < (a < c ? a : c)) { spre = scur; scur = stry; }
      else { spre = sbis; scur = sbis; }
    } else {
      spre = sbis; scur = sbis;
    }
    xpre = xcur; fpre = fcur;
    if (mag(scur) > delta) xcur += scur;
    else xcur += (sbis > R(0) ? delta : -delta);
    fcur = f(xcur);
    ++calls;
  }
  if (evals) *evals = calls;
  return xcur;
}

}  // namespace fs

#if defined(__HIPCC__)
#include "fs_kernel.hpp"
#include "../../include/flowsim_abi.h"

namespace fs {

template <typename R> struct InitArgs {
  KernelArgs<R> k;                   // what Geometry<R, SEC>::init reads, reach_nodes and reach_scheme; hk / Qk receive the state
  int32_t method;                    // FS_IC_*
  const R *flow;                     // [B]
  const R *depth_us, *depth_ds;      // [B] (LINEAR: both, GVF: depth_ds)
  const R *bed_slope;                // STEADY: [N] or [B][N]; nullptr in the uniform modes: (z_us - z_ds) / ((n_r - 1) dx_r)
  int32_t bed_slope_per_reach;
  int32_t *info;                     // [2][B]: FS_IC_* flag bits (zeroed before the launch); node of the first supercritical evaluation (-1)
};

constexpr int kInitTile = 64;        // nodes of the backwater march staged in LDS before they go out as rows
constexpr int kInitLanes = 64;       // reaches per workgroup of the march: one wave, one lane per reach

template <typename R> __device__ __forceinline__ int ic_reach_nodes(const KernelArgs<R> &a, int r) { return a.reach_nodes ? a.reach_nodes[r] : a.N; }
template <typename R> __device__ __forceinline__ R ic_reach_dx(const KernelArgs<R> &a, int r) {
  return a.reach_scheme ? a.reach_scheme[(size_t)2 * a.B + r] : a.dx;
}
template <typename R> __device__ __forceinline__ R ic_nan() { return R(__builtin_nanf("")); }

// dh/dx = (S0 - Se) / (1 - Fr^2) at one node (channel.py:346-366), Fr with the clamp of hydraulics.py:166-168 that is left once
// T >= 1e-6 and A >= 1e-6.  flags: FS_IC_SUPERCRITICAL ends the march, FS_IC_CLAMPED is the reference's warning
template <typename R> __device__ __forceinline__ R ic_gvf_slope(const NodeTerms<R> &t, R Q, R S0, int &flags) {
  if (t.T < R(1e-6) || t.A < R(1e-6)) return R(0);
  const R V = Q / t.A, D = t.A / t.T;
  const R Fr = V / sqrt_(R(kG) * fmax_(D, R(1e-6)));
  if (Fr > R(1)) { flags |= FS_IC_SUPERCRITICAL; return R(0); }
  R den = R(1) - Fr * Fr;
  if (den < R(0.01)) { flags |= FS_IC_CLAMPED; den = R(0.01); }
  return (S0 - t.Se) / den;
}

// A, T and Se of one node for the march.  At a polyline node NodeTerms::T is the section's dA/dh, a central difference over 2e-6 m
// (cross_section.py:533-538) that carries some 5e-10 of rounding noise; the reference's Froude number takes the geometric top width
// (channel.py:350), which the whole-section evaluation has exactly - without it the polyline profiles sat at 0.77 of the tolerance
template <typename R, int SEC> __device__ __forceinline__ NodeTerms<R> ic_march_terms(const Geometry<R, SEC> &geo, int node, R h, R Q) {
  NodeTerms<R> t = geo.terms(node, h, Q);
  if constexpr (SEC == FS_SEC_IRREGULAR) {
    if (geo.hint_init(node) != -2) {
      int ns_;
      t.T = poly_eval_whole(geo.poly(node), h + geo.bed(node), &ns_).T;
    }
  }
  return t;
}

// Backwater march (channel.py:307-378): Heun predictor-corrector from each reach's downstream depth towards its node 0.  The march
// is a serial recurrence, the batch supplies the parallelism: one lane per reach, 64 reaches per workgroup.  A lane's own stores
// would be N * sizeof(R) bytes apart, so the wave stages kInitTile nodes x 64 reaches in LDS and writes them out as rows, consecutive
// lanes on consecutive nodes.  Every lane walks the batch's N nodes from the top; above its own last node a lane idles (and
// holds its downstream depth, the padding fixture batches use).  The two stages of a step share one section evaluation in the
// code: the polyline evaluation is ~420 instructions and sits at the register allocator's edge.
template <typename R, int SEC>
__global__ __launch_bounds__(kInitLanes) void init_backwater_kernel(const InitArgs<R> p) {
  const KernelArgs<R> &a = p.k;
  __shared__ R tile[kInitTile][kInitLanes + 1];
  __shared__ R flows[kInitLanes];
  const int lane = threadIdx.x, B = a.B, N = a.N;
  const int first = blockIdx.x * kInitLanes;
  const bool valid = first + lane < B;
  const int reach = valid ? first + lane : B - 1;
  const int last = ic_reach_nodes(a, reach) - 1;
  const R dx = ic_reach_dx(a, reach), Q = p.flow[reach];
  Geometry<R, SEC> geo;
  geo.init(a, reach, last + 1);
  flows[lane] = Q;
  R h = p.depth_ds[reach];
  int flags = 0, where = -1;
  for (int top = N - 1; top >= 0; top -= kInitTile) {
    const int rows = min(kInitTile, top + 1);
    for (int j = 0; j < rows; ++j) {
      const int i = top - j;                       // the node this pass arrives at
      if (i < last && !(flags & FS_IC_SUPERCRITICAL)) {
        const R S0 = (geo.bed(i) - geo.bed(i + 1)) / dx;       // the interval's slope, predictor and corrector alike (channel.py:344)
        R k1 = R(0), hp = h;
#pragma clang loop unroll(disable)
        for (int s = 0; s < 2 && !(flags & FS_IC_SUPERCRITICAL); ++s) {
          const int node = i + 1 - s;
          const R k = ic_gvf_slope(ic_march_terms(geo, node, s == 0 ? h : hp, Q), Q, S0, flags);
          if (flags & FS_IC_SUPERCRITICAL) { where = node; break; }
          if (s == 0) {
            k1 = k;
            hp = h - k1 * dx;
            if (hp <= R(0)) hp = R(0.01);
          } else {
            h = h - R(0.5) * (k1 + k) * dx;
            if (h <= R(0)) { h = R(0.01); flags |= FS_IC_FLOORED; }
          }
        }
        if (flags & FS_IC_SUPERCRITICAL) h = ic_nan<R>();    // this node and the ones upstream of it were never reached
      }
      tile[j][lane] = h;
    }
    __syncthreads();
    // rows out: reach by reach, lane t on node top - t
    const int nb = min(kInitLanes, B - first);
    for (int rr = 0; rr < nb; ++rr) {
      if (lane < rows) {
        const size_t at = (size_t)(first + rr) * N + (top - lane);
        a.hk[at] = tile[lane][rr];
        a.Qk[at] = flows[rr];
      }
    }
    __syncthreads();
  }
  if (valid) { p.info[reach] = flags; p.info[(size_t)B + reach] = where; }
}

// conveyance of the whole section at water level hw = z_min + depth: what CrossSection.normal_flow multiplies by sqrt(S)
// (cross_section.py:177-182) and the normal-depth boundary rows evaluate (bc_eval, bc_normal_depth_poly)
template <typename R, int SEC> __device__ __forceinline__ R ic_conveyance(const Geometry<R, SEC> &geo, int node, R zmin, R hw) {
  if constexpr (SEC == FS_SEC_IRREGULAR) {
    if (geo.hint_init(node) != -2) {
      int ns_;
      return poly_eval_whole(geo.poly(node), hw, &ns_).K;
    }
  }
  return general_props(geo.section(node), hw - zmin).K;
}

// 'linear' (channel.py:380-390) and 'steady-state' (channel.py:296-305 over cross_section.py:177-202): one thread per (reach, node).
// Nodes beyond a reach's own last one repeat it.
template <typename R, int SEC>
__global__ __launch_bounds__(256) void init_per_node_kernel(const InitArgs<R> p) {
  const KernelArgs<R> &a = p.k;
  const size_t at = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (at >= (size_t)a.B * a.N) return;
  const int reach = (int)(at / a.N), n_r = ic_reach_nodes(a, reach);
  const int node = min((int)(at - (size_t)reach * a.N), n_r - 1);
  const R dx = ic_reach_dx(a, reach), Q = p.flow[reach];
  R h;
  if (p.method == FS_IC_LINEAR) {
    const R h0 = p.depth_us[reach], hN = p.depth_ds[reach];
    const R L = R(n_r - 1) * dx;
    const R x = L * R(node) / R(n_r - 1);
    h = h0 + (hN - h0) * x / L;
  } else {
    Geometry<R, SEC> geo;
    geo.init(a, reach, n_r);
    const R zmin = geo.bed(node);
    R S;
    if (p.bed_slope) S = p.bed_slope[(p.bed_slope_per_reach ? (size_t)reach * a.N : 0) + node];
    else S = (geo.bed(0) - geo.bed(n_r - 1)) / (R(n_r - 1) * dx);       // channel.py:286 (the uniform modes)
    const R hw_max = zmin + R(100);
    const bool sloped = S > R(0);                                        // normal_flow is 0 otherwise (cross_section.py:177-180)
    const R rt = sloped ? sqrt_(S) : R(0);
    auto f = [&](R hw) __attribute__((always_inline)) { return sloped ? Q - ic_conveyance(geo, node, zmin, hw) * rt : Q; };
    bool bracketed;
    // f(z_min) = Q by definition: K = 0 at zero depth
    const R root = brent_root(f, zmin, Q, hw_max, f(hw_max), &bracketed);
    h = root - zmin;
    if (!bracketed) {                                                    // cross_section.py:195-202
      h = Q < R(0) ? R(0) : hw_max - zmin;
      atomicOr(&p.info[reach], (int)FS_IC_NO_ROOT);
    }
  }
  a.hk[at] = h;
  a.Qk[at] = Q;
}

// the launchers (fs_part_init.hip): false when the library has no instantiation for this section mode in this type
bool launch_init_state(int section_mode, const InitArgs<double> &p, hipStream_t stream);
bool launch_init_state(int section_mode, const InitArgs<float> &p, hipStream_t stream);

}  // namespace fs
#endif
