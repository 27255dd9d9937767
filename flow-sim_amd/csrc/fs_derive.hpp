// fs_derive.hpp - the derived fields of a stored history (fs_batch_derive): one stream over the levels, no solver in it.
#pragma once
#include <cstddef>

#include "fs_device.hpp"
#include "fs_poly.hpp"

namespace fs {

// The section tables of a batch as the post-processing kernels read them: the seven geometry members of KernelArgs, nested in
// DeriveArgs, EnvelopeArgs and IntegralArgs where those members used to stand (the kernel-argument offsets are asserted below).
template <typename R> struct SectionTables {
  const R *geo_uniform, *geo_table;
  const R *poly_x, *poly_z;       // IRREGULAR (see KernelArgs)
  const int32_t *poly_n;
  int64_t geo_reach_stride, poly_reach_stride;      // per-reach tables (see KernelArgs), 0: shared
};

// the section of (reach, node) of a batch of B reaches by N node slots; nodes_r: the reach's own node count, as the step kernels'
// Geometry::init(a, reach, n_nodes).  p.n == 0: no polyline at this node.
template <typename R> __device__ __forceinline__ void section_at(const SectionTables<R> &t, int32_t section_mode, int32_t B, int32_t N, size_t reach,
                                                                 int node, int nodes_r, SecParams<R> &s, PolyNode<R> &p) {
  p.n = 0;
  if (section_mode == FS_SEC_TABLE || section_mode == FS_SEC_IRREGULAR) {
    auto g = [&](int row) { return t.geo_table[(size_t)reach * t.geo_reach_stride + (size_t)row * N + node]; };
    s.z = g(FS_GEO_Z_BED); s.b = g(FS_GEO_B_MAIN); s.m = g(FS_GEO_M_MAIN);
    s.compound = g(FS_GEO_IS_COMPOUND) > R(0.5);
    s.hbf = g(FS_GEO_H_BANKFULL); s.bl = g(FS_GEO_B_FP_LEFT); s.br = g(FS_GEO_B_FP_RIGHT); s.mfp = g(FS_GEO_M_FP);
    if (section_mode == FS_SEC_IRREGULAR) {
      const size_t po = (size_t)reach * t.poly_reach_stride, no = t.poly_reach_stride ? (size_t)reach * N : 0;
      if (t.poly_n[no + node] > 0) {
        p.x = t.poly_x + po + node; p.z = t.poly_z + po + node; p.stride = N; p.n = t.poly_n[no + node];
        p.tz = nullptr; p.K = 0; p.KP = 0;
      }
    }
  } else {
    const R z_us = t.geo_uniform[(size_t)FS_RU_Z_US * B + reach], z_ds = t.geo_uniform[(size_t)FS_RU_Z_DS * B + reach];
    const R w2 = R(node) * (R(1) / R(nodes_r - 1));       // the reach's own node count, as Geometry<R, *_UNIFORM>::bed
    s.z = z_us * (R(1) - w2) + z_ds * w2;
    s.b = t.geo_uniform[(size_t)FS_RU_WIDTH * B + reach];
    s.m = section_mode == FS_SEC_TRAP_UNIFORM ? t.geo_uniform[(size_t)FS_TU_SIDE_SLOPE * B + reach] : R(0);
    s.compound = false; s.hbf = s.bl = s.br = s.mfp = R(0);
  }
}

// area and top width of that section at depth h: cross_section.py:623-679 (incl. the over-bank convention), a polyline
// node by cross_section.py:248-328
template <typename R> __device__ __forceinline__ void section_area_top(const SecParams<R> &se, const PolyNode<R> &p, R h, R &Ae, R &Te) {
  const R d = fmax_(R(0), h);
  Te = se.b + R(2) * se.m * d;
  Ae = (se.b + Te) / R(2) * d;
  if (se.compound && d > se.hbf) {
    const R dfp = d - se.hbf, Tb = se.b + R(2) * se.m * se.hbf;
    Ae = (se.b + Tb) / R(2) * se.hbf + (se.bl + R(0.5) * se.mfp * dfp) * dfp + (se.br + R(0.5) * se.mfp * dfp) * dfp;
    Te = (se.bl + Tb + se.br) + R(2) * se.mfp * dfp;
  }
  if (d <= R(0)) { Ae = R(0); Te = R(0); }
  if (p.n > 0) poly_area_top(p, h + se.z, Ae, Te);
}

// ---------------------------------------------------------------------------------------------
// Post-processing (reference: Solver.prepare_results, solver.py:65-127).  One thread per V consecutive
// (reach, node) elements walks the stored levels: 16-byte loads / stores (V = 2 doubles, 4 floats), consecutive
// threads on consecutive elements, 16 B in and up to 56 B out per element - a plain HBM-bound stream.
// ---------------------------------------------------------------------------------------------
template <typename R> struct DeriveArgs {
  int32_t B, N, first, n, section_mode;
  const R *hist_h, *hist_Q;       // [levels][B][N]
  SectionTables<R> sec;
  R *level, *area, *top, *froude, *vel, *cel, *amp, *peak;   // [n][B][N] (peak: [B][N]) or nullptr
  const int32_t *reach_nodes;     // [B] or nullptr: nodes of each reach of a ragged batch (fs_batch_set_reach_nodes); entries beyond come out 0
};
// the kernel-argument layout, as it was when the tables were seven members of the struct itself
#define FS_ARGS_LAYOUT(Args, size, sec_at, after, after_at)                                                                         \
  static_assert(sizeof(Args<double>) == size && offsetof(Args<double>, sec) == sec_at && offsetof(Args<double>, after) == after_at && \
                sizeof(Args<float>) == size && offsetof(Args<float>, sec) == sec_at && offsetof(Args<float>, after) == after_at,     \
                #Args ": the kernel arguments moved")
FS_ARGS_LAYOUT(DeriveArgs, 168, 40, level, 96);

template <typename R, int V> struct Pack { typedef R type __attribute__((ext_vector_type(V))); };

// V elements from / to p: one 16-byte access when the thread's elements all exist and the row is aligned (whole)
template <typename R, int V> __device__ __forceinline__ void load_pack(const R *__restrict__ p, bool whole, int cnt, R (&out)[V]) {
  if (whole) {
    const typename Pack<R, V>::type q = *reinterpret_cast<const typename Pack<R, V>::type *>(p);
#pragma unroll
    for (int e = 0; e < V; ++e) out[e] = q[e];
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) out[e] = e < cnt ? p[e] : R(1);
  }
}
template <typename R, int V> __device__ __forceinline__ void store_pack(R *__restrict__ p, bool whole, int cnt, const R (&in)[V]) {
  if (whole) {
    typename Pack<R, V>::type q;
#pragma unroll
    for (int e = 0; e < V; ++e) q[e] = in[e];
    __builtin_nontemporal_store(q, reinterpret_cast<typename Pack<R, V>::type *>(p));     // written once, read by nobody on the device
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) if (e < cnt) p[e] = in[e];
  }
}

template <typename R, int V> __global__ __launch_bounds__(256) void derive_fields_kernel(const DeriveArgs<R> a) {
  const size_t BN = (size_t)a.B * a.N;
  const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i0 >= BN) return;
  const int cnt = (int)(BN - i0 < (size_t)V ? BN - i0 : (size_t)V);
  const bool whole = cnt == V && BN % V == 0;        // every level's row of this thread starts on a 16-byte boundary
  SecParams<R> s[V];
  PolyNode<R> pnode[V];
  bool beyond[V];                            // ragged batches: a slot past the reach's own node count (no history there: results 0)
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const size_t i = i0 + (e < cnt ? e : 0);
    const int reach = (int)(i / a.N), node = (int)(i - (size_t)reach * a.N);
    const int nodes_r = a.reach_nodes ? a.reach_nodes[reach] : a.N;        // the step kernels' Geometry::init(a, reach, n_nodes)
    beyond[e] = node >= nodes_r;
    section_at(a.sec, a.section_mode, a.B, a.N, reach, node, nodes_r, s[e], pnode[e]);
  }
  R h0[V], peak[V];                          // depth[0] (amplitude reference, solver.py:96-97)
  load_pack<R, V>(a.hist_h + i0, whole, cnt, h0);
#pragma unroll
  for (int e = 0; e < V; ++e) peak[e] = R(-3.0e38);
  for (int k = 0; k < a.n; ++k) {
    const size_t src = (size_t)(a.first + k) * BN + i0, dst = (size_t)k * BN + i0;
    R h[V], Q[V], lev[V], A[V], T[V], Fr[V], vel[V], cel[V], am[V];
    load_pack<R, V>(a.hist_h + src, whole, cnt, h);
    load_pack<R, V>(a.hist_Q + src, whole, cnt, Q);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (beyond[e]) { h[e] = R(1); Q[e] = R(0); }        // (never written by the step kernel)
      const SecParams<R> &se = s[e];
      R Te, Ae;
      section_area_top(se, pnode[e], h[e], Ae, Te);
      const R Ve = Q[e] / Ae;
      lev[e] = h[e] + se.z; A[e] = Ae; T[e] = Te; vel[e] = Ve;
      {                                        // hydraulics.py:155-168 with its clamps
        const R Vc = Q[e] / fmax_(Ae, R(1e-6)), D = Ae / fmax_(Te, R(1e-6));
        Fr[e] = Vc / sqrt_(R(kG) * fmax_(D, R(1e-6)));
      }
      cel[e] = Ve + sqrt_(R(kG) * Ae / Te);
      am[e] = h[e] - h0[e];
      peak[e] = fmax_(peak[e], am[e]);
      if (beyond[e]) { lev[e] = A[e] = T[e] = Fr[e] = vel[e] = cel[e] = am[e] = R(0); peak[e] = R(0); }
    }
    if (a.level) store_pack<R, V>(a.level + dst, whole, cnt, lev);
    if (a.area) store_pack<R, V>(a.area + dst, whole, cnt, A);
    if (a.top) store_pack<R, V>(a.top + dst, whole, cnt, T);
    if (a.froude) store_pack<R, V>(a.froude + dst, whole, cnt, Fr);
    if (a.vel) store_pack<R, V>(a.vel + dst, whole, cnt, vel);
    if (a.cel) store_pack<R, V>(a.cel + dst, whole, cnt, cel);
    if (a.amp) store_pack<R, V>(a.amp + dst, whole, cnt, am);
  }
  if (a.peak) store_pack<R, V>(a.peak + i0, whole, cnt, peak);
}

}  // namespace fs
