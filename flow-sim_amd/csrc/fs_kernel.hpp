// fs_kernel.hpp - the fused Preissmann time-step kernel for gfx950 (MI355X).
//
// One workgroup of W wavefronts advances ONE reach through n_steps time levels; the whole Newton
// loop of a level (residual, Jacobian, linear solve, norm, update - reference
// src/hydromodel/preissmann.py:101-163) runs on chip:
//
//   * lane t owns the M consecutive cells [t*M, (t+1)*M) and keeps their unknowns (h, Q) in
//     registers for the whole launch (M+1 nodes, the last one shared with lane t+1);
//   * the level-(k) halves of the 4-point Preissmann stencil (preissmann.py:899-910) are reduced
//     to 4 constants per cell, kept in LDS, written once per level, read once per iteration;
//   * the 2x2-block banded Jacobian is never materialised: in characteristic-like unknowns the continuity rows
//     are substitutions and the momentum rows one scalar tridiagonal system (fs_device.hpp); each cell's entries
//     (preissmann.py:407-733) are folded straight into the lane's running segment; the 64*W lane segments are
//     reduced by a log-depth tree - DPP moves inside a wave, one LDS mailbox and one barrier across waves - the
//     upstream boundary row closes the system, the separators come back down (every lane carries two numbers of
//     its group and reads the group's record from LDS: no cross-lane traffic) and each lane back-substitutes;
//   * HBM is read once per launch and written at its last level (every level only into an optional
//     history): the accepted iterate of level k (preissmann.py:166-177; SURVEY F2: the pre-update
//     iterate) seeds the level constants of k+1 straight from registers.  Boundary hydrographs and
//     iteration counts go to small per-level tables.
//
// Template parameters: R = float|double, SEC = FS_SEC_*, M = rows per lane (>= 2), W = waves per reach,
// RAGGED = false promises N = 64*W*M: then every row is a cell except the very last one (the downstream
// boundary row) and the per-row selects (and their 64-bit lane masks) disappear;
// BCK (boundary-kind class the kernel is compiled for): -1 = any kinds, 0 = any but FS_BC_STORAGE_CURVE (the row
// evaluation switches at run time),
// 1 = RECT_UNIFORM with bc_is_light() kinds on both ends (closed-form rows, parameters in LDS), 2 + k = flow
// hydrograph upstream and kind k downstream, known at compile time: the switch over the kinds folds away (rows the
// reach never evaluates still cost registers and shape the code around them: flagship +1.5 %, C5 +2-3.5 %).
// fs_dispatch.hpp picks the most specific instantiation that matches the batch.
#pragma once
#include <type_traits>
#include "fs_device.hpp"
#include "fs_poly.hpp"

namespace fs {

// In-kernel phase stamps for diagnostic builds only (never in the shipped library): cycle sums per
// phase of the Newton iteration, one row per wave, written once at the end of the launch.
#ifdef FS_STAMP
#define FS_T(i)                                                         \
  do {                                                                  \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();       \
    stamp_[i] += now_ - tprev_;                                         \
    tprev_ = now_;                                                      \
  } while (0)
#else
#define FS_T(i) do { } while (0)
#endif

template <typename R> __host__ __device__ constexpr R finite_max() { return sizeof(R) == 8 ? R(1.7976931348623157e308) : R(3.4028234e38); }
template <typename R> __host__ __device__ constexpr R eps_of() { return sizeof(R) == 8 ? R(2.220446049250313e-16) : R(1.1920929e-7); }

// Conditioning monitor.  The up row of a segment [a, b) reads  u1 p_a + m_a + u3 m_{b-1} = ru : u3 is the product of
// -(super-diagonal / pivot) over the segment's rows, i.e. how strongly the first unknown of the segment depends on its last
// one.  Subcritical, the rows are diagonally dominant and |u3| decays along the reach (typically 0.2 ... 0.6 over a whole
// reach); with v > c the upstream-travelling characteristic turns round, |u3| grows geometrically with the length of the
// segment, the two-point boundary value problem (one condition per end, boundary.py) is ill-posed and the Jacobian the
// reference hands to SuperLU is ill-conditioned (cond 1e13 ... 1e16 on the draws of profiles/round2/supercritical_scan.txt
// that part from the pivoted CPU solvers).  The kernel keeps the largest |u3| of any segment the tree forms - one integer
// (the high word of the magnitude) carried along with the segment - and raises FS_ILL_CONDITIONED above 2^10 (calibration:
// DESIGN.md section 4.1; every reference-generated near-critical fixture the kernel misses by more than 1e-8 lies above): the reference's
// `diagnos` check (preissmann.py:139-144, rcond < 1e-12 -> ValueError "Jacobian is ill-conditioned") stands behind it.
template <typename R> __host__ __device__ constexpr int growth_limit_bits() { return sizeof(R) == 8 ? ((1023 + 10) << 20) : ((127 + 10) << 23); }

template <typename R> struct KernelArgs {
  int32_t B, N, n_steps, level0, max_iter;
  int32_t iter_budget;     // kernels of boundary class -1 only: > 0 = Newton iterations this launch may spend on a reach (fs_batch_iterate)
  int32_t *it_done;        // [B] with iter_budget: iterations already spent on the open level, -1 once the reach has closed it
  R theta, dt, dx, tol;
  R *hk, *Qk;              // [B][N] accepted state of the current level (in: level0, out: level0+n_steps)
  R *hg, *Qg;              // [B][N] Newton start vector for the next level
  const R *geo_uniform;    // RECT_UNIFORM: [FS_RU_NPARAM][B]
  const R *geo_table;      // TABLE: [FS_GEOX_NROWS][N], shared by the batch, or one such table per reach (geo_reach_stride)
  const R *n_override;     // TABLE: [B] or nullptr
  const R *poly_x, *poly_z;      // IRREGULAR: [P][N] polyline stations / elevations (vertex-major)
  const R *poly_lim;             // IRREGULAR: [2][N] roughness strip limits
  const int32_t *poly_n;         // IRREGULAR: [N] vertex counts (0 = trapezoid-family node of the table)
  BCDesc<R> us, ds;
  R *Yprev;                // [B] storage stage of the current level
  R *stage_hist;           // [levels][B] storage stage per level (boundary.py:126-131)
  R *hydro;                // [levels][4][B]
  int32_t *iters;          // [levels][B]
  int32_t *status;         // [B]
  R *hist_h, *hist_Q;      // [levels][B][N] or nullptr
  R *trace;                // [levels][FS_TRACE_CAP][B] residual norms or nullptr
  unsigned long long *dbg; // diagnostic builds (-DFS_STAMP): [B][16][12] cycle sums per phase, else nullptr
  // ---- round 3 (kept behind the fields above: the benchmark kernels read none of these, and their code - down to the scalar
  // loads of the arguments - stays what it was) ----
  int64_t geo_reach_stride;      // elements between the tables of consecutive reaches (0: one table for the whole batch)
  int64_t poly_reach_stride;     // IRREGULAR: the same for poly_x / poly_z (P * N); poly_lim and poly_n follow with 2 N and N
  // heterogeneous batches (fs_batch_set_reach_*): each reach its own channel length, grid and scheme - what the reference
  // builds per Channel / Solver (channel.py:213-241, solver.py:34-38,53-55)
  const int32_t *reach_nodes;    // [B] or nullptr: nodes of each reach (<= N; N stays the row stride of every [B][N] array)
  const R *reach_scheme;         // [5][B] or nullptr: theta, dt, dx, tolerance, max_iter of each reach
  const int32_t *reach_kinds;    // [2][B] or nullptr: boundary kind of each reach, upstream row then downstream row (kinds <= FS_BC_STORAGE, or FS_BC_HOST_ROW)
  const R *poly_tz;              // IRREGULAR: stage tables (fs_poly.hpp): breakpoints [N][KP], then intervals [P][16][N] pairs
  int32_t poly_K;                // IRREGULAR: P, intervals per node in the stage tables (0: no tables, walk the edges)
  R *kc_scratch;           // long reaches (fs_long.hpp): [B][4][passes * 64 W M] level constants, owned by the batch
  int32_t passes;          // long reaches: passes of 64 W M rows a workgroup makes over its reach
  // ---- round 4: a reach longer than one lane grid as a TEAM of workgroups (kTeam below) ----
  int32_t team_size;             // G: workgroups per reach, member g owns rows [g C, (g + 1) C), C = 64 W M
  R *team_mail;                  // [B][2][G W + 1][kTeamWords] mailboxes of 16-byte (value, tag) words: one slot per (member, wave) + one for the upstream row, per iteration parity
  unsigned long long *team_sync; // [1]: the ticket counter of the launch (zeroed before every launch)
  uint32_t team_epoch;           // the number of this launch among the handle's team launches (>= 1): the high half of every mailbox tag
};
constexpr int kTeamSlots = 64;   // (member, wave) segments of a team: the top tree is one wave wide
// how long a member waits for its team before it gives the reach up (FS_TEAM_STALL): s_memtime ticks, 2.0e9 per second on gfx950 (tools/micro/rates.hip:
// 158 795 ticks in 0.079 ms of HIP-event time).  Eight seconds: a team's members start in ticket order as CUs become free, so the wait is bounded by the
// longest kernel of a co-tenant that holds the CUs meanwhile, not by anything of this library's own
constexpr unsigned long long kTeamPatience = 16000000000ull;

template <typename R, int SEC> struct Geometry;

// A team's mailbox (kTeam in the step kernel): every word is written and read with device-coherent stores and loads (sc1), no
// cache involved that another XCD could not see - so that the exchange needs neither the write-back of the L2 that an agent-scope
// release costs nor the invalidation of an acquire, both whole-cache operations and both on the critical path of every Newton
// iteration of every team (measured: the exchange took 22 600 ticks of a 43 000-tick iteration with them).
// Every mailbox word travels as ONE 16-byte store of (value, tag), tag = (launch, exchange); a reader polls the words themselves
// until every tag is the one it waits for.  No counter, no acknowledged stores, no barrier between posting and counting: the
// exchange is one store flight and the reader's polls.  (A lane's aligned 16-byte access is one request.)
constexpr int kTeamSleep = 1;        // s_sleep between two polls of the mailbox (units of 64 cycles)
typedef unsigned int fs_u4 __attribute__((ext_vector_type(4)));
constexpr int kTeamAuxSc1 = 16;      // cache-policy operand of the raw buffer intrinsics on gfx94x / gfx950: sc1 (device-coherent)
__device__ __forceinline__ void team_put2(__amdgpu_buffer_rsrc_t r, unsigned off, unsigned long long bits, unsigned long long tag) {
  fs_u4 v;
  v.x = (unsigned)bits; v.y = (unsigned)(bits >> 32); v.z = (unsigned)tag; v.w = (unsigned)(tag >> 32);
  __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, kTeamAuxSc1);
}
__device__ __forceinline__ fs_u4 team_get2(__amdgpu_buffer_rsrc_t r, unsigned off) { return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, kTeamAuxSc1); }
__device__ __forceinline__ unsigned long long team_tag(fs_u4 v) { return ((unsigned long long)v.w << 32) | v.z; }
__device__ __forceinline__ unsigned long long team_bits(fs_u4 v) { return ((unsigned long long)v.y << 32) | v.x; }

// the descriptor with its kind pinned to what the instantiation was compiled for (BCK >= 2)
template <int BCK, int SIDE, typename R>
__device__ __forceinline__ BCDesc<R> pinned(const BCDesc<R> &bc) {
  BCDesc<R> d = bc;
  if (BCK >= 2) d.kind = SIDE == 0 ? (int)FS_BC_FLOW_HYDROGRAPH : BCK - 2;
  return d;
}

template <typename R> struct Geometry<R, FS_SEC_RECT_UNIFORM> {
  static constexpr bool kConstT = true;      // dA/dh = b everywhere: no per-node top width to keep
  static constexpr int kEQScale = 2;         // terms().eQh is half of dSe/dQ (node_terms_rect): the fold's hx carries the 2
  R b, rb, n, rn, z_us, z_ds, inv_nm1, dz;
  __device__ __forceinline__ void init(const KernelArgs<R> &a, int reach, int n_nodes) {
    b = a.geo_uniform[(size_t)FS_RU_WIDTH * a.B + reach];
    n = a.geo_uniform[(size_t)FS_RU_MANNING * a.B + reach];
    z_us = a.geo_uniform[(size_t)FS_RU_Z_US * a.B + reach];
    z_ds = a.geo_uniform[(size_t)FS_RU_Z_DS * a.B + reach];
    rb = R(1) / b; rn = R(1) / n;
    inv_nm1 = R(1) / R(n_nodes - 1);
    dz = (z_ds - z_us) * inv_nm1;
  }
  __device__ __forceinline__ R bed_step(int) const { return dz; }   // bed(node+1) - bed(node)
  __device__ __forceinline__ R terms_T() const { return b; }
  __device__ __forceinline__ R rT_const() const { return rb; }
  // distance-weighted interpolation between the two end sections (cross_section.py:887-900)
  __device__ __forceinline__ R bed(int node) const {
    const R w2 = R(node) * inv_nm1;
    return z_us * (R(1) - w2) + z_ds * w2;
  }
  __device__ __forceinline__ NodeTerms<R> terms(int, R h, R Q) const { return node_terms_rect(b, rb, n, h, Q); }
  __device__ __forceinline__ SecParams<R> section(int node) const {
    SecParams<R> s;
    s.z = bed(node); s.b = b; s.m = R(0); s.nm = n; s.nl = n; s.nr = n; s.hbf = R(0);
    s.bl = R(0); s.br = R(0); s.mfp = R(0); s.curv = R(0); s.compound = false;
    s.sm = R(1); s.rnm = rn; s.sfp = R(1); s.Tb = b; s.Am = R(0); s.Pm = b; s.km15 = s.kl15 = s.kr15 = R(0);   // (not compound: unused)
    return s;
  }
  template <int BCK, int SIDE>
  __device__ __forceinline__ BCRow<R> boundary(const BCDesc<R> &bc, int reach, int B, int level, int node, R h, R Q,
                                               R Qold, R dt, R Yprev, R *Ynew, int *flag) const {
    // closed-form rows, bc.params points at the LDS copy made in the kernel prologue (fixed-size kinds only); with the kinds
    // fixed at compile time the rows this reach never evaluates are not compiled in (the flagship kernel: +1.5 %)
    if (BCK == 1 || (BCK >= 2 && bc_is_light(BCK - 2)))
      return bc_eval_rect(pinned<BCK, SIDE>(bc), (LdsParams<R>)bc.params, level, b, n, node == 0 ? z_us : z_ds, h, Q, Qold, dt, Yprev, Ynew, flag);
    return bc_eval<BCK != 0>(pinned<BCK, SIDE>(bc), reach, B, level, section(node), h, Q, Qold, dt, Yprev, Ynew, flag);
  }
};

template <typename R> struct Geometry<R, FS_SEC_TRAP_UNIFORM> {
  static constexpr bool kConstT = false;
  static constexpr int kEQScale = 2;         // (node_terms_trap: as the rectangle)
  R b, m, sm2, n, rn, z_us, z_ds, inv_nm1, dz;
  __device__ __forceinline__ void init(const KernelArgs<R> &a, int reach, int n_nodes) {
    b = a.geo_uniform[(size_t)FS_RU_WIDTH * a.B + reach];
    n = a.geo_uniform[(size_t)FS_RU_MANNING * a.B + reach];
    rn = R(1) / n;
    z_us = a.geo_uniform[(size_t)FS_RU_Z_US * a.B + reach];
    z_ds = a.geo_uniform[(size_t)FS_RU_Z_DS * a.B + reach];
    m = a.geo_uniform[(size_t)FS_TU_SIDE_SLOPE * a.B + reach];
    sm2 = R(2) * sqrt_(R(1) + m * m);
    inv_nm1 = R(1) / R(n_nodes - 1);
    dz = (z_ds - z_us) * inv_nm1;
  }
  __device__ __forceinline__ R bed_step(int) const { return dz; }
  __device__ __forceinline__ R terms_T() const { return R(0); }      // unused (kConstT == false)
  __device__ __forceinline__ R rT_const() const { return R(0); }
  __device__ __forceinline__ R bed(int node) const {
    const R w2 = R(node) * inv_nm1;
    return z_us * (R(1) - w2) + z_ds * w2;
  }
  __device__ __forceinline__ NodeTerms<R> terms(int, R h, R Q) const { return node_terms_trap(b, m, sm2, n, h, Q); }
  __device__ __forceinline__ SecParams<R> section(int node) const {
    SecParams<R> s;
    s.z = bed(node); s.b = b; s.m = m; s.nm = n; s.nl = n; s.nr = n; s.hbf = R(0);
    s.bl = R(0); s.br = R(0); s.mfp = R(0); s.curv = R(0); s.compound = false;
    s.sm = R(0.5) * sm2; s.rnm = rn; s.sfp = R(1); s.Tb = b; s.Am = R(0); s.Pm = b; s.km15 = s.kl15 = s.kr15 = R(0);   // (not compound: unused)
    return s;
  }
  template <int BCK, int SIDE>
  __device__ __forceinline__ BCRow<R> boundary(const BCDesc<R> &bc, int reach, int B, int level, int node, R h, R Q,
                                               R Qold, R dt, R Yprev, R *Ynew, int *flag) const {
    return bc_eval<BCK != 0>(pinned<BCK, SIDE>(bc), reach, B, level, section(node), h, Q, Qold, dt, Yprev, Ynew, flag);
  }
};

template <typename R> struct Geometry<R, FS_SEC_TABLE> {
  static constexpr bool kConstT = false;
  static constexpr int kEQScale = 1;         // node_terms_general hands over dSe/dQ itself in eQh (the curvature term is added to it)
  const R *tab;
  int N;
  R n_over, rn_over, k15_over;      // per-reach main-channel Manning n (ensembles), its reciprocal and its -1.5 power
  bool has_over;
  __device__ __forceinline__ void init(const KernelArgs<R> &a, int reach, int) {
    tab = a.geo_table + (size_t)reach * a.geo_reach_stride; N = a.N;       // (N: the row stride of the table)
    has_over = a.n_override != nullptr;
    n_over = has_over ? a.n_override[reach] : R(1);
    rn_over = R(1) / n_over; k15_over = pm15_(n_over);
  }
  __device__ __forceinline__ R terms_T() const { return R(0); }      // unused (kConstT == false)
  __device__ __forceinline__ R rT_const() const { return R(0); }
  __device__ __forceinline__ R bed_step(int node) const {
    return tab[(size_t)FS_GEO_Z_BED * N + min(node + 1, N - 1)] - tab[(size_t)FS_GEO_Z_BED * N + min(node, N - 1)];
  }
  __device__ __forceinline__ R bed(int node) const { return tab[(size_t)FS_GEO_Z_BED * N + node]; }
  __device__ __forceinline__ SecParams<R> section(int node) const {
    SecParams<R> s;
    auto g = [&](int row) { return tab[(size_t)row * N + node]; };
    s.z = g(FS_GEO_Z_BED); s.b = g(FS_GEO_B_MAIN); s.m = g(FS_GEO_M_MAIN);
    s.nm = has_over ? n_over : g(FS_GEO_N_MAIN);
    s.nl = g(FS_GEO_N_LEFT); s.nr = g(FS_GEO_N_RIGHT);
    s.compound = g(FS_GEO_IS_COMPOUND) > R(0.5);
    s.hbf = g(FS_GEO_H_BANKFULL); s.bl = g(FS_GEO_B_FP_LEFT); s.br = g(FS_GEO_B_FP_RIGHT);
    s.mfp = g(FS_GEO_M_FP); s.curv = g(FS_GEO_CURVATURE);
    s.sm = g(FS_GEOX_SM); s.sfp = g(FS_GEOX_SFP); s.Tb = g(FS_GEOX_TB); s.Am = g(FS_GEOX_AM); s.Pm = g(FS_GEOX_PM);
    s.rnm = has_over ? rn_over : g(FS_GEOX_RNM); s.km15 = has_over ? k15_over : g(FS_GEOX_KM15);
    s.kl15 = g(FS_GEOX_KL15); s.kr15 = g(FS_GEOX_KR15);
    return s;
  }
  __device__ __forceinline__ NodeTerms<R> terms(int node, R h, R Q) const {
    return node_terms_general(section(node), h, Q);
  }
  template <int BCK, int SIDE>
  __device__ __forceinline__ BCRow<R> boundary(const BCDesc<R> &bc, int reach, int B, int level, int node, R h, R Q,
                                               R Qold, R dt, R Yprev, R *Ynew, int *flag) const {
    return bc_eval<BCK != 0>(pinned<BCK, SIDE>(bc), reach, B, level, section(node), h, Q, Qold, dt, Yprev, Ynew, flag);
  }
};

// TABLE plus polyline nodes (IrregularSection): per node either a row of the trapezoid table or a
// polyline; both evaluations are inlined (out of line they spill the caller around every call).
template <typename R>
__device__ __forceinline__ NodeTerms<R> node_terms_general_call(const SecParams<R> s, R h, R Q) { return node_terms_general(s, h, Q); }

template <typename R> struct Geometry<R, FS_SEC_IRREGULAR> {
  static constexpr bool kConstT = false;
  static constexpr int kEQScale = 1;
  Geometry<R, FS_SEC_TABLE> tb;
  const R *px, *pz, *plim, *ptz;
  const int32_t *pn;
  int pK;
  __device__ __forceinline__ void init(const KernelArgs<R> &a, int reach, int n_nodes) {
    tb.init(a, reach, n_nodes);
    const bool own = a.poly_reach_stride != 0;
    px = a.poly_x + (size_t)reach * a.poly_reach_stride; pz = a.poly_z + (size_t)reach * a.poly_reach_stride;
    plim = a.poly_lim + (own ? (size_t)reach * 2 * a.N : 0); pn = a.poly_n + (own ? (size_t)reach * a.N : 0);
    pK = a.poly_K;                                     // stage tables: N * poly_table_stride(P) numbers per reach (or shared)
    ptz = pK ? a.poly_tz + (own ? (size_t)reach * a.N * poly_table_stride(pK) : 0) : nullptr;
  }
  __device__ __forceinline__ R terms_T() const { return R(0); }
  __device__ __forceinline__ R rT_const() const { return R(0); }
  __device__ __forceinline__ R bed_step(int node) const { return tb.bed_step(node); }
  __device__ __forceinline__ R bed(int node) const { return tb.bed(node); }
  __device__ __forceinline__ SecParams<R> section(int node) const { return tb.section(node); }
  // the node's slot in the interval part of the stage tables (behind the [N][KP] breakpoints; fs_poly.hpp)
  __device__ __forceinline__ const R *table_slot(int node) const { return ptz + (size_t)tb.N * poly_table_bp(pK) + 2 * (size_t)node; }
  __device__ __forceinline__ PolyNode<R> poly(int node) const {
    PolyNode<R> p;
#ifdef FS_BOUNDS
    node = (int)FS_CHK(16, node, tb.N);
#endif
    const int N = tb.N;
    typedef const __attribute__((address_space(1))) R *GlobalR;              // (device memory: global loads, not flat ones)
    typedef const __attribute__((address_space(1))) int32_t *GlobalI;
    auto g = [&](int row) { return ((GlobalR)tb.tab)[(size_t)row * N + node]; };
    p.x = px + node; p.z = pz + node; p.stride = N; p.n = ((GlobalI)pn)[node];
    p.nl = g(FS_GEO_N_LEFT); p.nm = tb.has_over ? tb.n_over : g(FS_GEO_N_MAIN); p.nr = g(FS_GEO_N_RIGHT);
    p.liml = ((GlobalR)plim)[node]; p.limr = ((GlobalR)plim)[N + node];
    p.curv = g(FS_GEO_CURVATURE); p.zmin = g(FS_GEO_Z_BED);
    p.K = pK; p.KP = poly_table_bp(pK);
    p.tz = ptz ? ptz + (size_t)node * p.KP : nullptr; p.tco = ptz ? table_slot(node) : nullptr; p.cstride = N;
    return p;
  }
  __device__ __forceinline__ NodeTerms<R> terms(int node, R h, R Q) const {
    if (((const __attribute__((address_space(1))) int32_t *)pn)[node] > 0) return node_terms_poly(poly(node), h, Q);
    return node_terms_general_call(section(node), h, Q);
  }
  // The same starting from the table interval of the node's last evaluation (fs_poly.hpp: node_terms_poly_hinted).  kh is the
  // caller's per-row hint: -2 a node without a polyline, -1 nothing to start from, >= 0 the interval.
  __device__ __forceinline__ int hint_init(int node) const {
    return ((const __attribute__((address_space(1))) int32_t *)pn)[node] > 0 ? -1 : -2;
  }
  __device__ __forceinline__ static TermsHint<R> terms_scan(const Geometry g, int node, R h, R Q) {
    TermsHint<R> r;
    r.t = node_terms_poly(g.poly(node), h, Q, &r.k, &r.bc);
    return r;
  }
  // (The paths beside the hinted one take the node index through an empty asm: everything they derive from it - a dozen row
  // addresses of the parameter table, the polyline's station pointers - is loop-invariant, and the compiler otherwise computes it
  // ahead of the time loop and keeps it in registers the Newton loop does not have: they went to scratch, and the hinted path
  // fetched its own table pointer and interval from scratch ahead of every evaluation, a memory round trip in front of the one it needs.)
  __device__ __forceinline__ static int opaque(int node) { asm volatile("" : "+v"(node)); return node; }
  __device__ __forceinline__ NodeTerms<R> terms_hinted(int node, R h, R Q, int &kh, PolyBC<R> &bc) const {
#ifdef FS_BOUNDS
    node = (int)FS_CHK(15, node, tb.N);
    if (kh >= 0) kh = (int)FS_CHK(14, kh, pK);
#endif
    if (kh == -2) return node_terms_general_call(section(opaque(node)), h, Q);
    return node_terms_poly_hinted(table_slot(node), tb.N, tb.has_over, tb.n_over, kh, h, Q, bc,
                                  [&]() { return terms_scan(*this, opaque(node), h, Q); });
  }
  // (No device function of this library is called out of line.  Until round 3 the kernels with many rows per lane called the
  // polyline evaluation, and the edge walk behind the stage tables was a call everywhere: the compiler's interprocedural register
  // allocation then trusted a register summary of the callee that did not hold - the (8, 1) polyline kernel returned wrong numbers
  // from the second level on, or not, depending on unrelated code around the call, the (8, 4) one faulted, and both are correct
  // with -mllvm -enable-ipra=0.  Inlined, nothing is left to summarise; the kernels are also faster: (2, 1) +8 %, (8, 1) +16 %,
  // (8, 4) +32 % on the polyline ensemble, profiles/round3/polyline_calls.txt.)
  template <int BCK, int SIDE>
  __device__ __forceinline__ BCRow<R> boundary(const BCDesc<R> &bc_, int reach, int B, int level, int node, R h, R Q,
                                               R Qold, R dt, R Yprev, R *Ynew, int *flag) const {
    const BCDesc<R> bc = pinned<BCK, SIDE>(bc_);
    if (pn[node] > 0 && bc.kind == FS_BC_NORMAL_DEPTH)
      return bc_normal_depth_poly(poly(node), ((LdsParams<R>)bc.params)[0], ((LdsParams<R>)bc.params)[1], h, Q);   // (LDS copy, as bc_eval)
    if (BCK != 0 && pn[node] > 0 && bc.kind == FS_BC_STORAGE_CURVE) {
      const PolyNode<R> nd = poly(node);
      int ns_;
      const PolyEval<R> er = poly_eval_whole(nd, nd.zmin + h, &ns_);
      const PolyEval<R> ed = poly_eval_whole(nd, h + bc_param(bc, FS_SC_BED_LEVEL, reach, B), &ns_);
      EntryProps<R> pr{er.A, er.Rh, er.neq, er.dRdA, er.dAdh}, pd{ed.A, ed.Rh, ed.neq, ed.dRdA, ed.dAdh};
      return bc_storage_curve(bc, reach, B, level, pr, pd, h, Q, Qold, dt, Yprev, Ynew, flag);
    }
    return bc_eval<BCK != 0>(bc, reach, B, level, section(node), h, Q, Qold, dt, Yprev, Ynew, flag);
  }
};

// LDS carve-up for one reach
// (A, Se, Q/A) of the nodes as the last fold saw them (kSaveTerms); an empty base otherwise
template <typename R, int M, int T, bool SAVE> struct SavedTerms { R nt[3][M + 1][T]; };
template <typename R, int M, int T> struct SavedTerms<R, M, T, false> {};

// what a team member needs on top (kTeam): the records of the top tree over the team's (member, wave) segments and its results
template <typename R, bool TEAM> struct TeamSmem {
  R xtree[4][64];          // records of the top tree (wave 0 of every member computes it, redundantly)
  R xres[kTeamSlots][4];   // per (member, wave): p of its first row, m of its last row, m of its first row, m of the next one's first row
  R xtot;
  int32_t xwarn, xflagT, xstall, xjob;
};
template <typename R> struct TeamSmem<R, false> {};

template <typename R, int M, int W, bool SAVE, bool TEAM = false, int XA = alignof(R)> struct Smem : SavedTerms<R, M, 64 * W, SAVE>, TeamSmem<R, TEAM> {
  static constexpr int T = 64 * W;
  R kc[4][M][T];           // per-cell level-k constants, lane-minor (conflict-free ds_read_b64)
  R tree[W][4][64];        // per-wave records of the in-wave tree (Elim: 4 numbers per merge, 63 merges)
  alignas(XA) R xseg[2][W][8];         // wave segments, double-buffered by iteration parity
  alignas(XA) R xbc[2][4];             // upstream boundary row on (p_0, m_0): aU, bU, rU
  R bcp[2][FS_BC_MAX_PARAMS];   // this reach's boundary parameters (fixed-size kinds), read every Newton iteration
  alignas(XA) R xnorm[2][W];
  int32_t xflag[2];
  int32_t xg[2][W];        // conditioning monitor: high word of the largest |u3| of each wave's tree
};

// What back-substitution needs for row j of a lane's chunk: m_{j-1} = R3 - R1 p_a - R2 m_j (the running down row at the
// time row j was added, divided by its pivot).  The continuity residual rc_{j-1} that turns m_{j-1} into p_j is
// recomputed from the still un-updated state when the top width is constant (kConstT), else it is kept in qc.
template <typename R> struct LocalElim { Parked<R> R1, R2, R3, qc; };

// Minimum number of waves per SIMD a kernel is compiled for: caps its registers at 512 / n.  One wave per SIMD cannot
// hide the latency of the in-wave tree, a second one is worth 20-80 % wherever the kernel fits 256 registers or nearly
// does; forcing it on the larger kernels sends them to scratch (measured 0.25-0.8x).
template <typename R, int SEC, int M, int W, int BCK, bool TEAM = false> constexpr int min_waves() {
  constexpr int kTeamWpe = 2;      // team kernels with <= 8 rows per lane: two workgroups per CU (one computes while the other waits for its team)
  if (TEAM && M <= 8 && sizeof(R) == 8) return kTeamWpe;
  if (W > 1) return 1;          // multi-wave table kernels with 2 cells per lane at two waves per SIMD: no better than the 4- and 8-cell ones
  constexpr int kWpeW1F32Uniform = 3; // fp32, uniform geometry, <= 8 cells per lane: 207 registers capped at 168, three waves per SIMD (C5 +14 %; four: -24 %)
  constexpr int kWpeW1F32 = 2;        // the other fp32 kernels: two waves per SIMD fit (<= 256 registers) and hide the tree's latency (C5 fp32 +18 %)
  if (sizeof(R) == 4) return (M <= 8 && (SEC == FS_SEC_RECT_UNIFORM || SEC == FS_SEC_TRAP_UNIFORM)) ? kWpeW1F32Uniform : kWpeW1F32;
  constexpr int kWpeRect8 = 2;        // rectangular fast-path kernels with <= 8 cells per lane: the ragged (8,1) one needs 310 registers, capped at 256 it runs two waves per SIMD (+21 % at N = 300)
  if (SEC == FS_SEC_RECT_UNIFORM && BCK >= 1 && M <= 8) return kWpeRect8;
  constexpr int kWpePinnedShort = 2;  // kernels with the boundary kinds fixed at compile time and <= 2 cells per lane: as the table kernels below
  if (BCK >= 2 && M <= 2) return kWpePinnedShort;
  constexpr int kWpeLeanShort = 2;    // fp64 table kernels of class 0 with <= 2 cells per lane: 314 registers capped at 256, two waves per SIMD (C4 +43 %)
  if (BCK == 0 && M <= 2 && SEC == FS_SEC_TABLE) return kWpeLeanShort;
  constexpr int kWpeTrap4 = 2;        // trapezoid kernels with 4 cells per lane: 348 registers capped at 256 (+29 % at N = 200; the table kernel of that shape, 406 registers, loses 20 % when capped)
  if (BCK == 0 && M == 4 && SEC == FS_SEC_TRAP_UNIFORM) return kWpeTrap4;
  constexpr int kWpeLeanPoly = 2;     // the same for the polyline kernels (332 registers capped at 256: +79 % on the polyline ensemble)
  if (BCK == 0 && M <= 2 && SEC == FS_SEC_IRREGULAR) return kWpeLeanPoly;
  constexpr int kWpeW1 = 1;           // the other one-wave-per-reach kernels (2..4 measured: scratch spills, 0.25-0.8x)
  return kWpeW1;
}

// Rows of the scalar system (fs_device.hpp): row k is the momentum row of cell k for k < N-1, the downstream boundary row
// for k = N-1 and an identity row (m_k = 0) beyond; lane t owns rows [t M, (t+1) M) and holds the nodes t M .. (t+1) M.
// RAGGED = false promises N = 64 W M: every row is a cell but the very last one, which is the boundary row.
// DIAG = false: no per-level history and no residual trace (batches created without FS_FLAG_HISTORY / FS_FLAG_TRACE): the
// stores are never executed there, but compiled in they cost the flagship kernel 1.1 %
// TAIL >= 0 (ragged one-wave kernels only; round 4): "every row a cell except in the tail lanes".  The batch's N is not the lane grid's,
// but the position of the downstream boundary row inside its lane is known at compile time (local row TAIL = (N - 1) mod M), so the
// per-row selects of the ragged form are gone: every row is assembled as a cell; in local row TAIL one select per number - taken by
// the ONE lane that owns node N - 1 - puts the boundary row in; the rows beyond it are not replaced by identity rows but left as the
// cells of clamped, frozen copies of node N - 1 ("phantom" cells: finite, diagonally dominant, and behind a boundary row whose
// super-diagonal is zero, so nothing upstream of it ever reads them - the real unknowns get the very bits of the ragged kernel);
// two lane masks hoisted out of the time loop keep the phantom rows out of the residual norm and the phantom nodes where they are.
// TEAM (round 4): a reach LONGER than one lane grid (N > 64 W M rows) advanced by a team of G = a.team_size workgroups, each holding
// C = 64 W M rows of it on chip exactly as a short reach is held - unknowns in registers, level constants in LDS, HBM read once per
// launch and written once - where the multi-pass kernel (fs_long.hpp) streams the Newton vector through memory twice per iteration.
// What the W waves of one workgroup exchange through LDS (step 4) the G W waves of a team exchange through a mailbox in device
// memory: every wave posts its segment as tagged words, polling for the tags of the exchange stands where the barrier
// stood, wave 0 of every member reduces the G W segments with one more DPP tree (the multi-pass kernel's top tree: identity segments
// pad the 64 lanes), closes the root with the upstream row and hands every wave its four numbers back through LDS.  All members
// see the same numbers and take the same decisions (convergence, failure, monitor), so the time loop needs no other exchange.
// Membership is by TICKET, not by blockIdx: a workgroup takes the next (reach, member) job when it starts, so the members of the
// oldest unfinished team are exactly the workgroups that started first - all resident, whatever order the dispatcher chose and
// whatever else runs on the device; a team therefore never waits for a workgroup that cannot start (no co-residency assumption
// beyond G <= CUs).  A wait that still exceeds kTeamPatience (16e9 ticks of s_memtime) ends the reach with FS_TEAM_STALL instead of spinning on.
template <typename R, int SEC, int M, int W, bool RAGGED = true, int BCK = 0, bool DIAG = true, int TAIL = -1, bool TEAM = false>
__global__ __launch_bounds__(64 * W, (min_waves<R, SEC, M, W, BCK, TEAM>())) void preissmann_step_kernel(const KernelArgs<R> a) {
  static_assert(M >= 2, "a lane's segment needs two rows (its up and its down row)");
  constexpr bool kTail = TAIL >= 0;
  constexpr bool kTeam = TEAM;
  static_assert(!kTeam || (W > 1 && BCK >= 0 && !kTail), "team form: multi-wave kernels, boundary kinds of the device");
  static_assert(!kTail || (RAGGED && W == 1 && TAIL < M && SEC == FS_SEC_TABLE && BCK >= 2), "tail-only form: ragged one-wave table kernels compiled for a boundary pair");
  constexpr int T = 64 * W;
  using Geo = Geometry<R, SEC>;
  // Short general-section kernels keep (A, Se, Q/A) of every node of the current fold in LDS: if the iterate is accepted they
  // are the node terms of level k, and the level constants of level k+1 come from them instead of from another pass over the
  // sections (1 of 6 section passes of the polyline ensemble, 1 of 11 of C4)
  constexpr int kSaveTermsMaxMF64 = 2;       // 4 and 8 cells per lane measured: trapezoid -13 % / -3 %, table +1 % (the LDS traffic of every fold outweighs one pass per level)
  constexpr bool kSaveTerms = !Geometry<R, SEC>::kConstT && (M <= 2 || (sizeof(R) == 8 && M <= kSaveTermsMaxMF64));
  // table kernels with 2 rows per lane: the section parameters of the lane's three nodes are loaded once per launch instead of
  // at every node evaluation (46 vector loads per Newton iteration, their latency only half hidden by the second wave of the
  // SIMD): C4 +8.5 %, the general table kernel +11.6 %, still within the 256-register cap (20 spilled registers)
  constexpr bool kRegGeo = SEC == FS_SEC_TABLE && W == 1 && M <= 2;
  // kernels compiled for a boundary pair evaluate the two rows in every lane, without a branch (step 1 below)
  constexpr bool kFlatBC = BCK >= 2 && sizeof(R) == 8 && SEC == FS_SEC_TRAP_UNIFORM;   // measured: C5 fp64 +1.5 %; flagship -1.5 %, C4 -7 %, polyline -1.3 %
  // Full lane grids of the rectangular fp64 kernels with 16 rows per lane (the flagship and its one- and two-wave siblings; round 9,
  // profiles/round9/fold_reads.txt): the fold is ONE straight-line block - the downstream boundary row enters the last lane's last
  // row by selects, not behind a branch - and the 4 M level constants are read from LDS kFoldAhead cells ahead of the cell that uses
  // them.  Behind the branch the compiler sank every cell's arithmetic into one block and left all 4 M reads in front of it, under one
  // wait, live in 128 registers from the first cell on: 366 registers against 344, 46 issue slots per iteration more, flagship -2.5 %.
  // Distance 0 / 1 / 2 / 3 measured +2.3 / +1.9 / +2.5 / +2.4 %.  With 8 rows per lane the selects cost more slots than the moves they
  // save (census); the ragged, team, polyline and fp32 forms keep their code.
  constexpr bool kFoldFlat = !RAGGED && !kTeam && !kTail && sizeof(R) == 8 && SEC == FS_SEC_RECT_UNIFORM && M >= 16;
  constexpr int kFoldAhead = 2;
  // ... and there the posted segments, the upstream row and the norms are 16-byte aligned: the cross-wave step reads them as ds_read_b128
  // instead of ds_read2_b64 pairs, all four waves at once right behind the barrier (flagship +1.9 % on top)
  constexpr int kXAlign = kFoldFlat ? 16 : alignof(R);
  __shared__ Smem<R, M, W, kSaveTerms, kTeam, kXAlign> sm;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int job = blockIdx.x;
  if constexpr (kTeam) {      // the next job in order of ARRIVAL (see above)
    if (t == 0) sm.xjob = (int)__hip_atomic_fetch_add(a.team_sync, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    job = sm.xjob;
  }
  const int G = kTeam ? a.team_size : 1;
  const int reach = kTeam ? job / G : job, member = kTeam ? job - reach * G : 0;
  const int gt = member * T + t;                 // the lane's place in the reach's lane grid (t itself unless the reach is a team's)
  // the reach's mailbox of one iteration parity as a raw buffer ((G W + 1) slots of kTeamWords (value, tag) pairs: fs_dispatch.hpp)
  auto mbox = [&](int par) __attribute__((always_inline)) {
    const size_t bytes = team_mailbox_bytes(G, W);
    char *base = reinterpret_cast<char *>(a.team_mail) + ((size_t)reach * 2 + par) * bytes;
    return __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)bytes, 0x27000);
  };
  // One Newton iteration per launch for batches with host-evaluated boundary rows (FS_BC_HOST_ROW, fs_batch_iterate): the
  // kernels of boundary class -1 carry an iteration budget and the count of the open level across launches.
  constexpr bool kBudget = (BCK == -1);
  int it_entry = 0;
  if (kBudget && a.iter_budget > 0) {
    it_entry = a.it_done[reach];
    if (it_entry < 0) return;                 // this reach has closed the level: it waits for the others (whole workgroup)
  }
  // nodes of this reach; NS = a.N stays the row stride of every [B][N] array (heterogeneous batches: RAGGED kernels only)
  const int NS = a.N;
  const int N = (RAGGED && a.reach_nodes) ? a.reach_nodes[reach] : a.N, NC = N - 1;
  const int s0 = gt * M;                      // first node / row of this lane
  // lane (of the reach's lane grid: gt) that owns node N-1 and the downstream boundary row ...  (the non-team forms spelled out as they
  // always were: the flagship's code is sensitive, at the 1 % level, to how its constants come about - profiles/round4/README.md)
  const int tD = RAGGED ? NC / M : (kTeam ? G * T - 1 : T - 1);
  const int jD = kTail ? TAIL : (RAGGED ? NC - tD * M : M - 1);   // ... as its local node / row jD (0..M-1; tail-only form: fs_abi.hip picks the instantiation with TAIL = NC mod M)
  // tail-only form: 1.0 in the lanes up to / before the one that owns node N - 1, else 0.0 (multiplied in, never selected on)
  const R mle = (kTail && gt > tD) ? R(0) : R(1), mlt = (kTail && gt >= tD) ? R(0) : R(1);
  const size_t base = (size_t)reach * NS;

  Geo geo;
  geo.init(a, reach, N);
  // node terms of the lane's local node j (0..M); kRegGeo: from section parameters loaded once per launch
  SecParams<R> secs[kRegGeo ? M + 1 : 1];
  if constexpr (kRegGeo) {
#pragma unroll
    for (int j = 0; j <= M; ++j) secs[j] = geo.section(min(s0 + j, N - 1));
  }
  // polyline nodes: the stage-table interval each of the lane's nodes was last evaluated in (Geometry::terms_hinted)
  constexpr int kPolyHintMaxM = 8;
  constexpr bool kHinted = SEC == FS_SEC_IRREGULAR && M <= kPolyHintMaxM;
  int khint[kHinted ? M + 1 : 1];
  PolyBC<R> polybc[kHinted ? M + 1 : 1];      // (K, dK/dA, dA/dh) of the lane's nodes as last evaluated: the fused normal-depth row below
  if constexpr (kHinted) {
#pragma unroll
    for (int j = 0; j <= M; ++j) {
      khint[j] = geo.hint_init(min(s0 + j, N - 1));
      polybc[j].K = R(0); polybc[j].dKdA = R(0); polybc[j].dAdh = R(0);
    }
  }
  auto terms_at = [&](int j, R hh, R QQ) __attribute__((always_inline)) {
    if constexpr (kRegGeo) return node_terms_general(secs[j], hh, QQ);
    else if constexpr (kHinted) return geo.terms_hinted(min(s0 + j, N - 1), hh, QQ, khint[j], polybc[j]);
    else return geo.terms(min(s0 + j, N - 1), hh, QQ);
  };

  const bool own_scheme = BCK <= 0 && a.reach_scheme != nullptr;          // (the kernels compiled for one boundary pair are the benchmark shapes)
  const R th = own_scheme ? a.reach_scheme[reach] : a.theta, dt = own_scheme ? a.reach_scheme[(size_t)a.B + reach] : a.dt;
  const R dx_ = own_scheme ? a.reach_scheme[(size_t)2 * a.B + reach] : a.dx;
  // (tolerance and iteration cap of the reach's own run(), preissmann.py:101: read where they are used, so that the kernels compiled for one
  // boundary pair - own_scheme is false at compile time there - keep the code they had)
  auto tol_of = [&]() __attribute__((always_inline)) -> R { if constexpr (BCK <= 0) { if (own_scheme) return a.reach_scheme[(size_t)3 * a.B + reach]; } return a.tol; };
  auto max_iter_of = [&]() __attribute__((always_inline)) -> int { if constexpr (BCK <= 0) { if (own_scheme) return (int)a.reach_scheme[(size_t)4 * a.B + reach]; } return a.max_iter; };
  R r2dt = R(1) / (R(2) * dt);
  const R Tr2dt = geo.terms_T() * r2dt;        // constant top width: T/(2dt), the weight of h_j + h_{j+1} in the continuity residual (rc_of below)
  R cq = th / dx_;                            // theta/dx
  const R cqk = (R(1) - th) / dx_;            // (1-theta)/dx
  R hth = R(0.5) * th;
  const R hthk = R(0.5) * (R(1) - th);
  R g = R(kG);
  // scalings into the characteristic-like unknowns p = t dh + cq dQ, m = t dh - cq dQ (t = T/(2dt), fs_device.hpp):
  // 1/(2t) = dt/T, 1/(2cq), and the quotient of the two time / space weights k = (1/(2dt)) / (2cq)
  R i2c = R(0.5) / cq;
  R kap = r2dt * i2c;
  R dtcq = dt * cq;
  R hx = R(Geo::kEQScale) * (hth * i2c);      // (theta/2) / (2cq), times the 2 that the fast paths' eQ leaves out
  R ghth = g * hth;                           // the level constant kc2 carries the factor g as well: g Abar in one fma
  const R ghthk = g * hthk;
  R ghdt = g * hth * dt;

  // ---- unknowns of this lane: nodes s0 .. s0+M (clamped copies beyond the last node) ----
  R h[M + 1], Q[M + 1];
  R QoldD = R(0);                              // flow[k] at the last node (vol_in of the storage BC)

  // level-k constants of the 4-point stencil from the accepted state (h, Q) of level k:
  //   C = [sumA]/(2dt) + cq*dQ                 + kc0
  //   M = [sumQ]/(2dt) + cq*d(Q^2/A)           + kc1 + (g*hth*sumA + kc2)*(cq*dh + hth*sumSe + kc3)     (kc2 carries g)
  // kc3 = cqk*(dz + dh_k) + hthk*sumSe_k + cq*dz: the bed step's share of the level-(k+1) water-surface slope cq*dY = cq*(dz + dh) is a constant of
  // the cell and rides in kc3 (two instructions per cell and iteration fewer; the table kernels also lose the fold's two bed loads per cell)
  // Node s0 + M is lane + 1's node s0 (both lanes hold bitwise equal copies of its unknowns): with one wave per reach the
  // neighbour's terms arrive by a wave rotate.  Lane 63 receives lane 0's, which only a padding row or the downstream boundary
  // row ever looks at (and discards): the lane grid holds N rows, so lane 63's last row is never a cell, and its node M is a
  // clamped copy beyond the reach.  (Until round 3 lane 63 evaluated that node itself whenever the reach filled the wave - a
  // whole section evaluation per iteration, executed by 64 lanes for a result nobody read: a quarter of the polyline ensemble's
  // instructions.)
  // So: one-wave-per-reach kernels with general sections take the neighbour's node terms (12 DPP moves) instead of evaluating
  // the node a second time.
  constexpr bool kShareNode = W == 1 && !Geo::kConstT;
  auto last_node_terms = [&](const NodeTerms<R> &first) __attribute__((always_inline)) {
    auto rol = [](R v) { return dpp_mov<0x134>(v); };     // wave_rol:1
    NodeTerms<R> r;
    r.A = rol(first.A); r.T = rol(first.T); r.Se = rol(first.Se); r.eAT = rol(first.eAT); r.eQh = rol(first.eQh); r.v = rol(first.v);
    r.rT = rol(first.rT);
    return r;
  };
  auto write_level_constants = [&](const R(&hh)[M + 1], const R(&QQ)[M + 1]) __attribute__((always_inline)) {
    NodeTerms<R> L = terms_at(0, hh[0], QQ[0]);
    NodeTerms<R> Rlast;
    if (kShareNode) Rlast = last_node_terms(L);
#pragma unroll
    for (int c = 0; c < M; ++c) {
      const NodeTerms<R> Rn = (kShareNode && c == M - 1) ? Rlast : terms_at(c + 1, hh[c + 1], QQ[c + 1]);
      const R sumA = L.A + Rn.A;
      // explicit fmas only (no a*b + c left to the compiler's choice): this code has two instances, ahead of the time loop and at acceptance
      // inside it, and chunked stepping / a restart gives the bits of one launch only if both compile to the same arithmetic (-ffp-contract=on, Makefile)
      sm.kc[0][c][t] = fma_(cqk, QQ[c + 1] - QQ[c], -(sumA * r2dt));
      sm.kc[1][c][t] = fma_(cqk, fma_(QQ[c + 1], Rn.v, -(QQ[c] * L.v)), -((QQ[c + 1] + QQ[c]) * r2dt));
      sm.kc[2][c][t] = ghthk * sumA;
      const R dzc = geo.bed_step(s0 + c);
      sm.kc[3][c][t] = fma_(cqk, dzc + (hh[c + 1] - hh[c]), fma_(hthk, L.Se + Rn.Se, cq * dzc));
      L = Rn;
    }
  };
  auto save_terms = [&](int j, const NodeTerms<R> &nt) __attribute__((always_inline)) {
    if constexpr (kSaveTerms) { sm.nt[0][j][t] = nt.A; sm.nt[1][j][t] = nt.Se; sm.nt[2][j][t] = nt.v; }
  };
  auto level_constants_from_saved = [&](const R(&hh)[M + 1], const R(&QQ)[M + 1]) __attribute__((always_inline)) {
    if constexpr (kSaveTerms) {
      R A0 = sm.nt[0][0][t], Se0 = sm.nt[1][0][t], v0 = sm.nt[2][0][t];
#pragma unroll
      for (int c = 0; c < M; ++c) {
        const R A1 = sm.nt[0][c + 1][t], Se1 = sm.nt[1][c + 1][t], v1 = sm.nt[2][c + 1][t];
        const R sumA = A0 + A1;
        sm.kc[0][c][t] = fma_(cqk, QQ[c + 1] - QQ[c], -(sumA * r2dt));
        sm.kc[1][c][t] = fma_(cqk, fma_(QQ[c + 1], v1, -(QQ[c] * v0)), -((QQ[c + 1] + QQ[c]) * r2dt));
        sm.kc[2][c][t] = ghthk * sumA;
        const R dzc = geo.bed_step(s0 + c);
        sm.kc[3][c][t] = fma_(cqk, dzc + (hh[c + 1] - hh[c]), fma_(hthk, Se0 + Se1, cq * dzc));
        A0 = A1; Se0 = Se1; v0 = v1;
      }
    }
  };

#pragma unroll
  for (int j = 0; j <= M; ++j) {
    const int node = min(s0 + j, N - 1);
    h[j] = a.hg[base + node];  Q[j] = a.Qg[base + node];
  }
  // per-lane base pointers: every later access is base + immediate offset
  R *const hk_p = a.hk + base + s0, *const Qk_p = a.Qk + base + s0;
  R *const hg_p = a.hg + base + s0, *const Qg_p = a.Qg + base + s0;

  // Boundary descriptors of this reach: the parameters of the fixed-size kinds are copied to LDS once
  // (the boundary rows are evaluated every Newton iteration on the critical path of the first and the
  // last wave; a global load there costs more than the row itself), the hydrograph value of a level
  // is fetched when the level starts.
  BCDesc<R> usd = a.us, dsd = a.ds;
  if (BCK <= 0 && a.reach_kinds) { usd.kind = a.reach_kinds[reach]; dsd.kind = a.reach_kinds[(size_t)a.B + reach]; }
  if (t < 2 * FS_BC_MAX_PARAMS) {
    const int side = t / FS_BC_MAX_PARAMS, i = t - side * FS_BC_MAX_PARAMS;
    // (a reference and the kind next to it, not a copy of the descriptor with the kind patched in: the copy cost the flagship
    // kernel 1.2 % - seven more scalar loads inside its loops and 18 more AGPR moves - for code it never executes)
    const BCDesc<R> &src = side ? a.ds : a.us;
    const int skind = side ? dsd.kind : usd.kind;
    if (skind <= FS_BC_STORAGE && i < bc_param_count(skind)) sm.bcp[side][i] = bc_param(src, i, reach, a.B);
    if (skind == FS_BC_NORMAL_DEPTH && i == 2) {        // derived: sign(S0) sqrt|S0| (hydraulics.py:4-13)
      const R S0 = bc_param(src, 0, reach, a.B);
      sm.bcp[side][2] = (S0 < R(0) ? R(-1) : R(1)) * sqrt_(fabs_(S0));
    }
  }
  if (usd.kind <= FS_BC_STORAGE) { usd.params = &sm.bcp[0][0]; usd.stride = 0; }
  if (dsd.kind <= FS_BC_STORAGE) { dsd.params = &sm.bcp[1][0]; dsd.stride = 0; }

  // Normal depth at a polyline node N-1 whose boundary bed level is the section's own z_min (boundary.py:80, :161-181 then
  // evaluate residual and derivative at the same stage): the row is K, dK/dA, dA/dh of node N-1 at the iterate - exactly what
  // the fold's evaluation of that node has just produced.  The row is then written in the fold, from that evaluation, and the
  // boundary's own section evaluation (a whole wave waiting on one lane: three dependent fetches and ~600 instructions per
  // Newton iteration, a third of the polyline ensemble's time) is not made.
  bool fuseD = false;
  R fuse_sg = R(1), fuse_rt = R(0);
  if constexpr (kHinted && !kFlatBC) {
    __syncthreads();                                    // (sm.bcp written above)
    if (pinned<BCK, 1>(dsd).kind == FS_BC_NORMAL_DEPTH && geo.hint_init(N - 1) != -2 && sm.bcp[1][1] == geo.bed(N - 1)) {
      fuseD = true;
      const R S0 = sm.bcp[1][0];
      fuse_sg = S0 < R(0) ? R(-1) : R(1); fuse_rt = sqrt_(fabs_(S0));
    }
  }
  // a compile-time constant in the kernels compiled for a boundary pair
  const bool ds_storage = BCK >= 2 ? bc_is_storage(BCK - 2) : bc_is_storage(dsd.kind);
  R Yprev = (ds_storage && gt == tD) ? a.Yprev[reach] : R(0);
  int status = a.status[reach];
  // FS_ILL_CONDITIONED is a warning that sticks to the reach, not a failure: the run goes on (and a later launch finds it here)
  constexpr bool kMonitor = DIAG;             // (what the monitor would cost the no-diagnostics flagship kernel: profiles/round3/README.md)
  bool warn = status == FS_ILL_CONDITIONED;
  if (warn) status = FS_OK;
  int parity = 0;
  int exchanges = 0;                          // team form: exchanges made in this launch (the low half of the mailbox tags)
  if (t == 0) { sm.xflag[0] = 0; sm.xflag[1] = 0; }
  __syncthreads();

  {   // accepted state of the entry level -> 4 constants per cell in LDS (a second instance of the acceptance block's code)
    R hk[M + 1], Qk[M + 1];
#pragma unroll
    for (int j = 0; j <= M; ++j) {
      const int node = min(s0 + j, N - 1);
      hk[j] = a.hk[base + node]; Qk[j] = a.Qk[base + node];
    }
    if (gt == tD) {
#pragma unroll
      for (int j = RAGGED ? 0 : M - 1; j < M; ++j) if (j == jD) QoldD = Qk[j];
    }
    write_level_constants(hk, Qk);
  }
#ifdef FS_STAMP
  unsigned long long stamp_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tprev_ = __builtin_amdgcn_s_memtime();
#endif
  for (int step = 0; step < a.n_steps && status == FS_OK; ++step) {
    const int level = a.level0 + step + 1;
    if (usd.target) usd.tgt = usd.target[(size_t)level * a.B + reach];
    if (dsd.target) dsd.tgt = dsd.target[(size_t)level * a.B + reach];
    int it = kBudget ? it_entry : 0;
    int budget = (kBudget && a.iter_budget > 0) ? a.iter_budget : 0x7fffffff;
    bool converged = false;
    R Ynew = Yprev;
    while (!converged && status == FS_OK) {
      // the update, pending until the acceptance block is through, as the two sums it is made of: dh = p + m and
      // dQ = p - m of the node; the scalings 1/(2t) and 1/(2cq) are applied with the addition, one fma per unknown
      R dh[M + 1], dQ[M + 1];
      if (kBudget && budget-- <= 0) break;
      ++it;
      if constexpr (BCK <= 0) { if (it - 1 >= max_iter_of()) { status = FS_MAX_ITER; break; } }
      else
      if (it - 1 >= a.max_iter) { status = FS_MAX_ITER; break; }     // preissmann.py:124-126
      parity ^= 1;
      bool grow = false;                        // conditioning monitor: this iteration's segments grew past the limit
      FS_T(7);

      // opaque lane offset (an integer, so the accesses stay LDS ds_read, not flat): the 4*M level
      // constants are Newton-loop invariants and would otherwise be hoisted into registers
      int kco = t;
      asm volatile("" : "+v"(kco));
      // the same for the lane number the tree-slot addresses derive from: as loop invariants the addresses
      // are hoisted and spilled to scratch, and every reload is a full memory round trip inside the tree
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const R *kcb = &sm.kc[0][0][0] + kco;
      // second half of the constants from a base of its own: beyond 64 KB a ds_read has no immediate offset left, and every
      // one of those loads would come with an address add (32 per iteration in the 4096-node kernels)
      int kco2 = kco + 2 * M * T;
      if constexpr (4 * M * T * sizeof(R) > 65536) asm volatile("" : "+v"(kco2));
      const R *kcb2 = &sm.kc[0][0][0] + kco2;

      // ================= 1. boundary rows (boundary.py:56-242) =================
      // lane 0: the upstream row on (dh_0, dQ_0); the lane of node N-1: the downstream row, which is row N-1 of the
      // scalar system and enters that lane's fold below like any other row
      BCRow<R> Urow, Drow;
      Drow.dh = R(1); Drow.dq = R(0); Drow.res = R(0);
      R nrm2 = R(0);
      int myflag = 0;                          // team form: the flag a storage row raised in this lane (the only value: FS_STORAGE_RANGE)
      if constexpr (kFlatBC) {
        // Boundary kinds fixed at compile time: EVERY lane evaluates both rows, on its own numbers, as straight-line code;
        // only lane 0 / the lane of node N-1 keep what comes out.  A wave executes a divergent branch for one lane at the
        // price of all 64 anyway - but a branch is a block of its own, and the row's dependent chain (a pow, a conveyance)
        // then runs alone at dependent-issue latency ahead of the fold; as straight-line code it is scheduled into the first
        // cell's independent work.  Pays only in the one-wave-per-SIMD trapezoid kernel (C5 fp64 +2 %), see kFlatBC.
        R dummy = R(0), YnewAll = Yprev;
        int fU = 0, fD = 0;
        Urow = geo.template boundary<BCK, 0>(usd, reach, a.B, level, 0, h[0], Q[0], R(0), dt, R(0), &dummy, &fU);
        R hD = h[0], QD = Q[0];
#pragma unroll
        for (int j = RAGGED ? 1 : M - 1; j < M; ++j) if (j == jD) { hD = h[j]; QD = Q[j]; }
        Drow = geo.template boundary<BCK, 1>(dsd, reach, a.B, level, N - 1, hD, QD, QoldD, dt, Yprev, &YnewAll, &fD);
        const bool isD = gt == tD;
        nrm2 = (gt == 0 ? Urow.res * Urow.res : R(0)) + (isD ? Drow.res * Drow.res : R(0));
        if (isD) {
          Ynew = YnewAll;
          if (fD) sm.xflag[parity] = fD;
        }
      } else {
        if (gt == 0) {
          R dummy; int flag = 0;
          Urow = geo.template boundary<BCK, 0>(usd, reach, a.B, level, 0, h[0], Q[0], R(0), dt, R(0), &dummy, &flag);
          nrm2 = Urow.res * Urow.res;
        }
        if (gt == tD && !fuseD) {
          R hD = h[0], QD = Q[0];
          int flag = 0;
#pragma unroll
          for (int j = RAGGED ? 1 : M - 1; j < M; ++j) if (j == jD) { hD = h[j]; QD = Q[j]; }
          Drow = geo.template boundary<BCK, 1>(dsd, reach, a.B, level, N - 1, hD, QD, QoldD, dt, Yprev, &Ynew, &flag);
          nrm2 += Drow.res * Drow.res;
          if (flag) sm.xflag[parity] = flag;
          if (kTeam && flag) myflag = flag;
        }
      }
      FS_T(1);

      // ================= 2. local assembly + fold (registers only) =================
      LocalElim<R> el[M - 1];
      R iTn[Geo::kConstT ? 1 : M + 1];           // dt / T = 1/(2t) of the nodes, only when the top width varies
      Seg<R> seg;                                 // running rows of the lane's segment
      seg.u1 = R(0); seg.u3 = R(-1); seg.ru = R(0);
      R rcLast = R(0);                            // rc of the lane's last row (links node M: p_M = rc - m_{M-1})
      // one-wave fp64 kernels: the root segment and the upstream row meet through v_readlane instead of an LDS round trip
      // (C5 fp64 +5.5 %, polyline ensemble +2.8 %, C4 +1.9 %; fp32: -0.5 %, left as it was)
      constexpr bool kW1Lanes = W == 1 && !kTeam && sizeof(R) == 8;
      R xb0 = R(0), xb1 = R(0), xb2 = R(0);      // kW1Lanes: the upstream row, valid in lane 0
      {
        NodeTerms<R> L = terms_at(0, h[0], Q[0]);
        NodeTerms<R> Rlast;
        if (kShareNode) Rlast = last_node_terms(L);
        save_terms(0, L);
        R i2tL = dt * L.rT;
        if (!Geo::kConstT) iTn[0] = i2tL;
        if (gt == 0) {                          // upstream row on (p_0, m_0): aU p_0 + bU m_0 = -res
          const R x = Urow.dh * i2tL, y = Urow.dq * i2c;
          if constexpr (kTeam) {                // (a team's: into the mailbox, next to the segments)
            const unsigned o = (unsigned)(G * W) * kTeamWords * 16u;
            const unsigned long long tg = ((unsigned long long)a.team_epoch << 32) | (unsigned)(exchanges + 1);
            const __amdgpu_buffer_rsrc_t mb = mbox(parity);
            team_put2(mb, o, __double_as_longlong((double)(x + y)), tg); team_put2(mb, o + 16, __double_as_longlong((double)(x - y)), tg);
            team_put2(mb, o + 32, __double_as_longlong((double)(-Urow.res)), tg);
          } else if constexpr (kW1Lanes) {
            xb0 = x + y; xb1 = x - y; xb2 = -Urow.res;
          } else {
          sm.xbc[parity][0] = x + y; sm.xbc[parity][1] = x - y; sm.xbc[parity][2] = -Urow.res;
          }
        }
        R rcPrev = R(0);
        R kq[kFoldFlat ? M : 1][4];               // kFoldFlat: the level constants of the cells, requested kFoldAhead cells ahead
        auto read_kc = [&](int c) __attribute__((always_inline)) {
          if constexpr (kFoldFlat) {
            kq[c][0] = kcb[(0 * M + c) * T]; kq[c][1] = kcb[(1 * M + c) * T]; kq[c][2] = kcb2[(0 * M + c) * T]; kq[c][3] = kcb2[(1 * M + c) * T];
          }
        };
        if constexpr (kFoldFlat) {
#pragma unroll
          for (int c = 0; c < kFoldAhead; ++c) read_kc(c);
        }
#pragma unroll
        for (int c = 0; c < M; ++c) {
          R k0, k1, k2, k3;
          if constexpr (kFoldFlat) {
            if (c + kFoldAhead < M) read_kc(c + kFoldAhead);      // (never past kc[3][M-1]; all of them behind the level pass: this iteration's fold)
            k0 = kq[c][0]; k1 = kq[c][1]; k2 = kq[c][2]; k3 = kq[c][3];
          } else {
            k0 = kcb[(0 * M + c) * T]; k1 = kcb[(1 * M + c) * T]; k2 = kcb2[(0 * M + c) * T]; k3 = kcb2[(1 * M + c) * T];
          }
          const NodeTerms<R> Rn = (kShareNode && c == M - 1) ? Rlast : terms_at(c + 1, h[c + 1], Q[c + 1]);
          save_terms(c + 1, Rn);
          const R i2tR = dt * Rn.rT;
          if (!Geo::kConstT) iTn[c + 1] = i2tR;
          Row<R> row;
          {
            const R sumA = L.A + Rn.A;
            const R Cres = sumA * r2dt + cq * (Q[c + 1] - Q[c]) + k0;                            // :220-249
            const R gA = fma_(ghth, sumA, k2);                                                    // g Abar
            const R S = fma_(cq, h[c + 1] - h[c], fma_(hth, L.Se + Rn.Se, k3));                  // (cq dz: in k3)
            const R Mres = (Q[c + 1] + Q[c]) * r2dt + cq * (Q[c + 1] * Rn.v - Q[c] * L.v) + k1 + gA * S;   // :251-301
            // momentum entries (preissmann.py:496-733) scaled by 1/(2t) of their node (dh) and 1/(2cq) (dQ):
            //   X0 = pm0 dt/T0, Y0 = pm1/(2cq), X1 = sm0 dt/T1, Y1 = sm1/(2cq)
            const R gAdt = gA * dt, gAx = gA * hx, sdt = ghdt * S;
            const R X0 = fma_(gAdt, fma_(hth, L.eAT, -(cq * L.rT)), fma_(dtcq, L.v * L.v, sdt));      // :558-612
            const R X1 = fma_(gAdt, fma_(hth, Rn.eAT, cq * Rn.rT), fma_(-dtcq, Rn.v * Rn.v, sdt));    // :496-550
            const R Y0 = fma_(gAx, L.eQh, kap - L.v);                                                 // :677-733
            const R Y1 = fma_(gAx, Rn.eQh, kap + Rn.v);                                               // :619-675
            const R ga = X1 + Y1;
            row.al = X0 + Y0; row.D = (X0 - Y0) - ga; row.de = X1 - Y1;
            row.rho0 = fma_(ga, Cres, -Mres);             // qm - ga rc with qm = -Mres, rc = -Cres
            row.rc = -Cres;
            // (Round 5 measured the norm as two fmas into the running sum where the row is a cell in every lane, and Mres as nested
            // fmas: the 62 fp64 instructions they save per iteration came back as AGPR moves and copies - 3 196.3 issue slots with them,
            // 3 188.3 without, 364 registers against 362 - and the flagship ran 0.3 % SLOWER with the two than without; DESIGN.md
            // section 10, profiles/round5/fold_diet.txt.  Both stay as they were.)
            R r2 = fma_(Cres, Cres, Mres * Mres);
            if constexpr (kTail) {
              if (c == TAIL) {                 // the boundary row, in the one lane that owns node N - 1 (its residual was added in step 1)
                const bool isD = gt == tD;
                const R x = Drow.dh * i2tL, y = Drow.dq * i2c;
                row.al = isD ? x + y : row.al; row.D = isD ? x - y : row.D; row.de = isD ? R(0) : row.de;
                row.rho0 = isD ? -Drow.res : row.rho0; row.rc = isD ? R(0) : row.rc;
              }
              nrm2 = fma_(r2, c < TAIL ? mle : mlt, nrm2);    // cells only: not the boundary row, not the phantom cells behind it
            } else if constexpr (kFoldFlat) {
              // full lane grid: the one row that is not a cell is the last row of the last lane, the downstream boundary row.  Put in by
              // selects, not behind a branch: the branch ends the block, the arithmetic of every cell sinks behind it and the fences
              // between the cells then hold nothing but the constants' reads (all 4 M of them ahead of the first row)
              if (c == M - 1) {
                const bool cell = t != T - 1;
                const R x = Drow.dh * i2tL, y = Drow.dq * i2c;
                const R bal = x + y, bD = x - y;
                r2 = cell ? r2 : R(0);
                row.al = cell ? row.al : bal; row.D = cell ? row.D : bD; row.de = cell ? row.de : R(0);
                row.rho0 = cell ? row.rho0 : -Drow.res; row.rc = cell ? row.rc : R(0);
              }
            } else
            // rows beyond the cells: the downstream boundary row (on p and m of node N-1), then identity rows
            if (RAGGED || c == M - 1) {
              const int k = s0 + c;
              const bool cell = RAGGED ? (k < NC) : (kTeam ? gt != G * T - 1 : t != T - 1);      // (k = s0 + c counts along the whole reach)
              const bool bcr = RAGGED ? (k == NC) : true;
              if (!cell) {
                BCRow<R> Dr = Drow;
                r2 = R(0);
                if constexpr (kHinted) {
                  if (fuseD) {                 // normal depth from the fold's own evaluation of node N-1 (= the row's left node)
                    Dr = normal_depth_row_poly(fuse_sg, fuse_rt, polybc[c].K, polybc[c].dKdA, polybc[c].dAdh, Q[c]);
                    r2 = bcr ? Dr.res * Dr.res : R(0);
                  }
                }
                const R x = Dr.dh * i2tL, y = Dr.dq * i2c;
                row.al = bcr ? x + y : R(0); row.D = bcr ? x - y : R(1); row.de = R(0);
                row.rho0 = bcr ? -Dr.res : R(0); row.rc = R(0);
              }
            }
            if constexpr (!kTail) nrm2 += r2;
          }
          if (c == 0) {
            seg.d1 = row.al; seg.d2 = row.D; seg.d3 = row.de; seg.rd = row.rho0;
          } else {
            // forward elimination of m_{c-1} (pivot: the running down row), the up row follows (fs_device.hpp)
            const R r = frcp(seg.d2);
            const R R1 = seg.d1 * r, R2 = seg.d3 * r, R3 = seg.rd * r;
            LocalElim<R> &e = el[c - 1];
            e.R1.put(R1); e.R2.put(R2); e.R3.put(R3);
            if (!Geo::kConstT) e.qc.put(rcPrev);
            const R rho = fma_(-row.al, rcPrev, row.rho0);
            seg.d1 = row.al * R1; seg.d2 = fma_(row.al, R2, row.D); seg.d3 = row.de; seg.rd = fma_(row.al, R3, rho);
            seg.u1 = fma_(-seg.u3, R1, seg.u1); seg.ru = fma_(-seg.u3, R3, seg.ru); seg.u3 = -(seg.u3 * R2);
          }
          rcPrev = row.rc;
          // the running rows must exist here: keeps row c's elimination inside cell c's scheduling region
          // (long chunks only: with M <= 4 the cells' node terms interleave profitably, measured on C4; fp32 only: C5 fp32 +5 % with
          // the pin - round 1's block fold gained 3 % at M >= 8 in fp64 too, the scalar fold has 8 running numbers instead of
          // 10 + a factor and schedules better without: +1.2 %)
          if constexpr (M >= 8 && sizeof(R) == 4)
            asm volatile("" :: "v"(seg.u1), "v"(seg.u3), "v"(seg.ru), "v"(seg.d1), "v"(seg.d2), "v"(seg.d3), "v"(seg.rd), "v"(rcPrev));
          L = Rn; i2tL = i2tR;
          if constexpr (!kTeam) { if (c == 0) FS_T(11); }     // (stamp builds: boundary rows' end to the end of the fold's first row; the rest of the fold stays in slot 0)
          __builtin_amdgcn_sched_barrier(0);        // one scheduling region per cell
        }
        seg.rc = rcPrev; rcLast = rcPrev;
      }
      const R upU1 = seg.u1, upU3 = seg.u3, upRu = seg.ru;    // the lane's finished up row, kept for the way back
      int gi = 0;                                  // conditioning monitor: largest |u3| of the segments this lane has seen
      if constexpr (kMonitor) gi = hi_abs(seg.u3);

      FS_T(0);
      // ================= 3. in-wave tree (up-sweep) =================
      Elim<R> rec[1];      // (never used: the polyline kernels' machine code depends on this declaration, on rcE, pre4 and pre3 below - tools/isa_digest.py)
      auto up_level = [&](auto lc) __attribute__((always_inline)) {
        constexpr int l = decltype(lc)::value;
        fs::up_level<l>(seg, sm.tree[wave], lane, ln);
        if constexpr (kMonitor) gi = monitor_level<l>(gi, seg);
      };
      up_level(std::integral_constant<int, 0>{}); up_level(std::integral_constant<int, 1>{});
      up_level(std::integral_constant<int, 2>{}); up_level(std::integral_constant<int, 3>{});
      up_level(std::integral_constant<int, 4>{}); up_level(std::integral_constant<int, 5>{});
      nrm2 = wave_sum(nrm2);
      if constexpr (kTeam) {
        const int wflag = __builtin_amdgcn_ballot_w64(myflag != 0) != 0 ? (int)FS_STORAGE_RANGE : 0;      // raised by a lane of this wave
        if (lane == 63) {                    // the wave's slot of the team's mailbox (device memory)
          const unsigned o = (unsigned)(member * W + wave) * kTeamWords * 16u;
          const unsigned long long tg = ((unsigned long long)a.team_epoch << 32) | (unsigned)(exchanges + 1);
          const __amdgpu_buffer_rsrc_t mb = mbox(parity);
          auto put = [&](int i, R v) __attribute__((always_inline)) { team_put2(mb, o + 16u * i, __double_as_longlong((double)v), tg); };
          put(0, seg.u1); put(1, seg.u3); put(2, seg.ru); put(3, seg.d1); put(4, seg.d2); put(5, seg.d3); put(6, seg.rd); put(7, seg.rc); put(8, nrm2);
          team_put2(mb, o + 16u * 9, ((unsigned long long)(unsigned)wflag << 32) | (unsigned)gi, tg);
        }
      } else if constexpr (kW1Lanes) {
        // nothing to post: the root segment is read from lane 63 below
      } else
      if (lane == 63) {
        put_seg(sm.xseg[parity][wave], seg);
        sm.xnorm[parity][wave] = nrm2;
        if constexpr (kMonitor) sm.xg[parity][wave] = gi;
      }
      FS_T(2);
      // the wave's own top tree record (level 5) for the way down (step 5), requested ahead of the barrier: its LDS latency passes
      // during the cross-wave step instead of after it (multi-wave kernels without diagnostics; the wave wrote it itself, in order)
      auto load_rec = [&](auto lc) __attribute__((always_inline)) {
        Elim<R> e;
        get_elim(&sm.tree[wave][0][tree_slot<decltype(lc)::value>(ln)], e);
        return e;
      };
      constexpr bool kPre = W > 1 && M >= 8 && !DIAG;
      Elim<R> pre5, pre4, pre3;      // (pre4 and pre3 are never used: see rec above)
      if constexpr (kPre) pre5 = load_rec(std::integral_constant<int, 5>{});
      // (the team form could do without this barrier - wave 0 polls the mailbox for every wave's post, its own workgroup's included - and is
      // 6 % SLOWER without it: a wave 0 that starts polling while its neighbours still fold takes their issue slots and their memory path)
      // (one-wave reaches: no s_barrier is emitted for 64 threads, and dropping the workgroup fence with it changes nothing - measured, C4 / C5 / polylines +-0.3 %)
      __syncthreads();
      FS_T(3);
      R rcE[1];            // (never used: see rec above)
      // ================= 4. across waves: fold, close with the upstream row, unfold =================
      // Waves per reach from which the step runs as a second, small DPP tree (lane w of every wave carries the segment of wave w: 8 live
      // numbers) instead of every thread folding all W segments in its own registers (16 W live doubles).  Measured on 65 536 x 4 096
      // (profiles/round3/second_wave_per_simd.md): W = 8 (the (8, 8) shape, two waves per SIMD) 7.9e6 -> 9.8e6 (the per-thread fold spills
      // at 256 registers); W = 4 (the flagship (16, 4) shape) 1.072e7 -> 1.058e7: with four segments the per-thread fold has the shorter
      // dependent chain
      constexpr int kXLanesMinW = 8;
      R tot = R(0);
      R pL, mR;                        // p of this wave's first row, m of its last one
      R mAw = R(0), mBw = R(0);        // m of this wave's first row / of the next wave's first row (shared nodes, below)
      if constexpr (kTeam) {
        // ---- the team's exchange: where one workgroup has a barrier, G workgroups have the tags of their mailbox in device memory ----
        ++exchanges;
        FS_T(11);
        if (wave == 0) {
          // the top tree over the S = G W posted segments, one per lane, identity segments beyond (the multi-pass kernel's, fs_long.hpp)
          const int S = G * W;
          Seg<R> xs;
          R nr, aU, bU, rU;
          int gx, fl;
          {
            // lane s polls the ten words of slot s, every lane the three of the upstream row, until all carry this exchange's tag
            const unsigned long long want = ((unsigned long long)a.team_epoch << 32) | (unsigned)exchanges;
            const __amdgpu_buffer_rsrc_t mb = mbox(parity);
            const unsigned o = (unsigned)(lane < S ? lane : 0) * kTeamWords * 16u, ou = (unsigned)S * kTeamWords * 16u;
            const unsigned long long t_in = __builtin_amdgcn_s_memtime();
            fs_u4 w[13];
            int stall = 0;
            for (;;) {
#pragma unroll
              for (int i = 0; i < 10; ++i) w[i] = team_get2(mb, o + 16u * i);
#pragma unroll
              for (int i = 0; i < 3; ++i) w[10 + i] = team_get2(mb, ou + 16u * i);
              bool ok = true;
#pragma unroll
              for (int i = 0; i < 13; ++i) ok = ok && team_tag(w[i]) == want;
              if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
              __builtin_amdgcn_s_sleep(kTeamSleep);
              if (__builtin_amdgcn_s_memtime() - t_in > kTeamPatience) { stall = 1; break; }     // give the reach up, do not spin on
            }
            if (lane == 0) sm.xstall = stall;
            auto val = [&](int i) { return (R)__longlong_as_double((long long)team_bits(w[i])); };
            const R posted[8] = {val(0), val(1), val(2), val(3), val(4), val(5), val(6), val(7)};
            get_seg(posted, xs);
            nr = val(8);
            gx = (int)(unsigned)team_bits(w[9]); fl = (int)(unsigned)(team_bits(w[9]) >> 32);
            aU = val(10); bU = val(11); rU = val(12);
          }
          if (lane >= S) { identity_seg(xs); nr = R(0); gx = 0; fl = 0; }
          const R u1o = xs.u1, u3o = xs.u3, ruo = xs.ru;
          auto xup = [&](auto lc) __attribute__((always_inline)) {
            constexpr int l = decltype(lc)::value;
            fs::up_level<l>(xs, sm.xtree, lane, lane);
            gx = monitor_level<l>(gx, xs);
            fl = max_(tree_from_below<(1 << l)>(fl), fl);
          };
          // (levels that would only merge identity segments are skipped: S <= 2^nl lanes carry something; the root then sits in lane 2^nl - 1)
          const int nl = S <= 8 ? 3 : (S <= 16 ? 4 : (S <= 32 ? 5 : 6));
          xup(std::integral_constant<int, 0>{}); xup(std::integral_constant<int, 1>{}); xup(std::integral_constant<int, 2>{});
          if (nl > 3) xup(std::integral_constant<int, 3>{});
          if (nl > 4) xup(std::integral_constant<int, 4>{});
          if (nl > 5) xup(std::integral_constant<int, 5>{});
          WaveSync{}();
          R p0, m0, ml;
          close_root(xs, aU, bU, rU, p0, m0, ml);            // valid in the root's lane
          const int rl = (1 << nl) - 1;
          R px = read_lane(p0, rl), mx = read_lane(ml, rl);
          auto xdown = [&](auto lc) __attribute__((always_inline)) {
            constexpr int l = decltype(lc)::value;
            Elim<R> e;
            get_elim(&sm.xtree[0][tree_slot<l>(lane)], e);
            const R sep = separator(e, px, mx);
            const bool upper = ((lane >> l) & 1) != 0;
            px = upper ? e.rc - sep : px;
            mx = upper ? mx : sep;
          };
          if (nl > 5) xdown(std::integral_constant<int, 5>{});
          if (nl > 4) xdown(std::integral_constant<int, 4>{});
          if (nl > 3) xdown(std::integral_constant<int, 3>{});
          xdown(std::integral_constant<int, 2>{}); xdown(std::integral_constant<int, 1>{}); xdown(std::integral_constant<int, 0>{});
          post_top_tree(sm.xres, lane, S, u1o, u3o, ruo, px, mx);
          const R tsum = wave_sum(nr);               // (a fixed order: the same total in every member)
          // (cross-lane reads in uniform control flow, fs_long.hpp)
          const int gtop = __builtin_amdgcn_readlane(gx, rl), ftop = __builtin_amdgcn_readlane(fl, rl);
          if (lane == 0) { sm.xtot = tsum; sm.xwarn = gtop > growth_limit_bits<R>() ? 1 : 0; sm.xflagT = ftop; }
        }
        __syncthreads();
        tot = sm.xtot;
        {
          const R *xr = sm.xres[member * W + wave];
          pL = xr[0]; mR = xr[1]; mAw = xr[2]; mBw = xr[3];
        }
        if constexpr (kMonitor) { if (sm.xwarn != 0) grow = true; }
        if (sm.xflagT != 0) status = sm.xflagT;
        if (sm.xstall != 0) status = FS_TEAM_STALL;
      } else if constexpr (kW1Lanes) {
        // One wave: the root segment sits in lane 63, the upstream row in lane 0.  Lane 63 closes the system on its own registers (every
        // lane executes it, lane 63's result is the one read) - the arithmetic of the general path below, without its LDS round trip.
        tot = nrm2;                                    // (wave_sum left the total in every lane)
        const R aU = read_lane(xb0, 0), bU = read_lane(xb1, 0), rU = read_lane(xb2, 0);
        R p0, m0, ml;
        close_root(seg, aU, bU, rU, p0, m0, ml);
        pL = read_lane(p0, 63); mR = read_lane(ml, 63);
        if constexpr (kMonitor) { if (__builtin_amdgcn_readlane(gi, 63) > growth_limit_bits<R>()) grow = true; }
      } else if constexpr (W > 1 && W >= kXLanesMinW) {
        // A second, small tree over the W wave segments, one segment per LANE: lane w of every wave takes the segment of
        // wave w and the W - 1 merges run as log2 W DPP levels (row_shr:1/2/4) exactly like the in-wave tree - the same
        // merges in the same order as the per-thread fold below, so the bits do not change - with 8 live numbers per lane
        // instead of 16 W.  Every wave does it redundantly on its own copy of the records (no second barrier).
        constexpr int LW = W == 2 ? 1 : (W == 4 ? 2 : 3);
        static_assert(W == 2 || W == 4 || W == 8, "cross-wave tree: 2, 4 or 8 waves per reach");
        const int wl = ln & (W - 1);
        const R *ps = sm.xseg[parity][wl];
        Seg<R> xs;
        get_seg(ps, xs);
        const R u1o = xs.u1, u3o = xs.u3, ruo = xs.ru;       // the wave's own up row (m of its first row, below)
#pragma unroll
        for (int w = 0; w < W; ++w) tot += sm.xnorm[parity][w];
        int gx = 0;
        if constexpr (kMonitor) gx = sm.xg[parity][wl];
        // Records stay in registers (valid in the lane that survives its level: low l + 1 bits set); on the way down the
        // group's record comes from the group's last lane by a quad permute (groups of 2 and 4 lanes) or a readlane (8).
        Elim<R> xe[LW];
        auto xup = [&](auto lc) __attribute__((always_inline)) {
          constexpr int l = decltype(lc)::value;
          constexpr int d = 1 << l;
          if constexpr (l < LW) {
            const Seg<R> left = seg_from_below<d>(xs);
            Seg<R> mg;
            merge(left, xs, mg, xe[l]);
            xs = mg;
            if constexpr (kMonitor) gx = max_(max_(tree_from_below<d>(gx), gx), hi_abs(mg.u3));
          }
        };
        xup(std::integral_constant<int, 0>{}); xup(std::integral_constant<int, 1>{}); xup(std::integral_constant<int, 2>{});
        R p0, m0, ml;
        close_root(xs, sm.xbc[parity][0], sm.xbc[parity][1], sm.xbc[parity][2], p0, m0, ml);     // valid in lane W - 1
        R px = read_lane(p0, W - 1), mx = read_lane(ml, W - 1);
        auto xdown = [&](auto lc) __attribute__((always_inline)) {
          constexpr int l = decltype(lc)::value;
          if constexpr (l < LW) {
            Elim<R> e;
            if constexpr (l == 0) {        // quad_perm:[1,1,3,3]
              e.A1 = dpp_mov<0xF5>(xe[l].A1); e.A2 = dpp_mov<0xF5>(xe[l].A2); e.A3 = dpp_mov<0xF5>(xe[l].A3); e.rc = dpp_mov<0xF5>(xe[l].rc);
            } else if constexpr (l == 1) { // quad_perm:[3,3,3,3]
              e.A1 = dpp_mov<0xFF>(xe[l].A1); e.A2 = dpp_mov<0xFF>(xe[l].A2); e.A3 = dpp_mov<0xFF>(xe[l].A3); e.rc = dpp_mov<0xFF>(xe[l].rc);
            } else {
              e.A1 = read_lane(xe[l].A1, 7); e.A2 = read_lane(xe[l].A2, 7); e.A3 = read_lane(xe[l].A3, 7); e.rc = read_lane(xe[l].rc, 7);
            }
            const R sep = separator(e, px, mx);
            const bool upper = ((wl >> l) & 1) != 0;
            px = upper ? e.rc - sep : px;
            mx = upper ? mx : sep;
          }
        };
        xdown(std::integral_constant<int, 2>{}); xdown(std::integral_constant<int, 1>{}); xdown(std::integral_constant<int, 0>{});
        // m of every wave's first row from its own up row: the node there is shared with the wave before, and both
        // copies must move by the same bits
        const R max_ = fma_(-u1o, px, fma_(-u3o, mx, ruo));
        const int ws = __builtin_amdgcn_readfirstlane(wave);
        pL = read_lane(px, ws); mR = read_lane(mx, ws); mAw = read_lane(max_, ws);
        mBw = read_lane(max_, (ws + 1) & (W - 1));
        if (ws == W - 1) mBw = R(0);
        if constexpr (kMonitor) { if (__builtin_amdgcn_readlane(gx, W - 1) > growth_limit_bits<R>()) grow = true; }
      } else {
      {
        // pairwise tree over the W wave segments (depth log2 W instead of a serial chain of W-1 merges;
        // the two merges of a level are independent and overlap); every thread does all of it
        Seg<R> sw[W], sw0[W];
        Elim<R> we[W > 1 ? W - 1 : 1];
#pragma unroll
        for (int w = 0; w < W; ++w) {
          const R *p = sm.xseg[parity][w];
          get_seg(p, sw[w]);
          sw0[w] = sw[w];
          tot += sm.xnorm[parity][w];
        }
        int gx = 0;
        if constexpr (kMonitor) {
#pragma unroll
          for (int w = 0; w < W; ++w) gx = max_(gx, sm.xg[parity][w]);
        }
#pragma unroll
        for (int st = 1; st < W; st *= 2)
#pragma unroll
          for (int i = 0; i + st < W; i += 2 * st) {
            merge(sw[i], sw[i + st], sw[i], we[i + st - 1]);
            if constexpr (kMonitor) gx = max_(gx, hi_abs(sw[i].u3));
          }
        if constexpr (kMonitor) { if (gx > growth_limit_bits<R>()) grow = true; }
        R pw[W], mw[W], p0, m0, ml;      // pw[w], mw[w]: the two numbers of wave w (valid for the group heads while unfolding)
        close_root(sw[0], sm.xbc[parity][0], sm.xbc[parity][1], sm.xbc[parity][2], p0, m0, ml);
        pw[0] = p0; mw[0] = ml;
#pragma unroll
        for (int st = W / 2; st >= 1; st /= 2)
#pragma unroll
          for (int i = 0; i + st < W; i += 2 * st) {
            const Elim<R> &e = we[i + st - 1];
            const R sep = separator(e, pw[i], mw[i]);
            pw[i + st] = e.rc - sep; mw[i + st] = mw[i]; mw[i] = sep;
          }
        // m of every wave's first row from its own up row: the node there is shared with the wave before, and both
        // copies must move by the same bits
        R ma[W + 1];
#pragma unroll
        for (int w = 0; w < W; ++w) ma[w] = fma_(-sw0[w].u1, pw[w], fma_(-sw0[w].u3, mw[w], sw0[w].ru));
        ma[W] = R(0);
        pL = pw[0]; mR = mw[0]; mAw = ma[0]; mBw = ma[1];
#pragma unroll
        for (int w = 1; w < W; ++w)
          if (wave == w) { pL = pw[w]; mR = mw[w]; mAw = ma[w]; mBw = ma[w + 1]; }
      }
      }
      FS_T(4);
      if (!kTeam && (BCK < 2 || ds_storage) && sm.xflag[parity] != 0) status = sm.xflag[parity];     // only the storage rows raise a flag (a team's: through the mailbox, above)
      // ||R|| = sqrt(tot) (utility.py:20-22) is NaN or beyond the blow-up bound (preissmann.py:135-137) exactly when tot is
      // not finite (the bound exceeds the root of the largest finite number in either precision)
      if (!(tot <= finite_max<R>())) status = FS_NAN;
      bool below;                                                      // ||R|| < tolerance (preissmann.py:153)
      if (DIAG || M < 8) {               // (the two-rows-per-lane kernels sit on their register cap: the branch below costs C4 19 %)
        const R err = sqrt_(tot);
        if constexpr (BCK <= 0) below = err < tol_of(); else
        below = err < a.tol;
        if (DIAG && a.trace && gt == 0 && it <= FS_TRACE_CAP) a.trace[((size_t)level * FS_TRACE_CAP + (it - 1)) * a.B + reach] = err;
      } else {
        // without a trace to write the root is only needed when tot lies within rounding of tol^2 (the decision must be
        // the one sqrt() gives, bit for bit: Newton counts are compared with the reference's)
        if constexpr (BCK <= 0) {
          const R tl = tol_of();
          const R t2 = tl * tl, band = R(16) * eps_of<R>() * t2;
          below = tot < t2 - band ? true : (tot > t2 + band ? false : sqrt_(tot) < tl);
        } else {      // (spelled as it always was: the benchmark kernels keep their machine code, tools/isa_digest.py)
        const R t2 = a.tol * a.tol, band = R(16) * eps_of<R>() * t2;
        below = tot < t2 - band ? true : (tot > t2 + band ? false : sqrt_(tot) < a.tol);
        }
      }
      converged = status == FS_OK && below;
      // The warning is about the system the level's result comes from - the Jacobian at the accepted iterate.  An iterate on the
      // way there may pass a small pivot by accident (a soak draw did: a three-node reach behind a reservoir, condition number
      // 3e4 throughout, |u3| > 2^10 once in the 12 iterations of its first level); Newton does not remember that.
      if (converged && grow) warn = true;

      FS_T(5);
      // ================= 5. separators down the tree, local back-substitution ============
      // Every lane carries two numbers of the group of 2^(l+1) lanes it belongs to at the current level: the p of the
      // group's first row and the m of its last one.  The group's record is one LDS slot that all its lanes read (a
      // broadcast read); each lane recovers the separator itself and keeps it as its new right number (lower half) or
      // turns it into its new left one (upper half): no cross-lane traffic, two dependent fp64 operations per level.
      auto down_level = [&](auto lc, const Elim<R> &e) __attribute__((always_inline)) {
        constexpr int l = decltype(lc)::value;
        const R sep = separator(e, pL, mR);
        const bool upper = ((lane >> l) & 1) != 0;
        pL = upper ? e.rc - sep : pL;
        mR = upper ? mR : sep;
      };
      {
        // records are requested one level ahead (the memory clobbers keep the compiler from requesting all six up front)
        using I5 = std::integral_constant<int, 5>; using I4 = std::integral_constant<int, 4>;
        using I3 = std::integral_constant<int, 3>; using I2 = std::integral_constant<int, 2>;
        using I1 = std::integral_constant<int, 1>; using I0 = std::integral_constant<int, 0>;
        __builtin_amdgcn_sched_barrier(0);
        Elim<R> r5, r4, r3;      // (declared ahead of their loads, not where they are loaded: the table and polyline kernels' machine code depends on it)
        if constexpr (kPre) r5 = pre5; else r5 = load_rec(I5{});
        r4 = load_rec(I4{});
        asm volatile("" ::: "memory");
        down_level(I5{}, r5);
        r3 = load_rec(I3{});
        asm volatile("" ::: "memory");
        down_level(I4{}, r4);
        const Elim<R> r2 = load_rec(I2{});
        asm volatile("" ::: "memory");
        down_level(I3{}, r3);
        const Elim<R> r1 = load_rec(I1{});
        asm volatile("" ::: "memory");
        down_level(I2{}, r2);
        const Elim<R> r0 = load_rec(I0{});
        asm volatile("" ::: "memory");
        down_level(I1{}, r1);
        down_level(I0{}, r0);
        asm volatile("" : "+v"(pL), "+v"(mR));
        __builtin_amdgcn_sched_barrier(0);
      }
      // m of the lane's first row from its up row; a wave's first lane takes the number the cross-wave step computed, so
      // that the last lane of the wave before (which gets the same number) moves its copy of the shared node identically
      R mA = fma_(-upU1, pL, fma_(-upU3, mR, upRu));
      if (W > 1 && lane == 0) mA = mAw;
      R mB = dpp_mov<0x134>(mA);                // wave_rol:1 - m of the next lane's first row = this lane's node M
      if (lane == 63) mB = mBw;

      // The update is kept pending in dh/dQ as p + m and p - m (they take the registers the elimination records free up):
      // the accepted iterate must still be intact for the level-constant pass below.
      if (Geo::kConstT) {
        // The continuity residuals are recomputed below on purpose (one value per node less to keep
        // across the solve).  Hide the operands so that common-subexpression elimination does not
        // resurrect the fold's copies of dQ / kc0 and keep 2 values per node alive instead.
        asm volatile("" : "+v"(kco));
        kcb = &sm.kc[0][0][0] + kco;
#pragma unroll
        for (int j = 0; j <= M; ++j) asm volatile("" : "+v"(h[j]), "+v"(Q[j]));
      }
      const R i2tc = dt * geo.rT_const();
      auto i2t_of = [&](int j) { return Geo::kConstT ? i2tc : iTn[j]; };
      {
        // rc of row j for the link p_{j+1} = rc_j - m_j: minus the continuity residual of cell j, 0 beyond the cells
        auto rc_of = [&](int j) __attribute__((always_inline)) {
          if (Geo::kConstT) {
            const R v = -(fma_(h[j] + h[j + 1], Tr2dt, cq * (Q[j + 1] - Q[j])) + kcb[(0 * M + j) * T]);
            return (RAGGED && s0 + j >= NC) ? R(0) : v;
          }
          return j + 1 < M ? el[j].qc.get() : rcLast;
        };
        R mj = mR;                                  // m of row M-1
        {
          // node M: p from this lane's last row, m from the next lane.  rcLast, not a recomputed residual: the next lane's
          // p of its first row is (this rc) - (this m), and both copies of the shared node must move by the same bits
          const R pM = rcLast - mR;
          dh[M] = pM + mB; dQ[M] = pM - mB;
        }
#pragma unroll
        for (int j = M - 1; j >= 1; --j) {
          // m_{j-1} = R3 - R1 p_a - R2 m_j ; row 0's m comes from the up row (mA)
          const R mprev = j == 1 ? mA : fma_(-el[j - 1].R2.get(), mj, fma_(-el[j - 1].R1.get(), pL, el[j - 1].R3.get()));
          const R pj = rc_of(j - 1) - mprev;
          dh[j] = pj + mj; dQ[j] = pj - mj;
          mj = mprev;
        }
        dh[0] = pL + mA; dQ[0] = pL - mA;
      }
      FS_T(6);
      // fp32 only: pin the back-substituted (pending) sums and fence them off from the acceptance block (three waves per SIMD at 168 registers:
      // the fence keeps them there, C5 fp32 +4.5 %; fp64: round 1 +0.9 %, with the round-2 solve flagship -2.3 %)
      if constexpr (sizeof(R) == 4) {
#pragma unroll
        for (int j = 1; j < M; ++j) asm volatile("" : "+v"(dh[j]), "+v"(dQ[j]));
        __builtin_amdgcn_sched_barrier(0);
      }

      // ================= 6. accepted iterate -> level k =================
      if (converged) {
        if (gt == 0) {
          a.hydro[((size_t)level * 4 + 0) * a.B + reach] = h[0];
          a.hydro[((size_t)level * 4 + 1) * a.B + reach] = Q[0];
          a.iters[(size_t)level * a.B + reach] = it;
        }
        // Level k+1 is rebuilt from registers, so the accepted state only has to reach HBM when
        // somebody can look at it: at the last level of this launch (fs_batch_get_state, next launch)
        // and, if a history is kept, at every level.  (A transposed, fully coalesced write-back
        // through LDS was measured too: no gain, three extra barriers.)
        const bool last = (step == a.n_steps - 1);
        R *const hh_p = (DIAG && a.hist_h) ? a.hist_h + ((size_t)level * a.B + reach) * NS + s0 : nullptr;
        R *const hQ_p = (DIAG && a.hist_h) ? a.hist_Q + ((size_t)level * a.B + reach) * NS + s0 : nullptr;
        if (last || hh_p) {
#pragma unroll
          for (int j = 0; j < M; ++j) {
            if (!RAGGED || s0 + j < N) {
              if (last) { hk_p[j] = h[j]; Qk_p[j] = Q[j]; }
              if (hh_p) { hh_p[j] = h[j]; hQ_p[j] = Q[j]; }
            }
          }
        }
        FS_T(8);
        if (gt == tD) {
#pragma unroll
          for (int j = RAGGED ? 0 : M - 1; j < M; ++j)
            if (j == jD) {
              a.hydro[((size_t)level * 4 + 2) * a.B + reach] = h[j];
              a.hydro[((size_t)level * 4 + 3) * a.B + reach] = Q[j];
              QoldD = Q[j];                                             // flow[k] of the next level's storage row
            }
          Yprev = Ynew;
          if (ds_storage) a.stage_hist[(size_t)level * a.B + reach] = Ynew;
        }
        FS_T(9);
        if (kSaveTerms) {                                             // level constants of the next level
          level_constants_from_saved(h, Q);
        } else {
          write_level_constants(h, Q);
        }
        FS_T(10);
      }

      FS_T(5);
#pragma unroll
      for (int j = 0; j <= M; ++j) {                                       // preissmann.py:146-147
        // tail-only form: the masks ride in the factor - phantom nodes (j > TAIL from the owner lane on, every j behind it) stay where they are
        const R mk = kTail ? (j <= TAIL ? mle : mlt) : R(1);
        h[j] = fma_(dh[j], kTail ? i2t_of(j) * mk : i2t_of(j), h[j]);
        Q[j] = fma_(dQ[j], kTail ? i2c * mk : i2c, Q[j]);
      }
    }
    if (status != FS_OK && gt == 0) a.iters[(size_t)level * a.B + reach] = it - (status == FS_MAX_ITER ? 1 : 0);
    if (kBudget && a.iter_budget > 0) {
      if (t == 0) a.it_done[reach] = (converged || status != FS_OK) ? -1 : it;
      if (!converged) break;                  // budget spent: the Newton vector goes back to hg / Qg below
    }
  }

  // ---- Newton start vector of the next level + per-reach bookkeeping ----
#pragma unroll
  for (int j = 0; j < M; ++j)
    if (!RAGGED || s0 + j < N) { hg_p[j] = h[j]; Qg_p[j] = Q[j]; }
  if (gt == 0) a.status[reach] = (status == FS_OK && warn) ? (int)FS_ILL_CONDITIONED : status;
  if (ds_storage && gt == tD) a.Yprev[reach] = Yprev;
#ifdef FS_STAMP
  if (a.dbg && lane == 0)
    for (int i = 0; i < 12; ++i) a.dbg[((size_t)reach * 16 + (member * W + wave) % 16) * 12 + i] = stamp_[i];
#endif
}

}  // namespace fs

#include "fs_long.hpp"
