// fs_dispatch.hpp - which kernel instantiation a batch gets: the key that describes an instantiation, the query a batch asks with,
// the environment's overrides, and fits() / pick() over a table of keys; and what a launch of the chosen one needs beside the batch's
// own arrays (plan_launch).  Plain C++17 apart from the __host__ __device__ marks of bc_is_light and team_mailbox_bytes under hipcc
// (the kernels use them too): tests/dispatch/ builds the key table from the very lists of the library (fs_entry_list.hpp) with the
// system compiler, checks every choice against tests/golden/dispatch/choices.npz and every plan against the kernels' layouts.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <tuple>

#include "../../include/flowsim_abi.h"
#include "fs_entry_list.hpp"      // FS_KIND_*: what FS_KEY reads a row's kind with
#include "fs_host_pack.hpp"       // sec_is_uniform

#ifndef FS_ST_HD
#ifdef __HIPCC__
#define FS_ST_HD __host__ __device__
#else
#define FS_ST_HD
#endif
#endif

namespace fs {

// the boundary kinds whose rows need no pow() and no storage curve (boundary class 1; fs_device.hpp: bc_eval_rect)
FS_ST_HD constexpr bool bc_is_light(int kind) { return kind != FS_BC_RATING_POWER && kind < FS_BC_STORAGE_CURVE; }

// What one kernel instantiation was compiled for.  (The one description of these fields; a list row of fs_entry_list.hpp carries them
// in this order behind its kind and type.)
struct KernelKey {
  int dtype;   // FS_F64 | FS_F32
  int sec;     // FS_SEC_*
  int M;       // rows of the scalar system per lane (>= 2): N - 1 cells + the downstream boundary row
  int W;       // waves per reach; one workgroup keeps a lane grid of 64 W M rows on chip
  int full;    // 1: no per-row selects - the boundary row takes the last row of the lane grid: only N == 64 W M (a team's: N a whole
               //    number of lane grids); 0: ragged, any N up to the capacity
  int bck;     // boundary class (fs_kernel.hpp): -1 any kind, 0 any but FS_BC_STORAGE_CURVE / FS_BC_HOST_ROW, 1 FS_SEC_RECT_UNIFORM
               //    with bc_is_light() kinds on both ends (closed-form rows), 2 + k (FS_BCK(k)) flow hydrograph upstream and kind k downstream
  int diag;    // 0: compiled without the history / residual-trace stores
  int longk;   // 1: the multi-pass kernel (fs_long.hpp) for reaches longer than one lane grid: up to 64 / W passes of 64 W M rows
  int tail;    // >= 0: tail-only form (fs_kernel.hpp, TAIL), compiled for the local row of the boundary row: only (N - 1) mod M == tail; -1: not
  int team;    // 1: a reach as a team of up to 64 / W workgroups of 64 W M rows each (fs_kernel.hpp, TEAM)
};
#define FS_KEY(KIND, R, DT, SEC, M, W, FULL, BCK, DIAG, TAIL) \
  fs::KernelKey{DT, SEC, M, W, FULL, (int)(BCK), DIAG, FS_KIND_##KIND == FS_KIND_LONG, TAIL, FS_KIND_##KIND == FS_KIND_TEAM}

// What a batch asks for.
struct Query {
  int dtype, sec;
  int N;                   // nodes per reach (the largest, where the reaches differ)
  int usk, dsk;            // boundary kinds (FS_BC_*) upstream and downstream
  bool need_diag = false;  // the batch keeps history, a residual trace or monitors
  bool need_any = false;   // boundary class -1 only: an iteration budget (fs_batch_iterate), host rows
  int hetero = 0;          // bit 0: per-reach node counts; bit 1: per-reach scheme or boundary kinds (classes 0 and -1 read them)
};

// What the environment narrows the choice to (experiments and tests).
struct Overrides {
  bool force_index = false;     // FS_KERNEL_INDEX=i: entry i or nothing
  int index = 0;
  std::string index_text;       //   as given: the refusal repeats it
  int M = 0, W = 0;             // FS_KERNEL_SHAPE="M,W": entries of this shape only (M == 0: any)
  bool general_only = false;    // FS_KERNEL_GENERAL=1: entries with diagnostics and a boundary class below 2 only
  bool no_team = false;         // FS_NO_TEAM (set to anything): no team entries - long reaches take the multi-pass kernel
  int team_M = -1;              // FS_TEAM_M=m: team entries with m rows per lane only (< 0: any)
};

inline Overrides overrides_from_environment() {
  Overrides o;
  if (const char *env = std::getenv("FS_KERNEL_INDEX")) { o.force_index = true; o.index = std::atoi(env); o.index_text = env; }
  if (const char *env = std::getenv("FS_KERNEL_SHAPE")) std::sscanf(env, "%d,%d", &o.M, &o.W);
  if (const char *env = std::getenv("FS_KERNEL_GENERAL")) o.general_only = env[0] == '1';
  o.no_team = std::getenv("FS_NO_TEAM") != nullptr;
  if (const char *env = std::getenv("FS_TEAM_M")) o.team_M = std::max(std::atoi(env), 0);      // (nonsense: 0, which no entry has)
  return o;
}

// can this instantiation advance that batch?  (The index and shape overrides choose among the entries that fit: pick().)
inline bool fits(const KernelKey &k, const Query &q, const Overrides &o) {
  if (k.dtype != q.dtype || k.sec != q.sec) return false;
  // size: one lane grid, or 64 / W of them (passes of the multi-pass kernel, members of a team)
  const long grid = 64L * k.W * k.M, cap = grid * ((k.longk || k.team) ? 64 / k.W : 1);
  if (q.N > cap || q.N > 32768) return false;
  if (k.full && (k.team ? q.N % grid != 0 : q.N != cap)) return false;
  if (k.tail >= 0 && (q.N - 1) % k.M != k.tail) return false;
  // a team only where one workgroup does not hold the reach, and never below 4 097 nodes
  if (k.team && (q.N <= 4096 || q.N <= grid || o.no_team || (o.team_M >= 0 && o.team_M != k.M))) return false;
  // per-reach node counts: the boundary row's place differs from reach to reach; per-reach kinds: read at run time
  if ((q.hetero & 1) && (k.full || k.tail >= 0)) return false;
  if ((q.hetero & 2) && k.bck > 0) return false;
  if (q.need_diag && !k.diag) return false;
  // boundary class
  if (q.need_any && k.bck != -1) return false;
  if (k.bck == 0 && (q.usk >= FS_BC_STORAGE_CURVE || q.dsk >= FS_BC_STORAGE_CURVE)) return false;
  if (k.bck == 1 && !(q.sec == FS_SEC_RECT_UNIFORM && bc_is_light(q.usk) && bc_is_light(q.dsk))) return false;
  if (k.bck >= 2 && (q.usk != FS_BC_FLOW_HYDROGRAPH || q.dsk != k.bck - 2)) return false;
  return true;
}

// The order of preference among the entries that fit, smaller first, compared field by field:
//   1. tier: a kernel that keeps the reach on chip whenever one fits - one workgroup (0), else a team of them (1), else the
//      multi-pass kernel (2);
//   2. capacity M W: the smallest lane grid that holds the reach (fewest idle rows);
//   3. waves per reach W: at equal capacity the shape with more rows per lane and fewer waves to synchronise - a 2 000-node reach takes
//      (16, 2), not (8, 4): both hold 2 048 rows;
//   4. specificity: at equal shape the instantiation compiled for more of what the batch is - tail-only form (16) > no diagnostics (8)
//      > boundary pair fixed (4) > closed-form rows (2) > any kind but the storage curve (1) > any kind (0), and full before ragged (1).
// Entries that compare equal: the first in table order.
inline std::tuple<int, int, int, int> preference(const KernelKey &k) {
  const int tier = k.longk ? 2 : (k.team ? 1 : 0);
  const int specificity = k.full + (k.bck >= 2 ? 4 : k.bck == 1 ? 2 : k.bck == 0 ? 1 : 0) + (k.diag ? 0 : 8) + (k.tail >= 0 ? 16 : 0);
  return {tier, k.M * k.W, k.W, -specificity};
}

// index of the entry of table[n] the batch gets, or -1 and the reason in *why (Row: anything with a KernelKey member "key")
template <typename Row>
int pick(const Row *table, int n, const Query &q, const Overrides &o, std::string *why) {
  if (o.force_index) {
    if (o.index >= 0 && o.index < n && fits(table[o.index].key, q, o)) return o.index;
    if (why) *why = "FS_KERNEL_INDEX=" + o.index_text + " does not fit this batch";
    return -1;
  }
  int best = -1;
  for (int i = 0; i < n; ++i) {
    const KernelKey &k = table[i].key;
    if (!fits(k, q, o)) continue;
    if (o.general_only && (!k.diag || k.bck >= 2)) continue;
    if (o.M && (k.M != o.M || k.W != o.W)) continue;
    if (best < 0 || preference(k) < preference(table[best].key)) best = i;
  }
  if (best < 0 && why) *why = "no kernel instantiation for N=" + std::to_string(q.N) + " (supported: 2..32768 nodes for the uniform section "
                              "modes, 2..16384 for tables and polylines)";
  return best;
}

// ---- what one launch of an instantiation needs beside the batch's own arrays (fs_abi.hip: launch_steps makes the HIP calls) ----
constexpr int kTeamWords = 12;   // per mailbox slot: the segment (8), the wave's residual sum (1), two ints (monitor word, boundary flag), pad
// bytes of one reach's mailbox of one iteration parity: a slot per (member, wave) and one for the upstream row, kTeamWords 16-byte (value,
// tag) words each.  The host allocates [B][2] of them; the team kernel (fs_kernel.hpp) strides them by this very number
FS_ST_HD constexpr size_t team_mailbox_bytes(int G, int W) { return (size_t)(G * W + 1) * kTeamWords * 16; }

struct LaunchPlan {
  int passes = 0;                 // multi-pass kernel: passes of 64 W M rows over a reach (0: another kernel)
  size_t kc_scratch_elems = 0;    //   its level constants [B][4][passes * 64 W M]; none for uniform sections (fs_long.hpp recomputes them)
  int team_size = 0;              // team kernel: G workgroups of 64 W M rows per reach (0: another kernel)
  size_t team_mail_bytes = 0;     //   their mailboxes [B][2][G W + 1][kTeamWords]
  // a launch of several levels: a reach that fails on a later one gets back what the launch began with (one level: nothing to keep)
  bool keep_entry = false;        //   the state: the multi-pass kernel of the uniform section modes writes every accepted level to hk / Qk
  bool keep_stage = false;        //   the reservoir stage: every step kernel writes back the last one it accepted
};
inline LaunchPlan plan_launch(const KernelKey &k, int section_mode, size_t B, size_t N, int n_steps, bool storage_downstream) {
  LaunchPlan p;
  const size_t grid = (size_t)64 * k.W * k.M;
  const int grids = (int)((N + grid - 1) / grid);
  const bool uniform = sec_is_uniform(section_mode);
  if (k.longk) { p.passes = grids; p.kc_scratch_elems = uniform ? 0 : B * 4 * grids * grid; }
  if (k.team) { p.team_size = grids; p.team_mail_bytes = B * 2 * team_mailbox_bytes(grids, k.W); }
  p.keep_entry = k.longk && uniform && n_steps > 1;
  p.keep_stage = storage_downstream && n_steps > 1;
  return p;
}

}  // namespace fs
