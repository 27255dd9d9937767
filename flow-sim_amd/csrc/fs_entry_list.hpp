// fs_entry_list.hpp - the kernel instantiation lists (X-macros): one row per instantiation, every row of the same shape,
//   X(KIND, R, DT, SEC, M, W, FULL, BCK, DIAG, TAIL)
// KIND is STEP (preissmann_step_kernel, one workgroup per reach), LONG (preissmann_long_kernel, fs_long.hpp: one workgroup, several
// passes) or TEAM (preissmann_step_kernel as a team of workgroups per reach); R / DT the arithmetic type and its FS_F64 / FS_F32;
// the other fields are those of fs::KernelKey (fs_dispatch.hpp), which says what each means.  Nothing but the preprocessor and
// include/flowsim_abi.h is needed to read the lists: fs_entries.hpp turns a row into an instantiation, an extern declaration or a row of
// the dispatch table of fs_abi.hip; FS_KEY (fs_dispatch.hpp) turns it into a fs::KernelKey, also under the system compiler (tests/dispatch/).
// A new kernel family is new rows in a list here (a new list: one more fs_part_*.hip and one more name in FS_ACTIVE_LIST).
#pragma once
#include "../../include/flowsim_abi.h"

enum { FS_KIND_STEP = 0, FS_KIND_LONG = 1, FS_KIND_TEAM = 2 };

#define FS_BCK(kind) (2 + (kind))      // boundary class: flow hydrograph upstream, this kind downstream

#define FS_LIST_RECT(X, R, DT) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 2, 1, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 4, 1, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 8, 1, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 1, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 2, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 4, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 8, 1, 0, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 2, 1, 0, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 4, 1, 0, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 4, 0, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 8, 1, 1, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 4, 1, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 8, 4, 1, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 8, 4, 0, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 8, 8, 1, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 1, 1, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 2, 1, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 1, 0, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 2, 0, 1, 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 4, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 4, 0, FS_BCK(FS_BC_NORMAL_DEPTH), 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 2, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 16, 1, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 8, 1, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 1, -1) \
  X(STEP, R, DT, FS_SEC_RECT_UNIFORM, 8, 1, 0, FS_BCK(FS_BC_NORMAL_DEPTH), 1, -1)

#define FS_LIST_TRAP(X, R, DT) \
  X(STEP, R, DT, FS_SEC_TRAP_UNIFORM, 2, 1, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_TRAP_UNIFORM, 4, 1, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_TRAP_UNIFORM, 8, 1, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_TRAP_UNIFORM, 8, 1, 1, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_TRAP_UNIFORM, 16, 4, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_TRAP_UNIFORM, 8, 1, 1, FS_BCK(FS_BC_RATING_POWER), 1, -1) \
  X(STEP, R, DT, FS_SEC_TRAP_UNIFORM, 8, 1, 0, FS_BCK(FS_BC_RATING_POWER), 1, -1)

#define FS_LIST_TABLE(X, R, DT) \
  X(STEP, R, DT, FS_SEC_TABLE, 2, 1, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_TABLE, 4, 1, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_TABLE, 8, 1, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_TABLE, 8, 2, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_TABLE, 8, 4, 0, 0, 1, -1) \
  X(STEP, R, DT, FS_SEC_TABLE, 2, 1, 0, -1, 1, -1) \
  X(STEP, R, DT, FS_SEC_TABLE, 4, 1, 0, -1, 1, -1) \
  X(STEP, R, DT, FS_SEC_TABLE, 8, 1, 0, -1, 1, -1) \
  X(STEP, R, DT, FS_SEC_TABLE, 8, 2, 0, -1, 1, -1) \
  X(STEP, R, DT, FS_SEC_TABLE, 8, 4, 0, -1, 1, -1)

// polyline sections: fp64 only, a few shapes (the section evaluation dominates, not the elimination)
#define FS_LIST_IRREGULAR(X) \
  X(STEP, double, FS_F64, FS_SEC_IRREGULAR, 2, 1, 0, 0, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_IRREGULAR, 8, 1, 0, 0, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_IRREGULAR, 8, 4, 0, 0, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_IRREGULAR, 2, 1, 0, -1, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_IRREGULAR, 8, 1, 0, -1, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_IRREGULAR, 8, 4, 0, -1, 1, -1)

// the hot shapes once more without the history / residual-trace stores (DIAG = 0), for batches created without those flags
#define FS_LIST_NODIAG(X) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 0, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 2, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 1, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 8, 1, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1) \
  X(STEP, double, FS_F64, FS_SEC_TRAP_UNIFORM, 8, 1, 1, FS_BCK(FS_BC_RATING_POWER), 0, -1) \
  X(STEP, float, FS_F32, FS_SEC_TRAP_UNIFORM, 8, 1, 1, FS_BCK(FS_BC_RATING_POWER), 0, -1) \
  X(STEP, double, FS_F64, FS_SEC_TABLE, 2, 1, 0, 0, 0, -1) \
  X(STEP, double, FS_F64, FS_SEC_TABLE, 2, 1, 0, FS_BCK(FS_BC_RATING_BLEND), 0, -1) \
  X(STEP, double, FS_F64, FS_SEC_IRREGULAR, 2, 1, 0, 0, 0, -1) \
  X(STEP, double, FS_F64, FS_SEC_IRREGULAR, 2, 1, 0, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1)

// reaches longer than one lane grid (fs_long.hpp): capacity 64 M rows per wave slot x 64 slots
#define FS_LIST_LONG(X) \
  X(LONG, double, FS_F64, FS_SEC_RECT_UNIFORM, 8, 4, 0, 0, 1, -1) \
  X(LONG, double, FS_F64, FS_SEC_TRAP_UNIFORM, 8, 4, 0, 0, 1, -1) \
  X(LONG, double, FS_F64, FS_SEC_TABLE, 4, 4, 0, -1, 1, -1) \
  X(LONG, double, FS_F64, FS_SEC_IRREGULAR, 4, 4, 0, -1, 1, -1) \
  X(LONG, float, FS_F32, FS_SEC_RECT_UNIFORM, 8, 4, 0, 0, 1, -1) \
  X(LONG, float, FS_F32, FS_SEC_TRAP_UNIFORM, 8, 4, 0, 0, 1, -1) \
  X(LONG, float, FS_F32, FS_SEC_TABLE, 4, 4, 0, -1, 1, -1)

// The ensemble shape of BASELINE configs[3] (cases/gerd_roseires: 121 nodes in a 128-row lane grid, gate curve downstream) in its
// tail-only form (fs_kernel.hpp, TAIL): TAIL = (N - 1) mod M = the local row of the boundary row; ragged, no diagnostics; a batch
// with per-reach node counts takes the general ragged kernel instead
#define FS_LIST_TAIL(X) \
  X(STEP, double, FS_F64, FS_SEC_TABLE, 2, 1, 0, FS_BCK(FS_BC_RATING_BLEND), 0, 0) \
  X(STEP, double, FS_F64, FS_SEC_TABLE, 2, 1, 0, FS_BCK(FS_BC_RATING_BLEND), 0, 1)

// reaches longer than one lane grid as a team of workgroups (fs_kernel.hpp, TEAM): 64 W M rows per member, up to 64 / W members;
// uniform section modes.  FULL: N a whole number of lane grids (every row a cell but the very last one).  The DIAG = 0 ones are the
// benchmark shapes of bench.py --workload long (flow hydrograph in, normal depth out, no history), as the flagship has them
// (measured, profiles/round4/team_kernel.txt: 16 rows per lane - the fewest members - wins at every length; an (8, 4) shape with two
// workgroups per CU, one computing while the other waits for its team, ties at 8 192 nodes and loses beyond: twice the members to wait for.
// A TABLE (8, 4) team - 2 048 rows per member, 512 registers + 992 B of scratch - gains 3 - 7 % on cases/gerd_roseires at 25 m and 10 m
// (1.91e5 against 1.84e5, 8.2e4 against 7.7e4): a compound-section reach is bound by its section evaluations, not by the passes' traffic;
// not kept)
#define FS_LIST_TEAM(X) \
  X(TEAM, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 0, 1, 1, -1) \
  X(TEAM, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 0, 0, 1, -1) \
  X(TEAM, double, FS_F64, FS_SEC_TRAP_UNIFORM, 16, 4, 0, 0, 1, -1) \
  X(TEAM, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 0, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1) \
  X(TEAM, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1)

// FS_ACTIVE_LIST: the dispatch table of this build, in table order (FS_KERNEL_INDEX and fs_batch_kernel_index count along it).
#if !defined(FS_MINIMAL)
// the library: every list; the fs_part_*.hip translation units instantiate one list each (nodiag: FS_LIST_NODIAG and FS_LIST_TAIL)
#define FS_ACTIVE_LIST(X) \
  FS_LIST_RECT(X, double, FS_F64) FS_LIST_TRAP(X, double, FS_F64) FS_LIST_TABLE(X, double, FS_F64) \
  FS_LIST_RECT(X, float, FS_F32) FS_LIST_TRAP(X, float, FS_F32) FS_LIST_TABLE(X, float, FS_F32) \
  FS_LIST_IRREGULAR(X) FS_LIST_NODIAG(X) FS_LIST_LONG(X) FS_LIST_TAIL(X) FS_LIST_TEAM(X)

#elif FS_MINIMAL == 2   // experiment builds (fs_abi.hip alone, build_variants.sh): shapes for 512-node trapezoid reaches
#define FS_ACTIVE_LIST(X) \
  X(STEP, float, FS_F32, FS_SEC_TRAP_UNIFORM, 8, 1, 1, 0, 1, -1) \
  X(STEP, float, FS_F32, FS_SEC_TRAP_UNIFORM, 4, 2, 1, 0, 1, -1) \
  X(STEP, float, FS_F32, FS_SEC_TRAP_UNIFORM, 2, 4, 1, 0, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_TRAP_UNIFORM, 8, 1, 1, 0, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_TRAP_UNIFORM, 4, 2, 1, 0, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_TRAP_UNIFORM, 2, 4, 1, 0, 1, -1)

#elif FS_MINIMAL == 3   // experiment builds: the polyline kernels
#define FS_ACTIVE_LIST(X) FS_LIST_IRREGULAR(X)

#else                   // experiment builds and the sanitizer build of tests/test_sanitizers.py: the flagship shapes and one of each family
#ifdef FS_NO_TAIL
#define FS_MINIMAL_TAIL(X)
#else
#define FS_MINIMAL_TAIL(X) FS_LIST_TAIL(X)
#endif
#ifdef FS_TEAM_8X4
#define FS_MINIMAL_TEAM_8X4(X) X(TEAM, double, FS_F64, FS_SEC_RECT_UNIFORM, 8, 4, 0, 1, 1, -1)
#else
#define FS_MINIMAL_TEAM_8X4(X)
#endif
#define FS_ACTIVE_LIST(X) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 8, 8, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1) \
  X(STEP, double, FS_F64, FS_SEC_TABLE, 2, 1, 0, FS_BCK(FS_BC_RATING_BLEND), 0, -1) \
  FS_MINIMAL_TAIL(X) \
  X(STEP, double, FS_F64, FS_SEC_IRREGULAR, 2, 1, 0, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 1, 1, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 0, 1, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 8, 4, 1, 1, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 8, 8, 1, 1, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 4, 4, 1, 1, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 8, 1, 0, 1, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 4, 1, 0, 1, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 2, 1, 0, 1, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 4, 1, 0, 0, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_RECT_UNIFORM, 2, 1, 0, 0, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_TABLE, 2, 1, 0, 0, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_IRREGULAR, 2, 1, 0, 0, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_TRAP_UNIFORM, 8, 1, 1, 0, 1, -1) \
  X(STEP, float, FS_F32, FS_SEC_TRAP_UNIFORM, 8, 1, 1, 0, 1, -1) \
  X(STEP, float, FS_F32, FS_SEC_TRAP_UNIFORM, 8, 1, 1, FS_BCK(FS_BC_RATING_POWER), 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_TRAP_UNIFORM, 8, 1, 1, FS_BCK(FS_BC_RATING_POWER), 0, -1) \
  X(STEP, float, FS_F32, FS_SEC_RECT_UNIFORM, 8, 1, 1, 1, 1, -1) \
  X(STEP, float, FS_F32, FS_SEC_RECT_UNIFORM, 8, 1, 0, 1, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_TRAP_UNIFORM, 4, 1, 0, 0, 1, -1) \
  X(STEP, double, FS_F64, FS_SEC_TABLE, 4, 1, 0, 0, 1, -1) \
  X(LONG, double, FS_F64, FS_SEC_RECT_UNIFORM, 8, 4, 0, 0, 1, -1) \
  X(TEAM, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 0, 1, 1, -1) \
  X(TEAM, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 0, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1) \
  X(TEAM, double, FS_F64, FS_SEC_RECT_UNIFORM, 16, 4, 1, FS_BCK(FS_BC_NORMAL_DEPTH), 0, -1) \
  FS_MINIMAL_TEAM_8X4(X)
#endif
