/*
 * flowsim_abi.h - C ABI of the MI355X-native batched Preissmann stepper (libflowsim_hip.so).
 *
 * Drop-in boundary for ONE path of cve-mohd/flow-sim: the per-timestep Newton loop of
 * PreissmannSolver.run (reference: src/hydromodel/preissmann.py:101-163) together with everything
 * it calls per node (preissmann.py:61-99, :200-344, :407-798, :899-910; solver.py:244-296;
 * channel.py:53-105,:172-190; cross_section.py:114-175,:623-793; hydraulics.py:4-229;
 * boundary.py:56-247; rating_curve.py:32-63,:132-147; lumped_storage.py:24-45) and the sparse
 * solve it hands to scipy.sparse.linalg.spsolve (preissmann.py:146).
 *
 * The reference is pure Python and has no FFI of its own; the binding a maintainer would add is a
 * ctypes stub inside PreissmannSolver.run (shown in INTEGRATION.md).  Every entry point below
 * states which reference interface it stands in for.
 *
 * Conventions
 *   - plain C, no torch / numpy types; all host arrays are caller-owned, contiguous, float64
 *     (also for FS_F32 batches - converted on upload) unless stated otherwise;
 *   - B = reaches in the batch (independent channels / ensemble members), N = nodes per reach,
 *     level k = time level (k = 0 is the initial condition);
 *   - return 0 on success, <0 on error (text via fs_last_error(), thread-local);
 *   - a handle owns its device buffers and one HIP stream; it is not thread-safe;
 *   - calls are asynchronous on the handle's stream unless they copy to host memory.
 */
#ifndef FLOWSIM_ABI_H
#define FLOWSIM_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS_ABI_VERSION 3

typedef struct fs_batch fs_batch;

/* arithmetic type of the path (reference: float64 everywhere, solver.py:43-44).  FS_F32 is a throughput mode for large
 * ensembles of short reaches (BASELINE configs[4]): it holds 5e-4 of the fp64 answer at tolerance 1e-3, cannot resolve
 * ||R|| below ~6e-8 |Q| sqrt(2N) (4 096-node reaches need a tolerance of ~2e-2) and carries no 1e-8 parity claim. */
enum { FS_F64 = 0, FS_F32 = 1 };

/* How node geometry reaches the kernel.
 *   RECT_UNIFORM : one rectangular prismatic channel per reach from per-reach scalars
 *                  (what Channel(width=, roughness=) builds, channel.py:282-294);
 *   TRAP_UNIFORM : one simple (non-compound) trapezoidal prismatic channel per reach from
 *                  per-reach scalars (two TrapezoidalSection(z_bank=None) end sections with equal
 *                  b_main / m_main / n_main, cross_section.py:641-645; BASELINE configs[4]);
 *   TABLE        : one [FS_GEO_NPARAM][N] table of TrapezoidalSection parameters at the nodes
 *                  (cross_section.py:569-613 after interpolation, channel.py:213-241), shared by
 *                  all reaches, optional per-reach main-channel Manning n
 *                  (cases/gerd_roseires/custom_functions.py:147).
 *   IRREGULAR    : TABLE plus polyline nodes: what Channel.xs_at_node holds when any input
 *                  section is an IrregularSection (cross_section.py:207-543; mixed interpolation
 *                  :932-968).  fp64 only (the reference's 1e-6 finite differences do not survive
 *                  single precision). */
enum { FS_SEC_RECT_UNIFORM = 0, FS_SEC_TRAP_UNIFORM = 1, FS_SEC_TABLE = 2, FS_SEC_IRREGULAR = 3 };

/* rows of the RECT_UNIFORM parameter block, each [B] */
enum { FS_RU_WIDTH = 0, FS_RU_MANNING = 1, FS_RU_Z_US = 2, FS_RU_Z_DS = 3, FS_RU_NPARAM = 4 };
/* rows of the TRAP_UNIFORM parameter block, each [B]: the four above + the side slope m (H:V) */
enum { FS_TU_SIDE_SLOPE = 4, FS_TU_NPARAM = 5 };

/* rows of the TABLE geometry block, each [N] (TrapezoidalSection attributes) */
enum {
  FS_GEO_Z_BED = 0, FS_GEO_B_MAIN, FS_GEO_M_MAIN, FS_GEO_N_MAIN, FS_GEO_N_LEFT, FS_GEO_N_RIGHT,
  FS_GEO_IS_COMPOUND, FS_GEO_H_BANKFULL, FS_GEO_B_FP_LEFT, FS_GEO_B_FP_RIGHT, FS_GEO_M_FP,
  FS_GEO_CURVATURE, FS_GEO_NPARAM
};

/* Boundary.condition (boundary.py:32) flattened; rating_curve split by RatingCurve.type
 * (rating_curve.py:10-31) plus the smooth Roseires gate curve of cases/gerd_roseires
 * (roseires_rating_curve.py:65-109,:202-208) and fixed_depth behind a constant-area
 * LumpedStorage (boundary.py:97-133, lumped_storage.py:24-45). */
enum {
  FS_BC_FLOW_HYDROGRAPH = 0,  /* params: -                      ; needs target table          */
  FS_BC_STAGE_HYDROGRAPH = 1, /* params: bed_level              ; needs target table          */
  FS_BC_FIXED_DEPTH = 2,      /* params: initial_depth                                        */
  FS_BC_NORMAL_DEPTH = 3,     /* params: bed_slope, bed_level                                 */
  FS_BC_RATING_POWER = 4,     /* params: a, b, stage_shift, bed_level                         */
  FS_BC_RATING_POLY = 5,      /* params: a, b, c, stage_shift, bed_level                      */
  FS_BC_RATING_BLEND = 6,     /* params: stage0, buffer, lo0, lo1, lo2, hi0, hi1, hi2, dY, bed_level
                                 Q = (1-s)*lo(z) + s*hi(z), lo/hi quadratics in z, s = smoothstep */
  FS_BC_STORAGE = 7,          /* params: surface_area, min_stage, Y_min, Y_max, bed_level (downstream only) */
  FS_BC_STORAGE_CURVE = 8,    /* general LumpedStorage (lumped_storage.py:8-179; downstream only): area curve,
                                 reservoir rating curve, entrance losses.  params[FS_SC_NFIXED + 2*n_curve]:
                                 the FS_SC_* scalars, then stage[n_curve], area[n_curve] of set_area_curve
                                 (n_curve = 0: constant surface_area).  The mass-balance root
                                 (lumped_storage.py:24-35) is found on the device with the algorithm of
                                 scipy.optimize.brentq and its default tolerances.  Section modes
                                 FS_SEC_TABLE and FS_SEC_IRREGULAR only (fs_batch_step refuses it in the
                                 uniform-geometry modes: describe such a channel as a table).  Shared by the
                                 batch (per_reach = 0) or one reservoir per reach (per_reach = 1:
                                 params[FS_SC_NFIXED + 2*n_curve][B], the same n_curve for every reach). */
  FS_BC_HOST_ROW = 9          /* a boundary whose plugin has no device form: any object with discharge(stage, time) /
                                 dQ_dz(stage, time) (rating_curve.py:32-63,:132-147; e.g. RoseiresRatingCurve(smooth=False),
                                 cases/gerd_roseires/roseires_rating_curve.py:65-140, whose gates move with time) or a
                                 LumpedStorage with a callable rating curve (lumped_storage.py:24-35).  params[3][B]
                                 (per_reach = 1) = (d/dh, d/dQ, residual) of the boundary equation at the current Newton
                                 vector, evaluated by the caller before every iteration (boundary.py:56-242) and handed over
                                 with fs_batch_set_host_rows; such a batch advances with fs_batch_iterate (one Newton
                                 iteration per launch), not fs_batch_step.  Section modes FS_SEC_TABLE / FS_SEC_IRREGULAR. */
};
/* scalar slots of FS_BC_STORAGE_CURVE */
enum {
  FS_SC_MIN_STAGE = 0, FS_SC_Y_MIN, FS_SC_Y_MAX, FS_SC_BED_LEVEL, FS_SC_SURFACE_AREA, FS_SC_ALPHA, FS_SC_BETA,
  FS_SC_N_CURVE,
  FS_SC_RC_TYPE,            /* 0: no outflow, 1: power a*(Y+shift)^b, 2: polynomial a*x^2 + b*x + c (rating_curve.py:10-63) */
  FS_SC_RC_A, FS_SC_RC_B, FS_SC_RC_C, FS_SC_RC_SHIFT,
  FS_SC_CAPTURE_LOSSES,     /* LumpedStorage.capture_losses (0/1) */
  FS_SC_RESERVOIR_LENGTH, FS_SC_K_Q,
  FS_SC_NFIXED
};
#define FS_BC_MAX_PARAMS 10   /* of the fixed-size kinds 0..7 */
enum { FS_UPSTREAM = 0, FS_DOWNSTREAM = 1 };

/* per-reach status after stepping (preissmann.py:124-126 raises ValueError; :135-137 NaN check)
 *
 * FS_MAX_ITER, FS_NAN and FS_STORAGE_RANGE are failures: the reach stops at the level it failed on (the FAILING LEVEL), the status
 * sticks, and later fs_batch_step / fs_batch_iterate calls leave the reach alone until fs_batch_restart (or a new initial state)
 * begins again from FS_OK.  The other reaches of the batch are not affected.  After a failure
 *  - fs_batch_get_iterations holds, at the failing level, the number of Newton iterations that level began before it gave up:
 *      FS_MAX_ITER        max_iter (the reference's "Convergence within N iterations couldn't be achieved"),
 *      FS_NAN             the iteration whose residual norm was not finite,
 *      FS_STORAGE_RANGE   the iteration whose reservoir row found no stage in [Y_min, Y_max] (brentq's ValueError in the reference);
 *    the rows of later levels are 0, the rows of earlier levels the counts of those levels;
 *  - the rows of fs_batch_get_hydrographs, fs_batch_get_history, fs_batch_get_storage_stages and fs_batch_get_residual_trace BEFORE
 *    the failing level are complete and are what a run without the failure gives; the rows of the failing level and of later
 *    levels are not written (hydrograph and storage-stage rows read 0 in a batch that has not held other results there, history
 *    rows are undefined, and so is the trace row of the failing level);
 *  - fs_batch_get_state and fs_batch_get_storage_stage are the state and the reservoir stage at the end of the previous call
 *    (see there): a pair that belongs to one level, whatever levels the reach completed in the failing call before it failed;
 *  - fs_batch_get_guess is the Newton vector of the failing level after its last update - it holds NaN after FS_NAN - and not a
 *    start vector for anything (after FS_MAX_ITER with max_iter = m it is the m-th Newton iterate of that level, which is what
 *    tests/test_gpu_newton_iterates.py holds to the reference's iterates for every step kernel): a caller that wants to go on from the last good level restarts from a (state, guess, stage)
 *    triple it read before the failing call (fs_batch_restart), which is also how the level can be tried again with other inputs. */
enum { FS_OK = 0, FS_MAX_ITER = 1, FS_NAN = 2, FS_STORAGE_RANGE = 3,
       /* A warning, not a failure (the reach keeps stepping and the status sticks): the linear systems of this reach are
        * ill-conditioned - in practice supercritical flow (v > c) over a long stretch, where one boundary condition per end
        * is not what the flow takes.  The on-chip elimination does not pivot; it watches how strongly the first unknown of any
        * segment of rows depends on the last one (a product of super-diagonal / pivot ratios that decays for subcritical
        * flow) and raises this status when that exceeds 2^10 in the iteration that accepts a level: results may then differ from another solver's (the reference's
        * SuperLU included) by more than the 1e-8 this library otherwise keeps.  The reference's counterpart is the
        * `diagnos` check of run(), ValueError("Jacobian is ill-conditioned (rcond too small)"), preissmann.py:139-144, and
        * the Froude diagnosis of check_criticality (:179-198).  Raised by the kernels compiled with diagnostics: every batch
        * with FS_FLAG_HISTORY, FS_FLAG_TRACE or FS_FLAG_MONITOR, and every batch no specialised kernel exists for. */
       FS_ILL_CONDITIONED = 4,
       /* A reach longer than one lane grid is advanced by a team of workgroups that meet once per Newton iteration (uniform section
        * modes beyond 4 096 nodes).  A member that waits for the others longer than about eight seconds gives the reach up with this
        * status instead of spinning on; it has not been seen to happen (a team's members are the workgroups that started first, so
        * none of them waits for one that cannot start) and would mean a lost or wedged workgroup.  The reach's state is that of the
        * last launch that completed. */
       FS_TEAM_STALL = 5 };

enum {
  FS_FLAG_HISTORY = 1,  /* keep depth/flow[level][B][N] on the device (solver.py:43-44); large batches that only need the
                           boundary hydrographs leave it (and FS_FLAG_TRACE) off: no [levels][B][N] arrays in HBM and
                           step kernels compiled without those stores */
  FS_FLAG_TRACE = 2,    /* keep ||R|| of every Newton iteration (what run(verbose=3) prints, preissmann.py:149-152) */
  FS_FLAG_MONITOR = 4   /* run the conditioning monitor (FS_ILL_CONDITIONED) also on a batch that keeps neither history nor trace:
                           selects the kernels compiled with diagnostics (measured: 1.2 % slower on the 4 096-node benchmark shape, 3 % on
                           the 121-node ensemble).  The Python binding sets it by default (PreissmannBatch(monitor=True), the reference's
                           per-run `diagnos` check stands behind it, preissmann.py:133-144); a caller that wants the fastest kernels and
                           knows its flow to be subcritical passes monitor=False, as bench.py does. */
};
#define FS_TRACE_CAP 64 /* iterations per level kept by FS_FLAG_TRACE */

typedef struct fs_batch_desc {
  int32_t n_reaches;     /* B */
  int32_t n_nodes;       /* N >= 2; up to 4 096 (uniform section modes) / 2 048 (tables, polylines) a reach stays on chip, longer ones -
                            to 32 768 / 16 384 nodes - run on the multi-pass kernel (state and level constants through L2) */
  int32_t dtype;         /* FS_F64 | FS_F32 */
  int32_t section_mode;  /* FS_SEC_* */
  int32_t device;        /* HIP device ordinal */
  int32_t max_levels;    /* capacity of per-level tables: time levels 0..max_levels-1 (solver.py:35) */
  int32_t flags;         /* FS_FLAG_* */
  int32_t reserved;
} fs_batch_desc;

int fs_abi_version(void);
int fs_device_count(void);                 /* 0 when no HIP device is visible */
const char *fs_last_error(void);

/* Solver.__init__ state arrays + PreissmannSolver.__init__ (solver.py:11-51, preissmann.py:23-46) */
fs_batch *fs_batch_create(const fs_batch_desc *desc);
void fs_batch_destroy(fs_batch *b);

/* theta / time_step / spatial_step of the solver and tolerance / max_iter of run()
 * (preissmann.py:23-46, :101; solver.py:32, :53-55) - shared by the whole batch */
int fs_batch_set_scheme(fs_batch *b, double theta, double dt, double dx, double tolerance, int32_t max_iter);

/* RECT_UNIFORM: params[FS_RU_NPARAM][B];  TRAP_UNIFORM: params[FS_TU_NPARAM][B] */
int fs_batch_set_geometry_uniform(fs_batch *b, const double *params);
/* TABLE: table[FS_GEO_NPARAM][N]; n_main_override[B] or NULL */
int fs_batch_set_geometry_table(fs_batch *b, const double *table, const double *n_main_override);
/* IRREGULAR: table[FS_GEO_NPARAM][N] as for TABLE.  Node i with n_pts[i] > 0 is the polyline
 * x[i][0..n_pts[i]), z[i][..] (rows of length max_pts, x ascending, >= 2 points; IrregularSection.x/.z
 * after its argsort, cross_section.py:231-233) with roughness strips split at limits[i][0..1]
 * (left_fp_limit, right_fp_limit, +-inf allowed; cross_section.py:105-111); of its table column only
 * Z_BED (= min z), N_MAIN, N_LEFT, N_RIGHT and CURVATURE are read.  n_pts[i] == 0: trapezoid-family
 * node described by the table column.  n_main_override[B] or NULL. */
int fs_batch_set_geometry_irregular(fs_batch *b, const double *table, const int32_t *n_pts, int32_t max_pts,
                                    const double *x, const double *z, const double *limits,
                                    const double *n_main_override);

/* Heterogeneous batches: every reach its own channel - what the reference builds per Channel / Solver object
 * (channel.py:213-241 node sections, cross_section.py:857-930 interpolation, solver.py:34-38,53-55 grid) - so that different
 * rivers, or a geometry Monte-Carlo of one river (bed levels, widths, bankfull depths), step in one launch.
 *   fs_batch_set_geometry_table_per_reach      tables[B][FS_GEO_NPARAM][N]: one TrapezoidalSection table per reach (FS_SEC_TABLE);
 *   fs_batch_set_geometry_irregular_per_reach  the same for FS_SEC_IRREGULAR: tables[B][FS_GEO_NPARAM][N], n_pts[B][N],
 *                                              x / z [B][N][max_pts], limits[B][N][2];
 *   fs_batch_set_reach_nodes                   n_nodes[B], 2 <= n_nodes[r] <= N of the batch (NULL: all N): reach r uses the
 *                                              first n_nodes[r] entries of its rows of every [B][N] array (state, tables - pad the
 *                                              rest with the last node's values -, history); entries beyond are left untouched;
 *   fs_batch_set_reach_scheme                  theta[B], dt[B], dx[B] (any may be NULL: the batch-wide value of
 *                                              fs_batch_set_scheme, which is called first);
 *   fs_batch_set_reach_tolerance               tolerance[B], max_iter[B] (either may be NULL: the batch-wide value): every run() of the reference
 *                                              has its own tolerance and iteration cap (preissmann.py:101);
 *   fs_batch_set_bc_per_reach                  kinds[B] (FS_BC_FLOW_HYDROGRAPH .. FS_BC_STORAGE, and FS_BC_HOST_ROW on the reaches whose
 *                                              plugin has no device form), params[FS_BC_MAX_PARAMS][B] (row i = parameter i of the
 *                                              reach's own kind, unused rows ignored), target[max_levels][B];
 *   fs_batch_set_bc_per_reach_wide             the same with params[n_params][B], n_params >= FS_BC_MAX_PARAMS: room for reaches of kind
 *                                              FS_BC_STORAGE_CURVE (a general reservoir behind some channels of the batch, each with
 *                                              its FS_SC_* rows and an area curve of its own length: FS_SC_NFIXED + 2*n_curve <= n_params).
 * Time level k of reach r is t = k * dt[r]: targets are sampled per reach.  These batches run on the general kernels (run-time
 * boundary switch, ragged node counts).  One FS_BC_HOST_ROW reach makes the batch one that advances with fs_batch_iterate (TABLE /
 * IRREGULAR section modes): the reference runs a RatingCurve subclass on one channel next to closed-form boundaries on the others
 * (boundary.py:56-141 is per Boundary object), and so does a batch. */
int fs_batch_set_geometry_table_per_reach(fs_batch *b, const double *tables, const double *n_main_override);
int fs_batch_set_geometry_irregular_per_reach(fs_batch *b, const double *tables, const int32_t *n_pts, int32_t max_pts,
                                              const double *x, const double *z, const double *limits,
                                              const double *n_main_override);
/* Geometry ensembles of ONE surveyed channel (FS_SEC_IRREGULAR): what the reference does by building one Channel of
 * IrregularSections per member (cross_section.py:205-246; z_min :231-233; the roughness strips of get_equivalent_n :449-500) is done
 * on the device from the shared channel - table, n_pts, x, z, limits exactly as fs_batch_set_geometry_irregular takes them, every
 * node a polyline (n_pts[i] > 0) - and a transform per member r:
 *   z'_j = z_j + dz_strip(j)[r][i]: vertex j of node i is in the left strip where x_j < limits[i][0], in the right one where
 *   x_j > limits[i][1], in the main channel otherwise; dz_left / dz_main / dz_right [B][N] each, or NULL (= 0);
 *   (n_left, n_main, n_right)' = (n_left, n_main, n_right)_i * n_scale[0..2][r]; n_scale [3][B] or NULL (= 1);
 *   Z_BED'[r][i] = min_j z'_j.  x, the limits and the curvature stay.
 * The batch is then where fs_batch_set_geometry_irregular_per_reach of the B transformed channels leaves it - polylines, tables and
 * stage tables (cross_section.py:248-328 summed per interval) bit for bit - without their n_sets * N * poly_table_stride doubles
 * built, staged and uploaded by the host.  FS_POLY_WALK / FS_POLY_TABLE_MAX_BYTES keep their meaning (fs_batch_poly_tables).  A
 * main-channel override (n_main_override of the other setters) is cleared: n_scale[1] takes its place.  The call returns when the
 * members are built; until the next fs_batch_step, fs_batch_last_step_ms reports the HIP-event time of its kernels.
 *   fs_batch_get_stage_table   node's stage table of reach `reach` (ignored where the batch shares one channel), however it was
 *                              built: out[max_pts + 16 rounded down to a multiple of 16, + 32 * max_pts]: the breakpoints padded
 *                              with +inf, then 32 doubles per interval; an error when the batch walks its polylines' edges;
 *   fs_batch_get_bed_levels    out[B][N]: row Z_BED of every reach's table (FS_SEC_TABLE / FS_SEC_IRREGULAR) - a member's boundary
 *                              rows take their bed_level from here (boundary.py:24-25). */
int fs_batch_set_geometry_irregular_members(fs_batch *b, const double *table, const int32_t *n_pts, int32_t max_pts,
                                            const double *x, const double *z, const double *limits,
                                            const double *dz_left, const double *dz_main, const double *dz_right,
                                            const double *n_scale);
int fs_batch_get_stage_table(fs_batch *b, int32_t reach, int32_t node, double *out);
int fs_batch_get_bed_levels(fs_batch *b, double *out);
int fs_batch_set_reach_nodes(fs_batch *b, const int32_t *n_nodes);
int fs_batch_set_reach_scheme(fs_batch *b, const double *theta, const double *dt, const double *dx);
int fs_batch_set_reach_tolerance(fs_batch *b, const double *tolerance, const int32_t *max_iter);
int fs_batch_set_bc_per_reach(fs_batch *b, int32_t side, const int32_t *kinds, const double *params, const double *target);
int fs_batch_set_bc_per_reach_wide(fs_batch *b, int32_t side, const int32_t *kinds, const double *params, int32_t n_params,
                                   const double *target);

/* one boundary (Boundary.__init__, boundary.py:10-46).  params[n_params] when per_reach == 0,
 * params[n_params][B] otherwise.  target[max_levels][B] (value at t = level*dt, i.e.
 * Hydrograph.get_at pre-sampled, hydrograph.py:15-22) or NULL. */
int fs_batch_set_bc(fs_batch *b, int32_t side, int32_t kind, const double *params, int32_t n_params,
                    int32_t per_reach, const double *target);

/* Channel.initial_conditions (channel.py:107-138) -> depth[0], flow[0] and the Newton start
 * vector (solver.py:61-63, preissmann.py:48-59).  h, Q: [B][N].  Resets the level counter. */
int fs_batch_set_state(fs_batch *b, const double *h, const double *Q);

/* Same for the 'steady-state' initial condition of a prismatic reach (channel.py:296-305: one
 * normal depth and the initial flow at every node): h[B], Q[B], broadcast along the reach on
 * the device (avoids staging B*N host values for large batches). */
int fs_batch_set_state_uniform(fs_batch *b, const double *h, const double *Q);

/* Channel.initialize_conditions (channel.py:107-138) on the device, on the geometry the batch holds: call it after the scheme, the
 * geometry and, where used, fs_batch_set_reach_nodes / fs_batch_set_reach_scheme (a reach's spatial step is its own dx).  flow[B] is
 * each reach's flow at every node.
 *   FS_IC_LINEAR  depth_us[B], depth_ds[B]: h_i = h_us + (h_ds - h_us) x_i / L (channel.py:380-390)
 *   FS_IC_GVF     depth_ds[B]: the backwater march from the downstream depth (channel.py:307-378)
 *   FS_IC_STEADY  normal depth at every node (channel.py:296-305); bed_slope: the nodes' interpolated CrossSection.bed_slope, [N]
 *                 shared or [B][N] (bed_slope_per_reach != 0); NULL in the two uniform modes: (z_us - z_ds) / ((n_r - 1) dx_r),
 *                 channel.py:286.  A NaN entry is the reference's None: "Bed slope must be defined.", the call fails.
 * The batch is then in the state fs_batch_set_state leaves when given the same values (nodes beyond a reach's own last one repeat
 * it).  A reach whose march met Fr > 1 keeps NaN depth at the nodes it did not reach: a later step reports FS_NAN for it.
 * info: NULL, or [2][B]: the FS_IC_* flag bits of each reach, then the node of its first supercritical evaluation (else -1).  The
 * call synchronises only when info is given. */
enum { FS_IC_LINEAR = 0, FS_IC_GVF = 1, FS_IC_STEADY = 2 };
/* bits of info[0][r]: the march stopped at Fr > 1; 1 - Fr^2 was replaced by 0.01; a depth <= 0 was set to 0.01; brentq found no
 * bracket (the result is one of the reference's fall-backs, cross_section.py:195-202) */
enum { FS_IC_SUPERCRITICAL = 1, FS_IC_CLAMPED = 2, FS_IC_FLOORED = 4, FS_IC_NO_ROOT = 8 };
int fs_batch_init_state(fs_batch *b, int32_t method, const double *flow, const double *depth_us, const double *depth_ds,
                        const double *bed_slope, int32_t bed_slope_per_reach, int32_t *info);

/* ---- Boundary forcing built on the device ----
 * What a hydrograph boundary follows, target[max_levels][B], computed where it is read instead of sampled on the host and uploaded.
 * Both steps compute in fp64 whatever the batch dtype and round once when they store into the target.
 *
 * fs_batch_set_bc_sampled: fs_batch_set_bc(b, side, kind, params, n_params, 0, target) for FS_BC_FLOW_HYDROGRAPH and
 * FS_BC_STAGE_HYDROGRAPH with
 *     target[k][r] = offset[r] + scale[r] * np.interp(k * dt_r - shift[r], times, values[table_of[r]])
 * i.e. Hydrograph.sample (hydrograph.py:26-32: np.interp over np.arange(n) * dt, end values held outside the table) of a table that
 * member r scales, lifts and delays; scale, offset and shift NULL are 1, 0 and 0, and such a member's column is bit for bit what
 * Hydrograph.sample returns.  times[n_pts] strictly increasing and shared, values[n_tables][n_pts], table_of[B] in 0 .. n_tables - 1
 * (NULL: table 0).  dt_r is the reach's own step where fs_batch_set_reach_scheme gave one, else the batch's: the scheme (and the
 * per-reach scheme, where used) must be set first, and a later change of dt does not resample.  The same validation as
 * fs_batch_set_bc.  The call waits for the batch's earlier work before it uploads its inputs (blocking copies) and does not wait for
 * its own kernel; if it fails after the arguments were accepted, the side is left without a boundary. */
int fs_batch_set_bc_sampled(fs_batch *b, int32_t side, int32_t kind, const double *params, int32_t n_params, const double *times,
                            const double *values, int32_t n_pts, int32_t n_tables, const int32_t *table_of, const double *scale,
                            const double *offset, const double *shift);
/* fs_batch_route_pool: level-pool routing of the side's target through a reservoir, GerdHydrograph.build
 * (cases/gerd_roseires/gerd_discharge.py:12-56) generalised to data, every member with its own pool.  The side must hold an
 * FS_BC_FLOW_HYDROGRAPH target: it is read as the inflow and overwritten, in place, with the release; the pool's stage goes to a buffer
 * of the handle (fs_batch_get_pool_stages).  Per level k = 1 .. max_levels - 1 (gerd_discharge.py:25-56), with V = np.interp over
 * (curve_stage, curve_volume):
 *     f(z1) = (V(z1) - V(z0)) - (0.5 (qin1 + qin0) - 0.5 (release(qin1, z1) + qout0)) * dt_r * vol_scale
 *     z1 = brentq(f, z_lo, z_hi) (scipy's defaults);  qout1 = release(qin1, z1)
 * and level 0 is z0 = initial_stage[r], qout0 = release(qin0, z0).  release (gerd_discharge.py:58-68): above the member's hold level -
 * its initial stage - the outlet capacity, at or below it max(min(inflow, capacity), base_flow).  capacity (gerd_discharge.py:70-94):
 *     sum over the weirs of C_w * weir_scale[w][r] * max(0, z - crest_w)^1.5 * ramp_w(z), plus base_flow
 * ramp_w rises linearly from 0 at crest_w to 1 at ramp_top_w (gerd_discharge.py:96-105) and is 1 where ramp_top_w <= crest_w.
 * curve_stage[n_curve] strictly increasing, 2 <= n_curve <= 64; weirs[n_w][4] = C, crest, ramp_top, 0 (reserved), 0 <= n_w <= 8;
 * vol_scale turns m3 into the curve's unit (GERD: 1e-6); z_lo < z_hi; initial_stage[B]; weir_scale[n_w][B] or NULL (1: gates out of
 * service are 0).  A member whose f has one sign at both ends of the bracket at some level (brentq's ValueError) gets
 * FS_POOL_NO_BRACKET; its target rows and stages from that level on are NaN, so that a later step reports FS_NAN for it; the rows before
 * are complete.  info: NULL, or [2][B]: the FS_POOL_* bits of each member, then the first level without a bracket (else -1).  The call
 * waits for the batch's earlier work before it uploads its inputs (blocking copies); it waits for its own kernel only when info is
 * given. */
enum { FS_POOL_NO_BRACKET = 1 };
int fs_batch_route_pool(fs_batch *b, int32_t side, const double *curve_stage, const double *curve_volume, int32_t n_curve,
                        const double *weirs, int32_t n_w, double base_flow, double vol_scale, double z_lo, double z_hi,
                        const double *initial_stage, const double *weir_scale, int32_t *info);
/* rows first .. first + n - 1 of the side's target as the kernels read it, out[n][B]: after fs_batch_set_bc the caller's table,
 * after fs_batch_set_bc_sampled the samples, after fs_batch_route_pool the release (Hydrograph.table[:, 1] of the built
 * GerdHydrograph; row 0 is what model.py:73 takes as the channel's initial flow) */
int fs_batch_get_bc_target(fs_batch *b, int32_t side, int32_t first, int32_t n, double *out);
/* the pool stage of every level of the last fs_batch_route_pool (stage_1 of gerd_discharge.py:45, which the reference does not keep),
 * out[n][B] in fp64 */
int fs_batch_get_pool_stages(fs_batch *b, int32_t first, int32_t n, double *out);

/* THE HOT PATH: advances every reach by n_steps time levels (preissmann.py:108-161).  Results
 * stay on the device: boundary hydrographs, Newton counts, status, (history).  Asynchronous. */
int fs_batch_step(fs_batch *b, int32_t n_steps);
int fs_batch_sync(fs_batch *b);
int32_t fs_batch_level(const fs_batch *b);   /* current time level k */

/* The same loop opened up for boundaries evaluated on the host (FS_BC_HOST_ROW): ONE Newton iteration
 * (preissmann.py:122-156: residual, Jacobian, solve, update, norm test) of level fs_batch_level() + 1 for every reach
 * that has not converged on it yet.  *n_open (may be NULL) returns how many reaches still iterate; when it reaches 0
 * the level is complete for the whole batch and fs_batch_level() has advanced.  Synchronous.  Works for any TABLE /
 * IRREGULAR batch (device-evaluated kinds included). */
int fs_batch_iterate(fs_batch *b, int32_t *n_open);
/* rows[3][B] = (d/dh, d/dQ, residual) of the side's boundary equation at the current Newton vector
 * (Boundary.df_dh, df_dQ, condition_residual: boundary.py:143-242, :56-141).  On a side with per-reach kinds the entries of the
 * reaches whose kind the device evaluates are ignored (their parameters stay). */
int fs_batch_set_host_rows(fs_batch *b, int32_t side, const double *rows);
/* the current Newton vector at the two boundary nodes, out[4][B] = h[0], Q[0], h[N-1], Q[N-1]
 * (what preissmann.py:200-218, :303-320 pass to the boundary: depth_at / flow_at of the iterate) */
int fs_batch_get_boundary_iterate(fs_batch *b, double *out);

/* Restart (the reference keeps its whole history in memory and has no restart, solver.py:43-44):
 * everything a run needs to continue bit-exactly from time level `level`: depth/flow[level] (h, Q: what
 * fs_batch_get_state returned), the Newton start vector of level+1 (h_guess, Q_guess: fs_batch_get_guess; after the
 * first level it differs from the state) and, behind a storage boundary, the reservoir stage of `level`
 * (storage_stage[B]: fs_batch_get_storage_stage; required behind a storage boundary when level > 0, NULL otherwise).  All
 * [B][N] float64.  A batch that keeps a history (FS_FLAG_HISTORY) holds, after a restart, the rows from `level` on:
 * fs_batch_get_history / fs_batch_derive refuse ranges that begin before it, and the amplitude fields of fs_batch_derive
 * (solver.py:96-97: depth - depth[0]) then refer to the restart state.  The per-reach status starts from FS_OK again. */
int fs_batch_restart(fs_batch *b, int32_t level, const double *h, const double *Q, const double *h_guess,
                     const double *Q_guess, const double *storage_stage);

/* depth[k], flow[k] of the current level (what update_guesses stored, preissmann.py:166-177).
 * The kernel writes the accepted state to HBM at the last level of each fs_batch_step call (and at
 * every level into the history when FS_FLAG_HISTORY is set); for a reach whose status is not FS_OK
 * this is therefore the state at the end of the previous call. */
int fs_batch_get_state(fs_batch *b, double *h, double *Q);
/* the post-update Newton vector that seeds the next level (preissmann.py:146-147); for a reach whose status is a failure: the
 * vector the failing level ended with (see the status enum) */
int fs_batch_get_guess(fs_batch *b, double *h, double *Q);
/* out[n_levels][4][B] = depth[k,0], flow[k,0], depth[k,-1], flow[k,-1] for k = first..first+n-1
 * (what cases read from solver.depth / solver.flow, cases/gerd_roseires/model.py:107-111) */
int fs_batch_get_hydrographs(fs_batch *b, int32_t first_level, int32_t n_levels, double *out);
int fs_batch_get_iterations(fs_batch *b, int32_t first_level, int32_t n_levels, int32_t *out); /* [n][B] */
int fs_batch_get_status(fs_batch *b, int32_t *out);                                            /* [B]   */
/* FS_FLAG_HISTORY only: h, Q [n_levels][B][N] (solver.depth / solver.flow, solver.py:43-44) */
int fs_batch_get_history(fs_batch *b, int32_t first_level, int32_t n_levels, double *h, double *Q);
/* FS_FLAG_TRACE only: out[n_levels][FS_TRACE_CAP][B] residual norms, iteration i of level k at
 * [k][i-1][reach]; entries beyond the iteration count of a level are 0 */
int fs_batch_get_residual_trace(fs_batch *b, int32_t first_level, int32_t n_levels, double *out);
/* reservoir stage kept per level by the storage boundary (boundary.py:126-131): out[B] */
int fs_batch_get_storage_stage(fs_batch *b, double *out);
/* the same per time level (LumpedStorage.stage_hydrograph, boundary.py:126-131): out[n_levels][B],
 * rows of levels that have not been computed (and level 0) are 0 */
int fs_batch_get_storage_stages(fs_batch *b, int32_t first_level, int32_t n_levels, double *out);

/* Solver.prepare_results (solver.py:65-127) for levels [first, first+n) of the stored history
 * (FS_FLAG_HISTORY): level = depth + bed, area, top width, Froude number (hydraulics.py:155-168),
 * velocity Q/A, wave celerity V + sqrt(g A / T), amplitude = depth - depth[0]; each [n][B][N], and
 * peak_amplitude [B][N] = max over those levels.  Any output pointer may be NULL.  One elementwise,
 * HBM-bound kernel; results are copied to the caller's host arrays (the device buffers behind them are
 * kept by the handle and reused by later calls). */
int fs_batch_derive(fs_batch *b, int32_t first_level, int32_t n_levels, double *level, double *area,
                    double *top_width, double *froude, double *velocity, double *celerity,
                    double *amplitude, double *peak_amplitude);
/* The same kernel with the results left on the device (no PCIe traffic): fields = bit mask of FS_DERIVE_* to
 * compute; fs_batch_derived_device_ptr(field index 0..7) then points at [n_levels][B][N] (index 7,
 * peak amplitude: [B][N]) in the batch dtype, valid until the next derive call on this handle. */
enum { FS_DERIVE_LEVEL = 1, FS_DERIVE_AREA = 2, FS_DERIVE_TOP_WIDTH = 4, FS_DERIVE_FROUDE = 8, FS_DERIVE_VELOCITY = 16,
       FS_DERIVE_CELERITY = 32, FS_DERIVE_AMPLITUDE = 64, FS_DERIVE_PEAK_AMPLITUDE = 128, FS_DERIVE_ALL = 255 };
int fs_batch_derive_device(fs_batch *b, int32_t first_level, int32_t n_levels, int32_t fields);
void *fs_batch_derived_device_ptr(fs_batch *b, int32_t field_index);

/* ---- Ensemble post-processing on the device ----
 * Three reductions of the boundary hydrograph block (what fs_batch_get_hydrographs downloads) over the levels [first, first + n),
 * which must lie inside 0 .. fs_batch_level() (after fs_batch_restart: from the restart level on).  They read the block where it is,
 * accumulate in fp64 whatever the batch dtype, copy only their results to the caller's host arrays, and synchronise.  A reach whose
 * status is a failure (FS_MAX_ITER, FS_NAN, FS_STORAGE_RANGE, FS_TEAM_STALL; see the status enum) enters the per-reach reductions with
 * the rows BEFORE its failing level only - the rows the status enum documents as complete - and is left out of the cross-member one;
 * FS_ILL_CONDITIONED is a warning and changes nothing.
 *
 * fs_batch_summarize: the numbers of the reference's result summary (solver.py:203-229) for every reach, out[FS_SUM_NROWS][B].  Level
 * indices are relative to `first`, as doubles; the caller multiplies by the reach's own dt.  The median-volume level is the reference's
 * loop as written (solver.py:219-229): with cum_i = sum(Q[:i]), i = 0 .. m-1, the first i with cum_i >= 0.5 cum_{m-1}.  A reach that
 * completed no row of the range reports FS_SUM_LEVELS 0, sums 0, peaks NaN and levels -1. */
enum { FS_SUM_LEVELS = 0,            /* rows of the range this reach completed */
       FS_SUM_Q_IN, FS_SUM_Q_OUT,    /* np.sum(Q_in), np.sum(Q_out) (solver.py:207) */
       FS_SUM_Q_NET,                 /* np.sum(Q_in - Q_out), accumulated as the difference (solver.py:206) */
       FS_SUM_PEAK_Q_IN,  FS_SUM_PEAK_Q_IN_LEVEL,      /* np.max / np.argmax (solver.py:211-212) */
       FS_SUM_PEAK_Q_OUT, FS_SUM_PEAK_Q_OUT_LEVEL,
       FS_SUM_PEAK_H_IN,  FS_SUM_PEAK_H_IN_LEVEL,
       FS_SUM_PEAK_H_OUT, FS_SUM_PEAK_H_OUT_LEVEL,     /* depth, first index of the maximum */
       FS_SUM_MEDIAN_IN_LEVEL, FS_SUM_MEDIAN_OUT_LEVEL,
       FS_SUM_NROWS };
int fs_batch_summarize(fs_batch *b, int32_t first, int32_t n, double *out);
/* np.interp(x=xq, xp=x_series, fp=y_series + y_offset) for every reach, as cases/gerd_roseires/n_calibrate.py:55-67 and the Q= branch
 * of model.run (model.py:105-113) call it: outside the range the end values, inside it the largest j with xp[j] <= x and
 * fp[j] + (x - xp[j]) (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]).  x_row, y_row: 0..3 = h[0], Q[0], h[N-1], Q[N-1].  y_offset: [B] or NULL
 * (bed level -> stage).  xq[n_q], 1 <= n_q <= 65535, shared by the batch.  values: [n_q][B] or NULL.  rmse: [B] or NULL,
 * sqrt(mean((values - target)^2)), needs target[n_q].  info: [B] or NULL, bit 0 = x descends somewhere in the range: np.interp is
 * defined for nondecreasing xp only, the values of such a reach are those of a plain bisection and promise nothing against numpy.  A
 * reach that completed no row of the range reports NaN.  At least one of values, rmse, info must be given. */
int fs_batch_lookup(fs_batch *b, int32_t first, int32_t n, int32_t x_row, int32_t y_row, const double *y_offset,
                    const double *xq, int32_t n_q, const double *target, double *values, double *rmse, int32_t *info);
/* Across the members, per level and signal (np.min / max / mean / std / quantile over the members of fs_batch_get_hydrographs' rows):
 * moments[n][4][4] = min, max, mean, std (ddof = 0; two passes) or NULL; quantiles[n][4][n_q] or NULL: the exact order statistics at
 * the levels q[n_q] in [0, 1], 0 <= n_q <= 16, with numpy's default method "linear" (virtual index (m - 1) q, interpolated between its
 * two neighbours); n_members[n] or NULL: the members that entered each level.  Failed members are left out of every level; a level of
 * which no member remains reports 0 members and NaN.  At least one output must be given. */
int fs_batch_bands(fs_batch *b, int32_t first, int32_t n, const double *q, int32_t n_q, double *moments, double *quantiles,
                   int32_t *n_members);

/* ---- Flood envelopes along the reach ----
 * fs_batch_envelope: for the levels [first, first + n) of the stored history (FS_FLAG_HISTORY), for every (reach, node), in one pass
 * over the levels: the extremes of the quantities of the bit mask `quantities` and the levels at which they occur,
 * out[n_selected][FS_ENV_NSTAT][B][N] with the selected quantities in bit order.  Each quantity is evaluated as fs_batch_derive
 * evaluates it (depth, stage = depth + bed, flow, velocity Q/A, Froude number with its clamps, top width), in the batch dtype, and
 * widened to double on output.  Levels are relative to `first`, as doubles, and are first indices (np.argmax / np.argmin); a NaN sample
 * behaves as in numpy: the extreme is NaN and its level is the first NaN's.
 * Crossings (threshold != NULL): crossing[FS_ENV_NCROSS][B][N] = the first level at which the quantity threshold_quantity (one FS_ENV_*
 * bit, selected or not; typical: stage against a bank or levee crest) is >= the threshold (-1: never), the last such level (-1) and
 * their number.  threshold[N] is shared, or [B][N] with threshold_per_reach != 0; it is rounded once to the batch dtype, in which the
 * comparison runs.  A NaN entry means "not assessed": -1, -1, 0.
 * A reach whose status is a failure enters with the rows before its failing level only (see above); levels[B] (or NULL) receives the
 * rows that entered.  A reach without rows reports NaN extremes, levels -1 and counts 0; nodes beyond a ragged reach's own count
 * (fs_batch_set_reach_nodes) report values 0, levels -1 and counts 0.  After fs_batch_restart, ranges that begin before the restart
 * level are refused.  out, crossing and levels may each be NULL (crossing must be NULL without a threshold).  The results stay on the
 * handle, in buffers that are kept and reused, for fs_batch_profile_bands; until the next fs_batch_step, fs_batch_last_step_ms reports
 * the HIP-event time of the kernel. */
enum { FS_ENV_DEPTH = 1, FS_ENV_STAGE = 2, FS_ENV_FLOW = 4, FS_ENV_VELOCITY = 8, FS_ENV_FROUDE = 16, FS_ENV_TOP_WIDTH = 32,
       FS_ENV_ALL = 63,
       FS_ENV_CROSSING = 64 };       /* fs_batch_profile_bands: a crossing row instead of a (quantity, statistic) pair */
enum { FS_ENV_MAX = 0, FS_ENV_MAX_LEVEL, FS_ENV_MIN, FS_ENV_MIN_LEVEL, FS_ENV_NSTAT };
enum { FS_ENV_CROSS_FIRST = 0, FS_ENV_CROSS_LAST, FS_ENV_CROSS_COUNT, FS_ENV_NCROSS };
int fs_batch_envelope(fs_batch *b, int32_t first, int32_t n, int32_t quantities, const double *threshold,
                      int32_t threshold_per_reach, int32_t threshold_quantity, double *out, double *crossing, int32_t *levels);
/* The same kernel with everything left on the device (no PCIe traffic but the threshold).  fs_batch_envelope_device_ptr(row) then
 * points at row `row` of the last envelope, [B][N] doubles: rows 0 .. n_selected * FS_ENV_NSTAT - 1 are out's, the FS_ENV_NCROSS
 * rows behind them the crossings (where a threshold was given); NULL for any other row.  Valid until the next envelope call. */
int fs_batch_envelope_device(fs_batch *b, int32_t first, int32_t n, int32_t quantities, const double *threshold,
                             int32_t threshold_per_reach, int32_t threshold_quantity);
void *fs_batch_envelope_device_ptr(fs_batch *b, int32_t row);
/* Across the members, per node, of one row of the envelope the handle holds: quantity = one FS_ENV_* bit that the envelope selected
 * and stat = FS_ENV_MAX .. FS_ENV_MIN_LEVEL, or quantity = FS_ENV_CROSSING and stat = FS_ENV_CROSS_FIRST .. FS_ENV_CROSS_COUNT.
 * moments[N][4] = min, max, mean, std (ddof = 0; two passes) or NULL; quantiles[N][n_q] or NULL: exact order statistics at the levels
 * q[n_q] in [0, 1], 0 <= n_q <= 16, numpy's method "linear" (as fs_batch_bands); exceed[N] or NULL: the fraction of the entering
 * members whose crossing count is > 0 (needs an envelope computed with a threshold); n_members[N] or NULL.  Left out: failed members,
 * members without rows and, at a given node, the members of a ragged batch that do not have that node - n_members varies along the
 * reach.  A node with no member left reports 0 members and NaN.  Fails when the handle holds no envelope or the row was not computed.
 * At least one output must be given. */
int fs_batch_profile_bands(fs_batch *b, int32_t quantity, int32_t stat, const double *q, int32_t n_q, double *moments,
                           double *quantiles, double *exceed, int32_t *n_members);

/* ---- Reach storage and the discrete water balance ----
 * The handle owns a block integ[max_levels][FS_INT_NROWS][B] of doubles, member minor as the hydrograph block, allocated by the first
 * call below.  A row that was never evaluated is NaN; fs_batch_set_state*, fs_batch_init_state and fs_batch_restart reset every row.
 *
 * fs_batch_reach_integrals: fills the rows first .. first + n - 1 from the stored depth history (FS_FLAG_HISTORY; the flow history is
 * not read).  first = -1 (n = 1) evaluates the CURRENT state into the row of the batch's current level instead and needs no history:
 * a batch that keeps none marks its state now and then, between two fs_batch_step calls.  Per (level, reach), with the trapezoid
 * weights w_i = 1/2 at node 0 and at the reach's own last node (fs_batch_set_reach_nodes), 1 between:
 *   FS_INT_VOLUME       dx_r sum_i w_i A_i          m^3 in the channel
 *   FS_INT_SURFACE      dx_r sum_i w_i T_i          m^2 of water surface
 *   FS_INT_LENGTH_OVER  dx_r sum_i w_i [h_i + z_i >= threshold_i]   metres of reach at or above a stage threshold; NaN without one
 *   FS_INT_BALANCE      NaN until fs_batch_water_balance writes it
 * A_i and T_i are evaluated in the batch dtype as fs_batch_derive evaluates them; products with the weights and sums are fp64 and dx_r
 * is the caller's double (fs_batch_set_reach_scheme's where given), not its rounding to the batch dtype.  threshold[N] is shared, or
 * [B][N] with threshold_per_reach != 0, rounded once to the batch dtype; a NaN entry means "not assessed" and adds nothing.  A row's
 * value depends on the row alone: the same bits whatever B, the reach's place in the batch, the range asked for and the source
 * (history row or current state).  The rows of a failed reach from its failing level on are NaN.  The call is stream-ordered and does
 * not wait for the device, except to upload a threshold (or the scheme, after it changed). */
enum { FS_INT_VOLUME = 0, FS_INT_SURFACE, FS_INT_LENGTH_OVER, FS_INT_BALANCE, FS_INT_NROWS };
int fs_batch_reach_integrals(fs_batch *b, int32_t first, int32_t n, const double *threshold, int32_t threshold_per_reach);
/* fs_batch_water_balance: per reach, over the levels [first, first + n), from each evaluated row to the next evaluated row (a span:
 * one level where every row was evaluated, a chunk of levels for a batch that was marked now and then), FS_INT_BALANCE of the span's
 * end row = (V_end - V_begin) - sum over the span's levels l of dt_r [theta_r (Q_0 - Q_last)_l + (1 - theta_r) (Q_0 - Q_last)_{l-1}]
 * with the boundary flows of the hydrograph block and the caller's fp64 theta_r, dt_r; the first evaluated row of the range gets 0.
 * The Preissmann continuity row is conservative, so a span's residual is dt dx times the summed continuity residuals of its levels:
 * bounded by the Newton tolerance.  totals[FS_BAL_NROWS][B] or NULL: spans, first and last evaluated level (relative to `first`, -1:
 * none), storage change, net inflow volume, inflow volume, summed residual, largest |residual| and the level of its span's end,
 * summed residual over inflow volume.  A failed reach enters with the rows before its failing level. */
enum { FS_BAL_SPANS = 0, FS_BAL_FIRST_LEVEL, FS_BAL_LAST_LEVEL, FS_BAL_STORAGE_CHANGE, FS_BAL_NET_INFLOW, FS_BAL_INFLOW,
       FS_BAL_RESIDUAL, FS_BAL_WORST, FS_BAL_WORST_LEVEL, FS_BAL_RELATIVE, FS_BAL_NROWS };
int fs_batch_water_balance(fs_batch *b, int32_t first, int32_t n, double *totals);
/* out[n][FS_INT_NROWS][B]: the rows first .. first + n - 1 of the block (any rows of 0 .. max_levels - 1), and the block on the
 * device, [max_levels][FS_INT_NROWS][B] doubles (NULL before the first evaluation) */
int fs_batch_get_reach_integrals(fs_batch *b, int32_t first, int32_t n, double *out);
void *fs_batch_reach_integrals_device_ptr(fs_batch *b);
/* fs_batch_bands on the integral block instead of the hydrograph block (the same kernel): moments[n][FS_INT_NROWS][4],
 * quantiles[n][FS_INT_NROWS][n_q], n_members[n].  Failed members are left out; a level that one of the remaining members has not
 * evaluated reports NaN, as numpy would. */
int fs_batch_integral_bands(fs_batch *b, int32_t first, int32_t n, const double *q, int32_t n_q, double *moments, double *quantiles,
                            int32_t *n_members);

/* ---- Interior gauges: station series, their bands across the members and fit scores ----
 * A gauge sits between node `node` and node + 1 of a reach, at weight in [0, 1) of the way: fs_batch_set_gauges takes node[G] and
 * weight[G] shared by the batch, or [B][G] with per_reach != 0 (ragged batches, per-reach dx), 0 <= G <= FS_GAUGE_MAX.  It checks
 * what the host can know - 0 <= node < n_nodes, weights finite and in [0, 1), node + 1 < n_nodes where the weight is not 0 - then
 * allocates the block gauge[G][max_levels][FS_GAUGE_NROWS][B] of doubles (gauge g's part has the shape of the hydrograph block,
 * member minor) and the marks [max_levels][B], one int32 per (level, member) whose bit g says that gauge g's row holds values, and
 * sets every row to NaN and every mark to 0.  G = 0 frees both.  fs_batch_set_state*, fs_batch_init_state and fs_batch_restart
 * reset every row and mark in the same way.
 *
 * fs_batch_gauges: fills the rows first .. first + n - 1 of every gauge from the stored history (FS_FLAG_HISTORY; ranges as
 * fs_batch_reach_integrals).  first = -1 (n = 1) fills the row of the batch's current level from the current state instead and needs
 * no history: a batch that keeps none marks its state between two fs_batch_step calls (refused while a level opened by
 * fs_batch_iterate is open).  Per (level, member, gauge) the four quantities are evaluated at node and, where the weight is not 0, at
 * node + 1 as fs_batch_derive evaluates them - depth h, flow Q, stage h + z, velocity Q / A - in the batch dtype, widened to double,
 * and the row is a + weight (b - a) in fp64, the product rounded before the sum.  With weight 0 the row is a itself and node + 1 is
 * not read: a gauge may sit on a reach's last node.  NaN rows with mark bit 0: those of a failed reach from its failing level on, and
 * at every level those of a reach that does not have the gauge (node, or node + 1 with a weight that is not 0, at or beyond its own
 * node count, fs_batch_set_reach_nodes).  A row's bits depend on (level, member, gauge) alone: not on B, on the member's place in the
 * batch, on the range asked for, or on the source (history row or current state).  The call is stream-ordered, does not wait for the
 * device, and fs_batch_last_step_ms then reports its kernel.
 *
 * fs_batch_get_gauges: out[n][FS_GAUGE_NROWS][B], the rows first .. first + n - 1 (any rows of 0 .. max_levels - 1) of one gauge;
 * fs_batch_gauges_device_ptr: its [max_levels][FS_GAUGE_NROWS][B] doubles on the device (NULL: no such gauge).
 * fs_batch_gauge_bands: fs_batch_bands on one gauge's block (the same kernel): moments[n][4][4], quantiles[n][4][n_q], n_members[n].
 * Failed members and members that do not have the gauge are left out; a level that a remaining member has not evaluated reports NaN.
 * fs_batch_gauge_lookup: fs_batch_lookup on one gauge's block (the same kernels), x_row and y_row being FS_GAUGE_*; a range in which
 * some level was never evaluated is refused.
 * fs_batch_gauge_score: per member, one signal (FS_GAUGE_*) of one gauge against observed[n], or [n][B] with observed_per_reach != 0;
 * a NaN in observed means "no observation".  A level counts when it is inside the member's completed rows, marked and observed.  Over
 * the m counted levels, in level order and in fp64 with every product rounded: out[FS_GS_NROWS][B] = m; sum(sim - obs) / m;
 * sqrt(sum((sim - obs)^2) / m); 1 - sum((sim - obs)^2) / sum((obs - mean(obs))^2) (whatever IEEE gives for a zero denominator); the
 * simulated peak and its level (first index of the maximum, relative to `first`); simulated minus observed peak; simulated minus
 * observed peak level.  m = 0: count 0, levels -1, the rest NaN.  A NaN simulated value at a counted level propagates as in numpy. */
enum { FS_GAUGE_DEPTH = 0, FS_GAUGE_FLOW, FS_GAUGE_STAGE, FS_GAUGE_VELOCITY, FS_GAUGE_NROWS };
#define FS_GAUGE_MAX 32
enum { FS_GS_COUNT = 0, FS_GS_BIAS, FS_GS_RMSE, FS_GS_NSE, FS_GS_PEAK_SIM, FS_GS_PEAK_SIM_LEVEL, FS_GS_PEAK_ERROR, FS_GS_PEAK_LAG,
       FS_GS_NROWS };
int fs_batch_set_gauges(fs_batch *b, int32_t n_gauges, const int32_t *node, const double *weight, int32_t per_reach);
int fs_batch_gauges(fs_batch *b, int32_t first, int32_t n);
int fs_batch_get_gauges(fs_batch *b, int32_t gauge, int32_t first, int32_t n, double *out);
void *fs_batch_gauges_device_ptr(fs_batch *b, int32_t gauge);
int fs_batch_gauge_bands(fs_batch *b, int32_t gauge, int32_t first, int32_t n, const double *q, int32_t n_q, double *moments,
                         double *quantiles, int32_t *n_members);
int fs_batch_gauge_lookup(fs_batch *b, int32_t gauge, int32_t first, int32_t n, int32_t x_row, int32_t y_row, const double *y_offset,
                          const double *xq, int32_t n_q, const double *target, double *values, double *rmse, int32_t *info);
int fs_batch_gauge_score(fs_batch *b, int32_t gauge, int32_t signal, int32_t first, int32_t n, const double *observed,
                         int32_t observed_per_reach, double *out);

/* ---- Assimilation of gauge observations: the analysis step of a stochastic ensemble Kalman filter over the members ----
 * fs_batch_assimilate corrects the state of every member that takes part, between two fs_batch_step calls, from n_obs observations
 * (1 .. FS_ASSIM_MAX_OBS): observation j is signal[j] (FS_GAUGE_*) of gauge[j] (of fs_batch_set_gauges, shared positions), observed as
 * value[j] with error variance[j] (finite, > 0).  perturb [n_obs][B] (or NULL: zeros) is what the caller adds to the observation per
 * member - the library draws no random numbers -, taper [n_obs][N] in [0, 1] (or NULL: ones) localises observation j along the reach.
 * The members must be one channel, node for node: per-reach gauges (per_reach != 0) and per-reach node counts are refused.
 *
 * Refused with a text that names fs_batch_assimilate, and with the state untouched bit for bit: no state, no geometry, no gauges;
 * per-reach gauges or node counts; a level opened by fs_batch_iterate; n_obs outside 1 .. FS_ASSIM_MAX_OBS; a gauge or signal out of
 * range; a variance that is not finite or not > 0; a value, perturbation or taper that is not finite, a taper outside [0, 1];
 * depth_floor negative or not finite; fewer than two active members; an active member with a NaN in an observed signal; an innovation
 * covariance whose Cholesky factor has a pivot that is not positive and finite.
 *
 * Gather and active members.  The call first fills the gauge row of the current level from the current state, exactly as
 * fs_batch_gauges(b, -1, 1) does (that row stays, also after a refusal).  Member r is ACTIVE when its mark at that level has the bit
 * of every observed gauge: failed members are inactive, and an inactive member is never written.  n_a: the active members; y_jr: the
 * gathered value of observation j in member r.
 *
 * Host part, in fp64, sequentially in member order over the active members, every product rounded (no contraction):
 *   ybar_j = sum_r y_jr / n_a;   S_jr = y_jr - ybar_j (0 for inactive members);
 *   C_jl = (sum_r S_jr S_lr) / (n_a - 1) + [j == l] variance_j;   C = L D L^T, the square-root-free lower Cholesky factor row by
 *   row (L unit lower, D the pivots: L_jl = (C_jl - sum_{k<l} (L_jk D_k) L_lk) / D_l, D_j = C_jj - sum_{k<j} (L_jk D_k) L_jk, the sums
 *   subtracted in ascending k).  The pivots are the squares of the pivots of C = G G^T; without the root, one observation is
 *   Z = D / C in a single rounding;
 *   D_jr = (value_j + perturb_jr) - y_jr;   Z_.r = C^-1 D_.r: w_j = D_jr - sum_{k<j} L_jk w_k, then from j = n_obs - 1 down
 *   z_j = w_j / D_j - sum_{k>j} L_kj z_k, the inner sums subtracted in ascending k (0 for inactive members).
 * Moments, per field f in {h, Q} and node i, in fp64: c = the value of the first active member.  The members are taken in chunks of
 * FS_ASSIM_CHUNK by batch index; within a chunk the active members sequentially in member order: d = x_r - c; s1 += d; s2 += d d;
 * p_j += d S_jr, every product rounded, every sum from 0.0.  The chunk partials are added in chunk order, beginning with chunk 0's.
 *   mean = c + s1 / n_a;   var = (s2 - (s1 s1) / n_a) / (n_a - 1);   P_fji = p_j / (n_a - 1).
 * (Subtracting c is exact algebra, since sum_r S_jr = 0; it keeps the sums conditioned on stages of hundreds of metres.)
 * Update, for active members only: inc = sum_j (taper_ji P_fji) Z_jr in j order from 0.0, each product rounded (taper NULL: P_fji
 * itself).  hk <- R(double(hk) + inc) and hg <- R(double(hg) + inc), R rounding to the batch dtype: the Newton start vector takes
 * the same increment; Qk and Qg likewise.  A new depth hk below depth_floor, or NaN, becomes depth_floor in both hk and hg at that
 * node (so does a new hg that is below the floor or NaN on its own); clamped[r] counts the nodes of hk where that happened.
 * Inactive members keep every bit.
 *
 * Outputs, each optional: prior [4][N] = mean h, var h, mean Q, var Q of the active members before the update; cross_cov
 * [2][n_obs][N] = P, before the taper; clamped [B]; *n_active (also set when the call is refused for too few active members, a NaN
 * or a pivot).
 *
 * What is left alone: the history, hydrograph and storage-stage blocks, the reservoir state, the level counter and the status.  They
 * record the forecast; the analysis acts on what is stepped next (every launch rebuilds its level constants from hk / Qk).  The
 * discrete water balance across an analysis level therefore no longer closes: the analysis adds or removes water.
 * fs_batch_last_step_ms then reports the moments, combine and update kernels (three launches); the call waits for the device. */
#define FS_ASSIM_MAX_OBS 16
#define FS_ASSIM_CHUNK   256      /* members per partial sum: part of the contract, the bits depend on it */
int fs_batch_assimilate(fs_batch *b, int32_t n_obs, const int32_t *gauge, const int32_t *signal, const double *value,
                        const double *variance, const double *perturb, const double *taper, double depth_floor, double *prior,
                        double *cross_cov, int32_t *clamped, int32_t *n_active);

/* zero-copy access for device-side consumers (RCCL gather of hydrographs): device pointer to the
 * [max_levels][4][B] hydrograph block in the batch dtype, and the handle's hipStream_t */
void *fs_batch_hydrograph_device_ptr(fs_batch *b);
void *fs_batch_stream(fs_batch *b);

/* measurement: HIP-event time of the kernels launched by the last fs_batch_step (ms, after
 * fs_batch_sync), their count, and the launch geometry chosen for this batch */
double fs_batch_last_step_ms(fs_batch *b);
int32_t fs_batch_last_launch_count(fs_batch *b);
int fs_batch_kernel_info(fs_batch *b, int32_t *cells_per_thread, int32_t *waves_per_reach,
                         int32_t *lds_bytes, int32_t *vgprs);
/* The dispatch table of the step kernel (what fs_batch_step chooses from): fs_kernel_table_size() entries,
 * entry i described by out[8] = dtype, section_mode, cells per lane M, waves per reach W, full (1: only N == 64*W*M),
 * boundary class (-1 any kind, 0 any but FS_BC_STORAGE_CURVE / FS_BC_HOST_ROW, 1 closed-form rectangular rows, 2+k flow
 * hydrograph upstream and kind k downstream), diag (0: no history / trace stores), long (1: the multi-pass kernel for reaches
 * longer than one lane grid).  The fields in full, and how an entry is chosen: fs::KernelKey and fs::pick in
 * flow-sim_amd/csrc/fs_dispatch.hpp.  The environment
 * variable FS_KERNEL_INDEX=i makes fs_batch_step use entry i or fail if it does not fit the batch (tests:
 * every instantiation is checked against the oracle). fs_batch_kernel_index: the entry the last step used. */
int32_t fs_kernel_table_size(void);
int fs_kernel_table_entry(int32_t i, int32_t *out);
int32_t fs_batch_kernel_index(fs_batch *b);
/* entry i in its tail-only form (round 4: ragged, but compiled for the local row the downstream boundary row takes in its lane):
 * that row, (N - 1) mod M, or -1 for every other entry (-2: no such entry).  fs_batch_step only picks such an entry for a batch
 * whose one node count gives that row. */
int32_t fs_kernel_table_entry_tail(int32_t i);
/* 1: entry i advances a reach LONGER than one lane grid as a team of ceil(N / (64 W M)) workgroups that each keep 64 W M rows on chip and
 * meet once per Newton iteration through device memory (uniform section modes, 4 097 ... 32 768 nodes; round 4) - fs_batch_step prefers it
 * to the multi-pass entries (long = 1), which remain for tables, polylines, host rows and FS_NO_TEAM=1; 0 otherwise (-2: no such entry). */
int32_t fs_kernel_table_entry_team(int32_t i);
/* FS_SEC_IRREGULAR: 1 when the batch evaluates its polylines from stage tables, 0 when it walks their edges (the same results at
 * about five times the instructions): the tables take about 10 KB per node at 40 stations, per channel, and
 * fs_batch_set_geometry_irregular(_per_reach) leaves them out beyond FS_POLY_TABLE_MAX_BYTES (environment, default 8 GiB) or with
 * FS_POLY_WALK=1.  The reference evaluates every call by walking the polyline (cross_section.py:248-538). -1: no polylines set. */
int32_t fs_batch_poly_tables(fs_batch *b);

#ifdef __cplusplus
}
#endif
#endif /* FLOWSIM_ABI_H */
