/*
 * dab.h — C ABI of the MI355X bundle-adjustment solver ("dab" = DeepArc BA).
 *
 * This is the drop-in boundary that replaces the Ceres modelling/solve calls made
 * by the reference's BA driver:
 *
 *   reference (pureexe/deeparc-sfm)                     replaced by
 *   ------------------------------------------------    ------------------------------
 *   SnavelyReprojectionError::Create + AddResidualBlock  dab_problem (SoA observation
 *     src/sfm.cc:36-48, snavely_reprojection_error.hh    arrays + gather indices)
 *     :121-141, ParameterBlock::get() ParameterBlock.hh
 *     :68-94
 *   Problem::SetParameterBlockConstant  sfm.cc:50-63     dab_problem.ext_const /
 *                                                         dab_problem.freeze_camera
 *   ceres::Solver::Options  sfm.cc:66-71                 dab_options (+ dab_options_init)
 *   ceres::Solve + Summary::FullReport  sfm.cc:72-74     dab_solve + dab_summary
 *   SnavelyReprojectionError::operator()(double)         dab_eval_residuals
 *     DeepArcManager.cc:335-346 (filterPoint3d)
 *   DeepArcManager::filterPoint3d DeepArcManager.cc:     dab_filter (device residuals +
 *     332-424                                              drop masks)
 *   DynamicAutoDiffCostFunction::Evaluate (jacobians)    dab_eval_jacobians
 *     snavely_reprojection_error.hh:11-14
 *
 * Conventions: plain pointers and sizes only. The caller owns every host array. The
 * library copies the problem to the device in dab_set_problem, runs every iteration
 * device-resident, and writes the optimised `points` / `ext` back into the caller's
 * arrays when dab_solve returns (the reference's Ceres writes into the user's double*
 * blocks in place, sfm.cc:47-48). Every entry point returns 0 on success and a negative
 * DAB_E* code on error; dab_last_error() gives the message. Nothing aborts.
 * A handle is used by one host thread at a time (not re-entrant per handle).
 */
#ifndef DAB_H_
#define DAB_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAB_ABI_VERSION 2

/* ---- status codes ---------------------------------------------------------------- */
#define DAB_OK 0
#define DAB_E_INVALID (-1)   /* bad argument / malformed problem */
#define DAB_E_DEVICE (-2)    /* HIP runtime error or no device */
#define DAB_E_NOMEM (-3)     /* device allocation failed */
#define DAB_E_STATE (-4)     /* call out of order (e.g. solve before set_problem) */
#define DAB_E_COMM (-5)      /* RCCL error */
#define DAB_E_UNSUPPORTED (-6)

/* ---- problem ----------------------------------------------------------------------
 * One residual block per observation (sfm.cc:36-48). Residual (snavely…hh:94-118):
 *   single extrinsic (ext1 < 0):   P = R(w0) X + t0
 *   composed arc∘ring (ext1 >= 0): P = R(w0) (R(w1) X + t1) + t0
 *      (ext0 = the arc extrinsic, ext1 = the ring extrinsic, snavely…hh:96-108,
 *       ParameterBlock.hh:83-87)
 *   xp = P0/P2, yp = P1/P2; d = 1 | 1+k0 r2 | 1+r2(k0+k1 r2)   (nk = 0|1|2)
 *   r = (f0 d xp + cx - x_obs,  f1' d yp + cy - y_obs),  f1' = nf==2 ? f1 : f0
 * Extrinsic layout: ext[e] = (w0,w1,w2, t0,t1,t2) — angle-axis rotation then
 * translation (the two 3-blocks of Extrinsic.hh:32).
 * Intrinsic layout: intr[i] = (cx, cy, f0, f1, k0, k1) with intr_nf[i] in {1,2},
 * intr_nk[i] in {0,1,2} (Intrinsic.hh:32; unused slots ignored).
 * Intrinsics are constant by default, as in the reference (sfm.cc:54-63);
 * dab_set_intrinsics_free frees them by group for the exact step.
 * Constancy: points are free unless dab_set_points_constant holds them (sfm.cc:59); an
 * extrinsic is free unless ext_const[e] != 0 or freeze_camera != 0 (sfm.cc:50-57). Parameter
 * blocks referenced by no observation are not part of the problem (Ceres only knows blocks
 * added via AddResidualBlock) and are left untouched.
 */
typedef struct dab_problem {
  int32_t num_obs;
  int32_t num_points;
  int32_t num_ext;
  int32_t num_intr;
  const double* obs_xy;      /* [num_obs][2] observed pixel (Point2d, Point2d.hh:12) */
  const int32_t* obs_point;  /* [num_obs] point index */
  const int32_t* obs_ext0;   /* [num_obs] extrinsic (arc when composed) */
  const int32_t* obs_ext1;   /* [num_obs] ring extrinsic when composed, else -1 */
  const int32_t* obs_intr;   /* [num_obs] intrinsic index */
  double* points;            /* [num_points][3] in/out */
  double* ext;               /* [num_ext][6] in/out */
  const double* intr;        /* [num_intr][6] */
  const int32_t* intr_nf;    /* [num_intr] */
  const int32_t* intr_nk;    /* [num_intr] */
  const uint8_t* ext_const;  /* [num_ext] or NULL */
  int32_t freeze_camera;     /* solve(..., freeze_camera=true), sfm.cc:54-57 */
  int32_t reserved;
} dab_problem;

/* ---- options (mirrors the ceres::Solver::Options fields the reference uses plus the
 * Ceres trust-region defaults it relies on implicitly) ------------- */
#define DAB_LINEAR_SOLVER_EXPLICIT_SCHUR 0  /* exact: DENSE_SCHUR equivalent (sfm.cc:67) */
#define DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG 1 /* inexact: ITERATIVE_SCHUR + SCHUR_JACOBI */
/* the exact step where it scales over the ranks, PCG where it does not: EXPLICIT_SCHUR on
 * one rank and, on several, for small camera systems (<= 160 free cameras: the rig; S is a
 * few MB to all-reduce and its factorisation takes microseconds); IMPLICIT_SCHUR_PCG for
 * large camera systems on several ranks (BASELINE config 4: the 288-MB S all-reduce and the
 * serial 5.5-ms factorisation on every rank would cap the speed-up near 1.2x). The summary's
 * linear_solver_type_used says which ran. */
#define DAB_LINEAR_SOLVER_AUTO 2

typedef struct dab_options {
  int32_t max_num_iterations;            /* sfm.cc:69 (call sites pass 100) */
  int32_t linear_solver_type;            /* DAB_LINEAR_SOLVER_* */
  double max_solver_time_in_seconds;     /* sfm.cc:71 */
  double function_tolerance;             /* 1e-6 */
  double gradient_tolerance;             /* 1e-10 */
  double parameter_tolerance;            /* 1e-8 */
  double min_relative_decrease;          /* 1e-3 */
  double initial_trust_region_radius;    /* 1e4 */
  double max_trust_region_radius;        /* 1e16 */
  double min_trust_region_radius;        /* 1e-32 */
  double min_lm_diagonal;                /* 1e-6 */
  double max_lm_diagonal;                /* 1e32 */
  int32_t max_num_consecutive_invalid_steps; /* 5 */
  int32_t jacobi_scaling;                /* 1 */
  int32_t minimizer_progress_to_stdout;  /* sfm.cc:68 */
  int32_t num_threads;                   /* CPU paths only (sfm.cc:70) */
  /* PCG (IMPLICIT_SCHUR_PCG only) — Ceres ITERATIVE_SCHUR defaults */
  int32_t max_linear_solver_iterations;  /* 500 */
  int32_t min_linear_solver_iterations;  /* 0 */
  double eta;                            /* 1e-1 (Nash–Sofer q-tolerance) */
  int32_t pcg_fp32;                      /* 1: fp32 matvec/preconditioner, fp64 accumulate */
  int32_t reserved;
} dab_options;

/* ---- summary (ceres::Solver::Summary subset, sfm.cc:72-74) ------------------------ */
#define DAB_CONVERGENCE 0
#define DAB_NO_CONVERGENCE 1
#define DAB_FAILURE 2

typedef struct dab_iteration {
  int32_t iteration;
  int32_t step_is_successful;
  int32_t step_is_valid;
  int32_t linear_solver_iterations;
  double cost;
  double cost_change;
  double gradient_max_norm;
  double step_norm;
  double relative_decrease;
  double trust_region_radius;
  double iteration_time_in_seconds;
} dab_iteration;

typedef struct dab_summary {
  double initial_cost;
  double final_cost;
  int32_t num_iterations;          /* index of the last iteration record */
  int32_t num_successful_steps;    /* iteration 0 counts, as in Ceres */
  int32_t num_unsuccessful_steps;
  int32_t termination_type;        /* DAB_CONVERGENCE / NO_CONVERGENCE / FAILURE */
  int32_t num_residuals;
  int32_t num_parameters;          /* free scalar parameters */
  int32_t num_free_points;
  int32_t num_free_ext;
  double total_time_in_seconds;
  double jacobian_evaluation_time_in_seconds;
  double residual_evaluation_time_in_seconds;
  double linear_solver_time_in_seconds;
  char message[256];
  dab_iteration* iterations;       /* optional caller buffer (may be NULL) */
  int32_t iterations_capacity;     /* entries available in `iterations` */
  int32_t iterations_written;      /* entries filled */
  int32_t linear_solver_type_used; /* the DAB_LINEAR_SOLVER_* that ran (the requested one, or
                                      what DAB_LINEAR_SOLVER_AUTO chose) */
  int32_t schur_assembly;          /* EXPLICIT_SCHUR: DAB_SCHUR_* (how S was assembled);
                                      IMPLICIT_SCHUR_PCG: DAB_PCG_* (the Schur products) */
} dab_summary;
/* schur_assembly values for DAB_LINEAR_SOLVER_EXPLICIT_SCHUR */
#define DAB_SCHUR_PAIRS 0   /* per camera-pair block sums over entry-pair tables (large NC) */
#define DAB_SCHUR_TILES 1   /* register-owned block tiles over per-step Y records (NC <= 160) */
#define DAB_SCHUR_DIRECT 2  /* no free point on any rank: S = U + D^2, no Schur complement */
/* schur_assembly values for DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG */
#define DAB_PCG_STORED_Y 0          /* products over stored Y records (fp32 records with pcg_fp32) */
#define DAB_PCG_MATRIX_FREE 1       /* rows re-evaluated per product, all fp64 (NC <= 160) */
#define DAB_PCG_MATRIX_FREE_FP32 2  /* as 1 with pcg_fp32: fp32 per-observation arithmetic, fp64
                                       sums, fp64 CG recurrences and true residuals */

typedef struct dab_handle dab_handle;

/* ---- lifecycle ---------------------------------------------------------------------- */
int dab_abi_version(void);
const char* dab_last_error(void);
void dab_options_init(dab_options* opt);

/* device: HIP ordinal. Single-process handle (world_size 1).
   Side effect, process-wide: every dab_create* sets hipSetDeviceFlags(hipDeviceScheduleSpin)
   (the LM loop's host round trips are latency-critical), so every host wait of the
   embedding process spins instead of blocking. DAB_SCHEDULE_BLOCKING=1 in the environment
   keeps the runtime's default; a refused flag is reported once on stderr. */
int dab_create(int device, dab_handle** out);
/* Multi-GPU (one process per GPU, RCCL over xGMI). `unique_id` is the 128-byte
 * ncclUniqueId produced on rank 0 by dab_comm_unique_id and broadcast by the caller.
 * world_size 1 with a non-null unique_id builds a one-rank RCCL communicator and runs
 * the solve's collectives through it — the evaluation pass's (the split schedule with its
 * camera all-reduce on the communication stream included), the LM step's and every PCG
 * iteration's: the same results as dab_create, with the multi-GPU transport executed on one
 * GPU. The set-up's free-camera and pair-set unions, the LINEAR_SOLVER_AUTO choice and the
 * rig's matrix-free PCG product (whose work-group partials a single rank sums inside the CG
 * update, no all-reduce) follow world_size, so they take the one-rank paths. */
int dab_comm_unique_id(uint8_t out_id[128]);
int dab_create_dist(int device, int rank, int world_size, const uint8_t unique_id[128],
                    dab_handle** out);
/* Host-staged collective, for rehearsing the multi-rank path where RCCL cannot run
 * (several ranks sharing one GPU; CI). Every all-reduce copies the device buffer to
 * host memory and calls cb(buf, count, op, user), which must reduce it in place across
 * the ranks (op 0 = sum, 1 = max; e.g. over gloo) and return 0. Not the product path:
 * one process per GPU uses dab_create_dist (RCCL over xGMI). */
typedef int (*dab_host_allreduce_fn)(double* buf, int64_t count, int op, void* user);
int dab_create_dist_host(int device, int rank, int world_size, dab_host_allreduce_fn cb, void* user,
                         dab_handle** out);
/* Frees the handle's device buffers. Its streams and small pinned host blocks go to a
 * process-wide cache that the next dab_create on the same device takes from (creating and
 * destroying a stream cost ~2 ms each); a cached stream that reports an error is destroyed
 * instead of reused. */
int dab_destroy(dab_handle* h);
/* Destroys the cached streams and frees the cached pinned blocks (an embedding process that
 * resets the device, or wants the memory back). Safe with handles alive: it touches only
 * the idle objects in the cache, never a live handle's own streams or pinned blocks (each
 * stream is destroyed with its own device current, the caller's device restored). To get
 * every stream back, destroy the handles first. */
int dab_release_caches(void);

/* ---- problem upload / solve ------------------------------------------------------------
 * dab_set_problem copies the problem to the device and builds the point-major and
 * camera-major orderings once. In a multi-GPU handle each rank passes its own shard
 * (observations of a disjoint point set; extrinsics and intrinsics replicated with
 * identical values on every rank). */
int dab_set_problem(dab_handle* h, const dab_problem* p);
/* Re-upload only the parameter values (points, ext) of the current problem. */
int dab_update_parameters(dab_handle* h, const double* points, const double* ext);
int dab_solve(dab_handle* h, const dab_options* opt, dab_summary* summary);

/* ---- robust loss ------------------------------------------------------------------------
 * The reference adds every residual block with a NULL loss and keeps
 * `//new ceres::CauchyLoss(0.5)` commented out beside it (sfm.cc:48-49); its outer
 * solve -> filterPoint3d -> solve loop stands in for one. Here the loss is state of the
 * handle, one for every observation. Ceres' definitions (an assumption labelled like SURVEY
 * App. B), with s = ru^2 + rv^2 per observation, a = scale, b = a^2, c = 1 / b:
 *   TRIVIAL     rho = s                               rho' = 1
 *   HUBER(a)    s <= b: s, else 2 a sqrt(s) - b       s <= b: 1, else max(DBL_MIN, a / sqrt(s))
 *   SOFT_L1(a)  2 b (sqrt(1 + s c) - 1)               max(DBL_MIN, 1 / sqrt(1 + s c))
 *   CAUCHY(a)   b log(1 + s c)                        max(DBL_MIN, 1 / (1 + s c))
 * All have rho'' <= 0, so Ceres' Corrector scales residual and Jacobian rows by sqrt(rho'(s))
 * at the linearisation point (alpha = 0): gradient, blocks, Jacobi scaling, Schur complement,
 * PCG, back substitution and the model cost change all use the scaled rows. Every cost
 * dab_solve reports (initial, per iteration, final) is 0.5 sum rho(s), not 0.5 |scaled r|^2.
 * dab_eval_residuals, dab_eval_jacobians and dab_filter keep returning the raw residuals,
 * Jacobians and 0.5 sum r^2 (the reference's filter calls the bare functor).
 *
 * The loss defaults to TRIVIAL, survives dab_set_problem and dab_update_parameters, and takes
 * effect at the next dab_solve, dab_bench_eval_pass or dab_bench_get_blocks (under a loss the
 * blocks are those of the scaled rows and *cost = 0.5 sum rho). In a multi-rank handle every
 * rank must set the same loss. DAB_E_INVALID (loss unchanged) for a null handle (checked
 * before any device use), an unknown type, or a scale that is not finite and > 0; the scale
 * is ignored for TRIVIAL. dab_solve with pcg_fp32 != 0 and a non-trivial loss returns
 * DAB_E_UNSUPPORTED: the fp32 matrix-free product never forms a residual to weight. */
#define DAB_LOSS_TRIVIAL 0
#define DAB_LOSS_HUBER   1
#define DAB_LOSS_SOFT_L1 2
#define DAB_LOSS_CAUCHY  3
int dab_set_loss(dab_handle* h, int32_t loss_type, double scale);
int dab_get_loss(dab_handle* h, int32_t* loss_type, double* scale);
/* Copy the device-resident parameters into host arrays (either may be NULL). */
int dab_get_parameters(dab_handle* h, double* points, double* ext);

/* ---- free intrinsics (self-calibration) -------------------------------------------------
 * ParameterBlock::get() hands Ceres the principal point, the focal length and the distortion
 * as parameter blocks [1], [2], [3], and sfm.cc:60-62 freezes them with three
 * SetParameterBlockConstant lines. Deleting those lines is, here, a mask on the handle: one
 * byte of DAB_INTR_* group bits per intrinsic (NULL = all constant, the default).
 *
 * Free set. The mask is state of the handle, set after dab_set_problem; dab_set_problem resets
 * it to all-constant (num_intr may change). It takes effect at the next dab_solve. An intrinsic
 * is free when some observation on some rank references it and its groups select at least one
 * active scalar: CENTER cx, cy; FOCAL f0 (and f1 when nf == 2; with nf == 1 the one focal
 * length drives both fx and fy'); DISTORTION k0 .. k_{nk-1}. Unreferenced intrinsics stay
 * untouched and uncounted, as unreferenced extrinsics do. dab_summary.num_parameters grows by
 * the active scalars. In a multi-rank handle every rank sets the same mask; dab_solve,
 * dab_covariance and dab_bench_eval_pass are collective, and so is the first
 * dab_get_intrinsics_free with a count pointer and a non-empty mask (the referenced union is
 * formed once per problem). On a single-rank handle dab_get_intrinsics_free counts on the host
 * and touches neither the device nor the handle's state.
 * With freeze_camera != 0 the mask is ignored: the handle takes the freeze path unchanged
 * (sfm.cc:54-57 freezes every block but the point). With an empty free set every call gives
 * bitwise what it gives on a handle whose mask was never set.
 *
 * Refined values stay on the handle: dab_problem.intr is const and is never written;
 * dab_get_intrinsics returns them ([num_intr][6], dab_problem layout; slots the model does not
 * have keep the problem's values), dab_update_intrinsics replaces them, and every later call
 * on the handle (residuals, Jacobians, filter, benchmark hooks, covariance) uses them.
 *
 * The step: the exact Schur step with a block z of six slots per free intrinsic bordering the
 * reduced camera system ("Free intrinsics"); Jacobi scaling, LM diagonal, loss
 * scaling, step norms and tolerances extend over the active scalars with the cameras' formulas.
 *
 * dab_eval_intrinsic_jacobians: raw, unscaled d r / d (cx, cy, f0, f1, k0, k1) per observation
 * in the caller's order, [num_obs][2][6] row-major, at the parameters on the handle; columns
 * of scalars the intrinsic's model does not have are zero, and with nf == 1 the f0 column
 * carries both rows. dab_get_intrinsic_blocks: per free intrinsic (ascending index) the sums of
 * the last evaluation that formed them, U_zz upper-packed (21) | g_z (6), over the active
 * columns, in dab_bench_get_blocks' convention (rows scaled by sqrt(rho') under a loss, summed
 * over the ranks). dab_solve forms them at every evaluation, dab_bench_eval_pass (with
 * assembly) when the free set is not empty. Query *num_free_intr with zg NULL first.
 *
 * Refusals, fail closed, state unchanged. dab_solve with a non-empty free set returns
 * DAB_E_UNSUPPORTED for IMPLICIT_SCHUR_PCG (requested or chosen by AUTO), for more than 16 free
 * intrinsics, and for a problem without a free extrinsic (unless freeze_camera is set);
 * dab_covariance with a non-empty free set returns DAB_E_UNSUPPORTED (it would report the
 * intrinsics as exactly known; dab_covariance_intrinsics covers them). DAB_E_INVALID for a null handle (checked before any device
 * use), a null array where one is required, or group bits above 7; DAB_E_STATE before
 * dab_set_problem. */
#define DAB_INTR_CENTER     1   /* cx, cy                      block [1], sfm.cc:60 */
#define DAB_INTR_FOCAL      2   /* f0, and f1 when nf == 2     block [2], sfm.cc:61 */
#define DAB_INTR_DISTORTION 4   /* k0 .. k_{nk-1}              block [3], sfm.cc:62 */
int dab_set_intrinsics_free(dab_handle* h, const uint8_t* groups /* [num_intr], NULL = all constant */);
int dab_get_intrinsics_free(dab_handle* h, uint8_t* groups, int32_t* num_free_intr, int32_t* num_free_scalars);
int dab_get_intrinsics(dab_handle* h, double* intr /* [num_intr][6], dab_problem layout */);
int dab_update_intrinsics(dab_handle* h, const double* intr);
int dab_eval_intrinsic_jacobians(dab_handle* h, double* J /* [num_obs][2][6], caller order */);
int dab_get_intrinsic_blocks(dab_handle* h, int32_t* num_free_intr, double* zg /* [nfi][27] = U_zz upper 21 | g_z 6 */);

/* ---- constant points --------------------------------------------------------------------
 * sfm.cc:59 keeps `//problem.SetParameterBlockConstant(parameter_block[0]); //freeze point3d`
 * commented out beside the three intrinsic freezes. Here it is a mask on the handle, one byte
 * per point in the caller's order (any non-zero byte = constant; NULL = all free, the default):
 * pose-only refinement against a trusted model (all points), ground-control points (a few, which
 * also fix the scale gauge dab_covariance needs), resectioning.
 *
 * The mask is state of the handle, set after dab_set_problem; dab_set_problem resets it to
 * all-free (num_points may change); it survives dab_update_parameters and dab_set_loss and
 * takes effect at the next dab_solve, dab_covariance or dab_covariance_intrinsics. A flagged
 * point that no observation references is ignored, as unreferenced blocks are everywhere else.
 * In a multi-rank handle each rank passes the mask of its own shard (the calls that honour it are
 * collective already). dab_get_points_constant returns the mask as set (zeros when never set)
 * and in *num_constant the points of this rank that are both referenced and constant.
 *
 * A constant point is out of the problem, as in Ceres' reduced program: it is not counted in
 * num_parameters or num_free_points (dab_summary, dab_covariance_info), takes no part in
 * gradient_max_norm, x_norm or step_norm, has no Jacobi scale or LM diagonal of its own; its
 * observations still contribute residuals, cost and camera (and intrinsic) rows in full.
 * dab_solve never writes it: its three doubles in the caller's `points` and in
 * dab_get_parameters are bitwise the input, also after rejected steps. With an empty constant
 * set (never set, NULL, all zero, or only unreferenced points flagged) every call gives bitwise
 * what it gives on a handle that never set a mask.
 *
 * The step. With some points free: the exact or PCG step as before, the constant points' PU and
 * q set to zero ("Constant points"); every linear solver, assembly, loss and
 * free-intrinsics combination that works without a mask works with one. With no free referenced
 * point on any rank (decided collectively, once per solve), an empty free-intrinsics set and
 * EXPLICIT_SCHUR (requested, or AUTO, which then resolves to EXPLICIT_SCHUR on any world size:
 * U is all-reduced by the evaluation pass already), there is no Schur complement: S = U + D^2,
 * summary.schur_assembly = DAB_SCHUR_DIRECT. Without arc-ring cross blocks S is block diagonal
 * and every camera's 6x6 block is solved on its own (no dense S is allocated); with cross blocks
 * (the rig) S is filled from U and factored densely. No point factor, Y or pair / tile tables
 * either way. DAB_POINTS_DIRECT=0 in the environment (read at dab_create) forces the general
 * masked step for this case; so do a non-empty free-intrinsics set and an explicitly requested
 * IMPLICIT_SCHUR_PCG.
 *
 * No free parameter at all (every referenced point constant, and freeze_camera or no free
 * extrinsic): dab_solve returns DAB_OK with DAB_CONVERGENCE, num_iterations = 0, no iteration
 * record, initial_cost == final_cost and Ceres' message "Function tolerance reached. No
 * non-constant parameter blocks found."; the parameters are untouched.
 *
 * Covariance: Sigma is over the free points, the free extrinsics and (second call) the active
 * intrinsic scalars; point_cov rows of constant points are exactly 0 (known exactly, as
 * intr_cov's inactive slots), unreferenced points stay NaN, and constant points are left out of
 * the point rank test, deficient_points and first_deficient_point. With every point constant
 * Sigma_cc = U^-1.
 *
 * dab_eval_residuals, dab_eval_jacobians, dab_filter, dab_bench_eval_pass and
 * dab_bench_get_blocks ignore the mask (raw quantities). Errors: DAB_E_INVALID for a null handle
 * (checked before any device use); DAB_E_STATE before dab_set_problem. */
int dab_set_points_constant(dab_handle* h, const uint8_t* mask /* [num_points], caller order; NULL = all free */);
int dab_get_points_constant(dab_handle* h, uint8_t* mask /* nullable */, int32_t* num_constant /* nullable */);

/* ---- constant scalars of an extrinsic ---------------------------------------------------
 * ParameterBlock::get() hands Ceres an extrinsic as two blocks, rotation and translation, and
 * sfm.cc:51-52 freezes them with two separate SetParameterBlockConstant lines; Ceres'
 * SubsetManifold holds single coordinates constant. ext_const and freeze_camera know only "all
 * or nothing". Here it is a mask on the handle, one byte per extrinsic, bit k = scalar k of
 * ext[e] = (w0,w1,w2,t0,t1,t2) is constant (NULL = none, the default): the minimal hard gauge
 * (camera 0 constant plus one translation coordinate of a second camera: 7 scalars, where one
 * more constant extrinsic removes 6 degrees of freedom to fix one), a turntable ring whose
 * translation is a design value, arc positions known from CAD, rotation-only or translation-only
 * refinement.
 *
 * The mask is state of the handle, set after dab_set_problem; dab_set_problem resets it to none
 * (num_ext may change); it survives dab_update_parameters and every other setter and takes effect
 * at the next dab_solve, dab_covariance or dab_covariance_intrinsics. In a multi-rank handle
 * every rank sets the same mask (extrinsics are replicated).
 *
 * Effective set. Only bits on an extrinsic of the free set count: referenced on some rank, not
 * ext_const, freeze_camera not set; all other bits are ignored. dab_get_ext_scalars_constant
 * returns the bytes as set (zeros when never set) and in *num_constant_scalars the effective
 * bits. With no effective bit (never set, NULL, all zero, only constant or unreferenced
 * extrinsics flagged, freeze_camera) every call gives bitwise what it gives on a handle that
 * never set a mask, and no masked kernel is launched.
 *
 * A constant scalar is out of the problem, as a constant point is: it is not counted in
 * num_parameters (dab_summary and both covariance infos), takes no part in gradient_max_norm,
 * x_norm or step_norm, has no Jacobi scale or LM diagonal of its own, and is never written: its
 * double in the caller's `ext` and in dab_get_parameters is bitwise the input, also after
 * rejected steps and for an input of -0.0. Its observations keep every residual, cost and other
 * column. Deliberate differences to Ceres' SubsetManifold: there x_norm runs over the ambient
 * block and num_parameters counts ambient sizes; here both run over the free scalars.
 *
 * The camera set does not change: num_free_ext, the row order of ug, ext_cov, ext_full and
 * cam_full and the Schur tables stay as they are. An extrinsic with all six bits set stays in
 * the reduced system as six decoupled unit rows; ext_const is the way to take it out (the two
 * solves agree to rounding). Every linear solver, assembly, loss, free-intrinsics, constant-
 * points and prior combination that works without the mask works with it ("Constant
 * scalars of an extrinsic"). No free parameter at all (every referenced point constant, every
 * scalar of every free extrinsic constant, no free intrinsic): the "No non-constant parameter
 * blocks found" summary described under constant points, the parameters untouched.
 *
 * Extrinsic priors keep Ceres' semantics: the residual is A (x_e - mu) over all six values; a
 * constant scalar enters through the constant offset only, its column of A gives no gradient or
 * curvature. dab_eval_ext_priors is unchanged.
 *
 * Covariance: Sigma is over the free scalars. Rows and columns of constant scalars in ext_cov,
 * ext_full and cam_full are exactly 0 (known exactly, like inactive intrinsic slots), and they
 * are left out of the camera rank test, like the unit rows of inactive intrinsic slots.
 *
 * dab_eval_residuals, dab_eval_jacobians, dab_eval_intrinsic_jacobians, dab_filter,
 * dab_bench_eval_pass, dab_bench_get_blocks and dab_get_intrinsic_blocks ignore the mask (raw
 * quantities). Errors, state unchanged: DAB_E_INVALID for a null handle (checked before any
 * device use) or a byte above 63; DAB_E_STATE before dab_set_problem. */
#define DAB_EXT_ROTATION    0x07  /* w0 w1 w2: block [4] / [6], sfm.cc:51 */
#define DAB_EXT_TRANSLATION 0x38  /* t0 t1 t2: block [5] / [7], sfm.cc:52 */
int dab_set_ext_scalars_constant(dab_handle* h, const uint8_t* bits /* [num_ext]; bit k = scalar k constant; NULL = none */);
int dab_get_ext_scalars_constant(dab_handle* h, uint8_t* bits /* nullable */, int32_t* num_constant_scalars /* nullable */);

/* ---- Gaussian priors on extrinsics ------------------------------------------------------
 * "This pose is known to within sigma", without holding it constant: what in Ceres is
 *   problem.AddResidualBlock(new ceres::NormalPrior(A, mu), NULL, ext)
 * on an extrinsic's block. A prior adds the residual block r = A (x_e - mu) to the problem,
 * x_e = ext[e] = (w, t) as the library stores it (the angle-axis vector as it stands, no rotation
 * manifold), A = sqrt_info 6x6 row-major. Rows of A may be zero: a position-only prior is
 * A = [0 0; 0 I / sigma]. The prior adds 0.5 |r|^2 to every cost dab_solve and the covariance
 * calls report and is never under the handle's robust loss (a NULL loss of its own). Uses: a rig
 * whose arcs and rings have design values (between "constant" and "free"), and the soft remedy
 * for the scale gauge dab_covariance needs: a position prior on one or a few cameras gives a
 * covariance that carries that uncertainty instead of claiming it is zero.
 *
 * The priors are state of the handle, like the loss and the masks: set after dab_set_problem,
 * which resets them to none (num_ext may change); they survive dab_update_parameters,
 * dab_set_loss, dab_set_intrinsics_free and dab_set_points_constant and take effect at the next
 * dab_solve, dab_covariance or dab_covariance_intrinsics. count = 0 (arrays may be NULL) clears
 * them. At most one prior per extrinsic. In a multi-rank handle every rank sets the same priors
 * (extrinsics are replicated; the prior's sums are added once, after the sums over the ranks,
 * identically on every rank).
 *
 * Effective set. A prior is effective when its extrinsic is in the free set the solve uses:
 * referenced on some rank, not ext_const, freeze_camera not set. Any other prior is ignored
 * entirely: no cost, no residual rows, zeros from dab_eval_ext_priors. This is a deliberate
 * simplification: Ceres would carry the constant cost of such a block. *num_effective counts
 * the effective priors; dab_summary.num_residuals and dab_covariance_info.num_residuals grow by 6
 * per effective prior, num_parameters is unchanged. With no effective prior (never set, count 0,
 * only constant or unreferenced extrinsics named, freeze_camera) every call gives bitwise what it
 * gives on a handle that never set one, and no prior kernel is launched.
 *
 * Where it enters: A^T A and A^T r are added to the camera's U | g_c row after each evaluation
 * pass and its all-reduce, so every linear solver, assembly, pcg_fp32, loss, free-intrinsics and
 * constant-points combination that works without priors works with them (there are no new
 * DAB_E_UNSUPPORTED cases); the model cost change and the candidate cost get the prior's terms
 * after the candidate pass. Every prior sum has a fixed order: two solves agree bitwise.
 *
 * dab_get_ext_priors returns what was set (arrays nullable, sized by a first call for *count).
 * dab_eval_ext_priors evaluates at the parameters now on the handle: residuals [count][6] in the
 * order set, cost = 0.5 sum |r|^2 over the effective priors.
 *
 * dab_eval_residuals, dab_eval_jacobians, dab_filter, dab_bench_eval_pass, dab_bench_get_blocks,
 * dab_get_intrinsic_blocks and dab_jacobian_bytes ignore priors (raw observation quantities;
 * dab_bench_get_blocks reads the camera rows where the last evaluation left them: raw after
 * dab_bench_eval_pass, with A^T A | A^T r added after a dab_solve or covariance call with priors).
 * Errors, all leaving the state unchanged: DAB_E_INVALID for a null handle (checked before any
 * device use), count < 0, a null array with count > 0, an index outside [0, num_ext), a duplicate
 * index, or a non-finite entry of mean or sqrt_info; DAB_E_STATE before dab_set_problem. */
int dab_set_ext_priors(dab_handle* h, int32_t count, const int32_t* ext_index /* [count] */,
                       const double* mean /* [count][6] */, const double* sqrt_info /* [count][6][6] row-major */);
int dab_get_ext_priors(dab_handle* h, int32_t* count, int32_t* num_effective, int32_t* ext_index, double* mean,
                       double* sqrt_info);
int dab_eval_ext_priors(dab_handle* h, double* residuals /* [count][6], as set; nullable */, double* cost /* nullable */);

/* ---- Gaussian priors on points -----------------------------------------------------------
 * "This point is known to within sigma", without holding it constant: a surveyed ground-control
 * point, a calibration-target corner. What in Ceres is
 *   problem.AddResidualBlock(new ceres::NormalPrior(A, mu), NULL, point)
 * on a point's block. A prior adds the residual block r = A (X_p - mu) to the problem, X_p =
 * points[p], A = sqrt_info 3x3 row-major. Rows of A may be zero: height-only control is
 * A = [0 0 0; 0 0 0; 0 0 1 / sigma]. The prior adds 0.5 |r|^2 to every cost dab_solve and the
 * covariance calls report and is never under the handle's robust loss (a NULL loss of its own).
 * It is the third state of a point between "free" and "constant" (dab_set_points_constant), the
 * soft remedy for the scale gauge dab_covariance needs (the covariance then carries the control
 * points' uncertainty instead of claiming it is zero), and the only prior that acts with
 * freeze_camera, where the points are the free parameters.
 *
 * The priors are state of the handle, like the loss, the masks and the extrinsic priors: set
 * after dab_set_problem, which resets them to none (num_points may change); they survive
 * dab_update_parameters, dab_set_loss, dab_set_intrinsics_free, dab_set_points_constant and
 * dab_set_ext_priors and take effect at the next dab_solve, dab_covariance or
 * dab_covariance_intrinsics. count = 0 (arrays may be NULL) clears them. point_index holds the
 * caller's point ids; at most one prior per point. In a multi-rank handle each rank sets the
 * priors of the points of its own shard, as with the constant mask (points are sharded: a prior's
 * sums go in on its rank, before the sums over the ranks); the calls that honour them are
 * collective already.
 *
 * Effective set. A prior is effective when its point is referenced on this rank and not constant.
 * Any other prior is ignored entirely: no cost, no residual rows, zeros from
 * dab_eval_point_priors, the same deliberate simplification as for extrinsic priors (Ceres would
 * carry the constant cost of such a block). freeze_camera does not disable point priors. Without a
 * free point on any rank (DAB_SCHUR_DIRECT) the effective set is empty by definition.
 * *num_effective counts this rank's effective priors; dab_summary.num_residuals and both
 * covariance infos' num_residuals grow by 3 per effective prior of this rank (they count this
 * rank's observations too), num_parameters is unchanged. With no effective prior on any rank
 * (never set, count 0, only constant or unreferenced points named) every call gives bitwise what
 * it gives on a handle that never set one, and no point-prior kernel is launched. (Whether any
 * rank has an effective prior is a second word in the max-reduce a multi-rank dab_solve already
 * makes per call; a multi-rank covariance call makes one such small reduce of its own.)
 *
 * Where it enters: A^T A and A^T r are added to the point's V | g after each evaluation pass, so
 * every linear solver, assembly, pcg_fp32, loss, free-intrinsics, constant-points,
 * extrinsic-prior and freeze_camera combination that works without point priors works with them
 * (there are no new DAB_E_UNSUPPORTED cases); the model cost change and the candidate cost get the
 * priors' terms after the candidate pass, before their sum over the ranks. Every prior sum has a
 * fixed order: two solves agree bitwise, and the result of a one-rank handle does not depend on
 * the order the priors were set in.
 *
 * dab_get_point_priors returns what was set (arrays nullable, sized by a first call for *count).
 * dab_eval_point_priors is not collective; it evaluates at the parameters now on the handle:
 * residuals [count][3] in the order set, cost = 0.5 sum |r|^2 over this rank's effective priors.
 *
 * dab_eval_residuals, dab_eval_jacobians, dab_filter, dab_bench_eval_pass, dab_bench_get_blocks,
 * dab_get_intrinsic_blocks and dab_jacobian_bytes ignore point priors (raw observation
 * quantities; dab_bench_get_blocks reads V | g where the last evaluation left them: raw after
 * dab_bench_eval_pass, with A^T A | A^T r added after a dab_solve or covariance call with priors).
 * Errors, all leaving the state unchanged: DAB_E_INVALID for a null handle (checked before any
 * device use), count < 0, a null array with count > 0, an index outside [0, num_points), a
 * duplicate index, or a non-finite entry of mean or sqrt_info; DAB_E_STATE before
 * dab_set_problem. */
int dab_set_point_priors(dab_handle* h, int32_t count, const int32_t* point_index /* [count], caller's point ids */,
                         const double* mean /* [count][3] */, const double* sqrt_info /* [count][3][3] row-major */);
int dab_get_point_priors(dab_handle* h, int32_t* count, int32_t* num_effective, int32_t* point_index, double* mean,
                         double* sqrt_info);
int dab_eval_point_priors(dab_handle* h, double* residuals /* [count][3], as set; nullable */, double* cost /* nullable */);

/* ---- Gaussian priors on intrinsics -------------------------------------------------------
 * "This calibration is known to within its certificate", between holding the intrinsics constant
 * (the default) and freeing them (dab_set_intrinsics_free): what in Ceres is
 *   problem.AddResidualBlock(new ceres::NormalPrior(A, mu), NULL, block)
 * on an intrinsic's blocks. Ceres keeps three blocks, [1] (cx, cy), [2] (f0, f1), [3] (k0, k1);
 * one 6x6 A over x_i = (cx, cy, f0, f1, k0, k1), dab_problem's slot layout, is the superset of
 * them: a block-diagonal A is three NormalPriors, a full A carries a calibration's
 * focal-distortion correlation. A prior on intrinsic i adds the residual block r = A (x_i - mu),
 * x_i at the values on the handle (the refined ones), A = sqrt_info 6x6 row-major. Rows and
 * columns of A may be zero. The prior adds 0.5 |r|^2 to every cost dab_solve and
 * dab_covariance_intrinsics report and is never under the handle's robust loss (a NULL loss of
 * its own). Uses: self-calibration from a calibration certificate, and the remedy for a problem
 * that is rank deficient for the intrinsics alone (a camera with too few observations for its
 * free intrinsic scalars).
 *
 * Inactive slots. A slot the model lacks (f1 with nf == 1, k beyond nk) or the mask leaves
 * constant takes no part: its column of A and its entry of mu are dropped,
 * r = A_act (x_act - mu_act). This is a deliberate simplification, the one below one level down:
 * Ceres would carry the constant offset A_inact (x_inact - mu_inact) of a constant block. The
 * values in A's inactive columns and mu's inactive entries change nothing, bitwise.
 *
 * The priors are state of the handle, like the loss, the masks and the other priors: set after
 * dab_set_problem, which resets them to none (num_intr may change); they survive
 * dab_update_parameters, dab_update_intrinsics, dab_set_loss, dab_set_intrinsics_free,
 * dab_set_points_constant, dab_set_ext_priors and dab_set_point_priors and take effect at the next
 * dab_solve or dab_covariance_intrinsics; dab_set_intrinsics_free after them changes the
 * effective set at that call. count = 0 (arrays may be NULL) clears them. At most one prior per
 * intrinsic. In a multi-rank handle every rank sets the same priors (intrinsics are replicated;
 * the prior's sums are added once, after the sums over the ranks, identically on every rank).
 *
 * Effective set. A prior is effective when its intrinsic is in the free set the solve uses:
 * referenced on some rank, at least one active scalar, freeze_camera not set: the set
 * dab_get_intrinsics_free counts. Any other prior is ignored entirely: no cost, no residual rows,
 * zeros from dab_eval_intr_priors (Ceres would carry the constant cost of such a block).
 * *num_effective counts the effective priors (collective on a multi-rank handle with a non-empty
 * mask, as dab_get_intrinsics_free is); dab_summary.num_residuals and
 * dab_covariance_info.num_residuals grow by 6 per effective prior, num_parameters is unchanged.
 * With no effective prior (never set, count 0, the mask all constant, only constant or
 * unreferenced intrinsics named, freeze_camera) every call gives bitwise what it gives on a
 * handle that never set one, and no prior kernel is launched. Plain dab_covariance is always in
 * this case: it refuses a non-empty free set. The effective priors are ordered by intrinsic index,
 * so the order they were set in changes nothing, bitwise.
 *
 * Where it enters: A^T A and A^T r are added to the intrinsic's U_zz | g_z after each evaluation
 * and its all-reduce, so the Jacobi scale, the gradient norm, the bordered system of the exact
 * step and dab_covariance_intrinsics take them with no other change (there are no new
 * DAB_E_UNSUPPORTED cases: the refusals of a non-empty free set stay as they are); the model cost
 * change and the candidate cost get the prior's terms after the candidate pass. Every prior sum
 * has a fixed order: two solves agree bitwise.
 *
 * dab_get_intr_priors returns what was set (arrays nullable, sized by a first call for *count).
 * dab_eval_intr_priors evaluates at the intrinsics now on the handle, for the mask now on it:
 * residuals [count][6] in the order set, cost = 0.5 sum |r|^2 over the effective priors. On a
 * multi-rank handle with priors set and a non-empty mask every rank calls it (it works out the
 * free set as dab_solve does).
 *
 * dab_eval_residuals, dab_eval_jacobians, dab_eval_intrinsic_jacobians, dab_filter,
 * dab_bench_eval_pass, dab_bench_get_blocks and dab_jacobian_bytes ignore these priors (raw
 * observation quantities). dab_get_intrinsic_blocks reads U_zz | g_z where the last evaluation
 * left them: raw after dab_bench_eval_pass, with A^T A | A^T r added after a dab_solve or a
 * dab_covariance_intrinsics call with effective priors.
 * Errors, all leaving the state unchanged: DAB_E_INVALID for a null handle (checked before any
 * device use), count < 0, a null array with count > 0, an index outside [0, num_intr), a duplicate
 * index, or a non-finite entry of mean or sqrt_info; DAB_E_STATE before dab_set_problem.
 * dab_eval_intr_priors returns DAB_E_UNSUPPORTED for more than 16 free intrinsics, as dab_solve
 * does. */
int dab_set_intr_priors(dab_handle* h, int32_t count, const int32_t* intr_index /* [count] */,
                        const double* mean /* [count][6] */, const double* sqrt_info /* [count][6][6] row-major */);
int dab_get_intr_priors(dab_handle* h, int32_t* count, int32_t* num_effective, int32_t* intr_index, double* mean,
                        double* sqrt_info);
int dab_eval_intr_priors(dab_handle* h, double* residuals /* [count][6], as set; nullable */, double* cost /* nullable */);

/* ---- evaluation (parity / filterPoint3d) ---------------------------------------------
 * residuals: [num_obs][2] in the caller's observation order.
 * jacobians: [num_obs][2][15] row-major, columns = [X(3) | w0(3) t0(3) | w1(3) t1(3)]
 *            (d r / d param, unscaled; w1/t1 columns are zero for single-extrinsic obs).
 * cost: 0.5 * sum r^2. Any pointer may be NULL. */
int dab_eval_residuals(dab_handle* h, double* residuals, double* cost);
int dab_eval_jacobians(dab_handle* h, double* residuals, double* jacobians);

/* DeepArcManager::filterPoint3d (DeepArcManager.cc:332-424) on the device, at the
 * parameters currently on the handle (after dab_solve: the optimised ones):
 *   1. an observation is dropped when mse = (r0^2 + r1^2) / 2 < error_boundary
 *      (quirk Q4: the *small*-error ones, exactly as the reference);
 *   2. a point with no remaining observation is dropped (Point3d::empty);
 *   3. a remaining point is dropped when |X - center|^2 > radius / 2 (radius is the
 *      fitted *squared* radius, hemisphere_radius.hh:26), and so are its observations.
 * obs_keep[num_obs] and point_keep[num_points] (caller order; 1 = kept) may be NULL;
 * unreferenced points are reported as dropped. Counts of kept items in *n_obs_kept /
 * *n_points_kept (nullable). The handle's problem is not modified. */
int dab_filter(dab_handle* h, double error_boundary, const double center[3], double radius,
               uint8_t* obs_keep, uint8_t* point_keep, int32_t* n_obs_kept, int32_t* n_points_kept);

/* ---- covariance at the current parameters (ceres::Covariance) -----------------------------
 * J = the Jacobian of the handle's problem at the parameters now on the handle, over the free
 * parameters only (referenced points, then referenced non-constant extrinsics, as
 * dab_summary.num_parameters counts them); under a non-trivial loss its rows are scaled by
 * sqrt(rho') exactly as dab_solve scales them. The covariance is Sigma = (J^T J)^-1, undamped
 * and without a sigma^2 factor: info->cost and the degrees of freedom (num_residuals -
 * num_parameters) let the caller multiply by 2 cost / dof. Returned are the diagonal blocks of
 * Sigma and, optionally, its whole camera part (the blocks between two points, or between a point
 * and an extrinsic or an intrinsic: dab_covariance_blocks):
 *   point_cov [num_points][6]   upper-packed 00 01 02 11 12 22, caller's point order; rows of
 *                               points referenced by no observation on this rank are NaN
 *   ext_cov   [num_free_ext][21] upper-packed 6x6 per free extrinsic, ascending extrinsic index
 *                               (dab_bench_get_blocks' order)
 *   ext_full  [6 nfe][6 nfe]    row-major, both triangles (bitwise symmetric; its diagonal
 *                               blocks equal ext_cov bitwise)
 * Every array may be NULL; with all three NULL the call fills info (sizes, rank test) only.
 * With freeze_camera, or no free extrinsic, Sigma_pp = V^-1 and the camera arrays are empty.
 *
 * Route: always the exact one, all fp64, whatever solver the handle last used and whatever
 * pcg_fp32 said: evaluation pass, point factor without LM diagonal, explicit Schur complement
 * S (pair tables or block tiles, built on first use as dab_solve does for EXPLICIT_SCHUR),
 * dense Cholesky, C = S^-1 from the factor, Sigma_pp = PU (I + sum Y^T C Y) PU^T, all in the
 * Jacobi-scaled variables (jacobi_scaling) and unscaled at the end. The first call that needs C
 * allocates a second n x n buffer (n = 6 num_free_ext; DAB_E_NOMEM when it cannot), freed by
 * dab_set_problem and dab_destroy. The handle's parameters, loss and problem are unchanged: a
 * dab_solve after it gives bitwise the trajectory it would have given without it, and two calls
 * in a row give bitwise the same arrays.
 *
 * Rank test, fail closed. J^T J must be invertible, and for this project's problems it often
 * is not: the reference's own gauge rule (only arc 0 constant, sfm.cc:50-53) leaves the global
 * scale of the rig free (J^T J has exactly one singular value at ~1e-11 of the largest; its null
 * vector is translations plus points), and so does a BAL-shaped problem with one constant
 * camera. A point with a single observation has a rank-2 block. The call tests
 *   - every point's scaled undamped 3x3 block: min / max pivot of its Cholesky must be
 *     > min_pivot_ratio;
 *   - the camera system: the dense factor must not flag a non-positive pivot, and min / max of
 *     its squared diagonal must be > min_pivot_ratio.
 * Measured ratios: >= 9.9e-3 on well-posed problems, |ratio| <= 2.5e-12 on gauge-free ones,
 * <= 5e-15 for single-observation points; the default 1e-10 sits between. A failure returns
 * DAB_OK with info->status = DAB_COV_RANK_DEFICIENT and writes no array; the point side fills
 * first_deficient_point / deficient_points, the camera side camera_pivot_ratio (0 when the
 * factor met a non-positive pivot). Deficient points are not skipped: their observations would
 * still sit in U and S would be overconfident. Remedies: drop such points from the problem
 * (Problem.subset in the Python layer), and fix the scale gauge with one constant point
 * (dab_set_points_constant: a ground-control point) or with one more constant extrinsic
 * (ext_const) beside the reference's arc 0 / camera 0, or, minimally, with one constant
 * translation coordinate of a second extrinsic (dab_set_ext_scalars_constant: the 7-scalar
 * gauge; a rotation coordinate does not fix the scale); or, softly, with a position prior on one
 * or a few cameras (dab_set_ext_priors) or a prior on a few ground-control points
 * (dab_set_point_priors), whose uncertainty the covariance then carries. A deficiency of the
 * intrinsics alone under dab_covariance_intrinsics (a camera with too few observations for its
 * free scalars) has its own soft remedy: a calibration prior (dab_set_intr_priors).
 *
 * Multi-rank handles: every rank calls it. S is all-reduced as in the exact step, every rank
 * inverts its own copy (identical camera arrays) and gets the covariances of its own shard's
 * points; the point-side deficiency count is max-reduced, so every rank returns the same status.
 * Errors: DAB_E_INVALID for a null handle (checked before any device use), a min_pivot_ratio
 * that is not finite and > 0, or a null info together with null arrays; DAB_E_STATE before
 * dab_set_problem. */
#define DAB_COV_OK 0
#define DAB_COV_RANK_DEFICIENT 1
typedef struct dab_covariance_options {
  double min_pivot_ratio;   /* 1e-10; see the rank test */
  int32_t jacobi_scaling;   /* 1 */
  int32_t reserved;
} dab_covariance_options;
void dab_covariance_options_init(dab_covariance_options* opt);

typedef struct dab_covariance_info {
  int32_t status;                 /* DAB_COV_OK | DAB_COV_RANK_DEFICIENT */
  int32_t num_free_ext, num_free_points;
  int32_t first_deficient_point;  /* caller's point index (the lowest on this rank), or -1 */
  int32_t deficient_points;       /* count (max over the ranks) */
  int32_t schur_assembly;         /* DAB_SCHUR_PAIRS | DAB_SCHUR_TILES */
  double point_pivot_ratio_min, camera_pivot_ratio;  /* what the rank test saw */
  double cost; int32_t num_residuals, num_parameters;
  double evaluate_ms, factor_ms, inverse_ms, points_ms;  /* device times, HIP events */
} dab_covariance_info;

int dab_covariance(dab_handle* h, const dab_covariance_options* opt /* NULL = defaults */,
                   double* point_cov, double* ext_cov, double* ext_full, dab_covariance_info* info);

/* ---- covariance with free intrinsics ------------------------------------------------------
 * dab_covariance refuses a handle with a non-empty free set (dab_set_intrinsics_free): treating
 * the intrinsics as exactly known understates every other variance. This call is the same
 * contract over one more parameter group: Sigma = (J^T J)^-1 over the referenced points, the
 * free extrinsics and the active intrinsic scalars (those dab_solve counts in num_parameters,
 * which info->num_parameters includes here), undamped, no sigma^2 factor, rows scaled by
 * sqrt(rho') under a loss, all fp64, jacobi_scaling honoured.
 *   point_cov, ext_cov  as dab_covariance
 *   intr_cov [nfi][21]  upper-packed 6x6 per free intrinsic, ascending intrinsic index, slots
 *                       (cx, cy, f0, f1, k0, k1)
 *   cam_full [n'][n']   row-major, n' = 6 nfe + 6 nfi: extrinsics first, then intrinsics; both
 *                       triangles, bitwise symmetric, its diagonal 6x6 blocks equal ext_cov and
 *                       intr_cov bitwise
 * Slots a model lacks or the mask leaves out are known exactly: their rows and columns in
 * intr_cov and cam_full are exactly 0. Every array may be NULL; with all NULL the call is the
 * size and rank query (zinfo: num_free_intr, num_free_scalars). With an empty free set (mask
 * never set, all zero, or freeze_camera) every array and info are bitwise dab_covariance's:
 * intr_cov is empty and cam_full is ext_full.
 *
 * Route: the exact step's bordered system S' of n' rows ("Covariance with free
 * intrinsics") built as one undamped LM step builds it, its Cholesky factor, C' = S'^-1 from the
 * factor (a second n' x n' buffer, lazy, DAB_E_NOMEM when it cannot be had, freed by
 * dab_set_problem and dab_destroy), and the point fold-back over the cameras and the free
 * intrinsics each point sees. zinfo->border_ms is the device time of the z rows of S'.
 *
 * Rank test: dab_covariance's, on the factor of the n' system: the camera test takes min / max of
 * the squared diagonal over the rows of extrinsics and of active intrinsic scalars (the unit rows
 * of inactive slots are left out). Return value, camera_pivot_ratio and "no array is written on
 * a failure" as there.
 *
 * Refusals, state unchanged: DAB_E_UNSUPPORTED for more than 16 free intrinsics and for a
 * non-empty free set without a free extrinsic (dab_solve's rule and wording); DAB_E_INVALID and
 * DAB_E_STATE as dab_covariance. The handle's parameters, intrinsics, mask, loss and problem
 * are untouched, a dab_solve after the call walks bitwise the trajectory it would have walked
 * without it, and two calls in a row give bitwise equal arrays. Collective on a multi-rank
 * handle: the border sums are all-reduced as in the step, every rank gets identical ext_cov,
 * intr_cov and cam_full and its own shard's points. */
typedef struct dab_covariance_intr_info {
  int32_t num_free_intr;     /* free intrinsics (the set dab_solve would use) */
  int32_t num_free_scalars;  /* their active scalars */
  double border_ms;          /* device time of the z rows of S' (HIP events) */
  double reserved;
} dab_covariance_intr_info;

int dab_covariance_intrinsics(dab_handle* h, const dab_covariance_options* opt /* NULL = defaults */,
                              double* point_cov, double* ext_cov, double* intr_cov, double* cam_full,
                              dab_covariance_info* info, dab_covariance_intr_info* zinfo);

/* ---- cross blocks of the covariance ------------------------------------------------------------
 * The blocks of Sigma that involve a point and something else, for a caller-given list of pairs:
 * what ceres::Covariance answers for any two parameter blocks and the two calls above leave out
 * (the pairs of two cameras are in ext_full / cam_full).
 *   pp_cov [num_pp][9]   Sigma_ab, row-major 3x3, rows point a, columns point b
 *   pe_cov [num_pe][18]  Sigma_pe, row-major 3x6, rows the point, columns w0 w1 w2 t0 t1 t2
 *   pz_cov [num_pz][18]  Sigma_pz, row-major 3x6, rows the point, columns cx cy f0 f1 k0 k1
 * Points are the caller's point ids, extrinsics and intrinsics the problem's indices (not the
 * positions in ext_cov / intr_cov). Duplicates and (a, a) are allowed. The block (a, b) is bitwise
 * the transpose of the block (b, a): both are one computation, and (a, a) is symmetric bitwise.
 * (a, a) is point_cov's block within the accuracy of the route, not bitwise (the two sum in
 * different orders).
 *
 * Which Sigma: one call serves both kinds of handle. With an empty free set it is dab_covariance's
 * Sigma, with a non-empty one dab_covariance_intrinsics's, with their options, their rank test,
 * info and zinfo, loss, priors, constant points, constant extrinsic scalars and freeze_camera: the
 * call is theirs with the fold-back run for the pairs ("Covariance cross blocks").
 *
 * Known exactly, written as +0: a block with a constant point (dab_set_points_constant); a pe block
 * of a constant extrinsic (ext_const, freeze_camera); the columns of constant extrinsic scalars
 * (dab_set_ext_scalars_constant) and of inactive intrinsic slots; a pz block of an intrinsic that
 * is not in the free set. No information, written as NaN (as point_cov's rows): a block with a
 * point referenced by no observation on this rank, and a pe block of a non-constant extrinsic that
 * nothing references. NaN goes before +0 where both apply.
 *
 * req NULL or all three counts 0: the size and rank query (info, zinfo). A list with count > 0 and
 * a NULL index or output array, a negative count, or an index out of range: DAB_E_INVALID, nothing
 * written, state unchanged. The other refusals are those of the two calls above (more than 16 free
 * intrinsics, a non-empty free set without a free extrinsic: DAB_E_UNSUPPORTED). On
 * DAB_COV_RANK_DEFICIENT no array is written. blocks_ms (nullable): the device time of the
 * cross-block kernels (HIP events; 0 when none ran); info->points_ms is the point blocks' fold-back,
 * which runs here too (it builds the records the pairs read).
 *
 * The pair lists are translated on the host and uploaded once per call; device scratch is lazy and
 * freed by dab_set_problem and dab_destroy. Two calls in a row give bitwise equal arrays; a
 * dab_solve after the call walks bitwise the trajectory it would have walked without it; the two
 * calls above return bitwise what they return without it. Collective on a multi-rank handle: each
 * rank asks about its own shard's points (a point of another rank is NaN), the camera side is
 * identical on all ranks. */
typedef struct dab_cov_blocks_request {
  int32_t num_pp; const int32_t* pp;   /* [num_pp][2] caller's point ids (a, b)            */
  int32_t num_pe; const int32_t* pe;   /* [num_pe][2] (caller's point id, extrinsic index) */
  int32_t num_pz; const int32_t* pz;   /* [num_pz][2] (caller's point id, intrinsic index) */
} dab_cov_blocks_request;

int dab_covariance_blocks(dab_handle* h, const dab_covariance_options* opt /* NULL = defaults */,
                          const dab_cov_blocks_request* req,
                          double* pp_cov /* [num_pp][9]  row-major 3x3, rows a, cols b        */,
                          double* pe_cov /* [num_pe][18] row-major 3x6, cols w0 w1 w2 t0 t1 t2 */,
                          double* pz_cov /* [num_pz][18] row-major 3x6, cols cx cy f0 f1 k0 k1 */,
                          dab_covariance_info* info, dab_covariance_intr_info* zinfo,
                          double* blocks_ms /* nullable: device time of the new kernels */);

/* Dense SPD solve A x = b on the handle's device with the library's blocked Cholesky (the
 * reduced-camera-system factorisation of DAB_LINEAR_SOLVER_EXPLICIT_SCHUR; Eigen LLT in
 * Ceres' DENSE_SCHUR). A: n x n row-major, only the lower triangle is read. factor_ms
 * (nullable): device time of factorisation + solves. Returns DAB_OK, 1 when A is not
 * numerically positive definite, or a negative error. */
int dab_dense_spd_solve(dab_handle* h, int n, const double* A, const double* b, double* x,
                        double* factor_ms);

/* ---- benchmark hooks -------------------------------------------------------------------
 * `count` evaluation passes on device-resident data, enqueued back to back: residual +
 * Jacobian with the JtJ / Jtr block assembly (per-point V,g and per-camera U,g, all-reduced
 * across ranks). Asynchronous on the handle's stream; dab_sync waits for them. One call per
 * batch keeps the host's launch cost off the device's critical path. */
int dab_bench_eval_pass(dab_handle* h, int with_assembly, int count);
int dab_sync(dab_handle* h);
/* What the last evaluation pass left on the device, copied to host arrays (the benchmark's
 * output dump; waits for the handle's stream). V[num_points][6] (upper-packed 3 x 3 point
 * blocks) and g[num_points][3] in the caller's point order, zero for points of no
 * observation on this rank; ug[*num_free_ext][27] (U upper-packed (21) | g_c (6) per free
 * extrinsic in ascending index, summed over the ranks); ux[*num_cross][36] (the arc-ring cross blocks);
 * *cost = 0.5 * sum r^2. Every pointer may be NULL: query the two counts first, then call
 * again with arrays of those sizes. The handle's state is unchanged.
 * Cross blocks: one per (arc, ring) = (ext0, ext1) pair that has, on some rank, a composed
 * observation whose two extrinsics are both free. Order: ascending key col(ext0) * num_free_ext
 * + col(ext1), col = the extrinsic's rank among the free ones (its row in ug), i.e. by arc, then
 * by ring. Orientation: the 36 numbers are J_c0^T J_c1 row-major, ux[k][6 a + b] = sum over the
 * pair's observations and their two residual rows of (d r / d ext0_a) (d r / d ext1_b): rows
 * index the arc's (w, t), columns the ring's; this is the block at (row block col(ext0),
 * column block col(ext1)) of the camera part of J^T J; the block at (col(ext1), col(ext0)) is its
 * transpose and is not stored. */
int dab_bench_get_blocks(dab_handle* h, int32_t* num_free_ext, int32_t* num_cross, double* V, double* g,
                         double* ug, double* ux, double* cost);
/* Kernel timing: average device time (ms) of the point-side residual+Jacobian kernel and
 * of the rest of the pass, over the passes since the last call, measured with HIP events on
 * the handle's stream (every 8th pass of a dab_bench_eval_pass batch and its first one;
 * environment DAB_BENCH_SAMPLE sets the stride). */
int dab_bench_kernel_ms(dab_handle* h, double* jac_ms, double* assembly_ms);
/* Algorithmic HBM bytes of one residual+Jacobian launch on the resident problem. */
int dab_jacobian_bytes(dab_handle* h, double* bytes);
/* The rig's pair-major camera kernel (k_eval_pair; composed observations with both
 * cameras free): its average device time (ms) over the sampled passes of the batches read
 * by the last dab_bench_kernel_ms call, and its algorithmic bytes per launch (0 when the
 * resident problem has no pair-major pass). */
int dab_bench_pair_ms(dab_handle* h, double* ms, double* bytes);
/* Which evaluation schedule the resident problem uses: *fused = 1 when the pass is the
 * single fused launch (k_eval_fused: camera and point side together), 2 when it is the
 * same kernel as a camera-side then a point-side launch (several ranks: the camera blocks'
 * all-reduce overlaps the point side), 0 for the two-kernel pass (k_eval_cams +
 * k_eval_points). */
int dab_eval_schedule(dab_handle* h, int32_t* fused);
/* After an IMPLICIT_SCHUR_PCG solve: *matrix_free = 1 when the Schur products re-evaluate
 * the observation rows in every pass (small camera sets, fp64, no Y records), 2 for the
 * same with pcg_fp32 (fp32 per-observation arithmetic, fp64 sums and true residuals), 0 for
 * the stored-Y products. */
int dab_pcg_schedule(dab_handle* h, int32_t* matrix_free);
/* How the handle's sums over ranks run: *p2p = 1 when the one-shot peer-to-peer all-reduce
 * over xGMI (IPC-mapped peer regions, fixed rank order) carries the camera-sized sums (every
 * pair of devices peer-accessible; environment DAB_P2P=0 disables it, DAB_P2P=1 also enables
 * it on host-staged handles), 0 when every collective is RCCL or host-staged. */
int dab_comm_schedule(dab_handle* h, int32_t* p2p);

/* ---- host utilities (no device needed) ----------------------------------------------- */
/* Deterministic synthetic problems. kind 0: BAL-shaped (non-shared, one
 * intrinsic per camera); kind 1: DeepArc rig (arcs x rings, shared intrinsics).
 * Query sizes with arrays NULL, then call again with caller-allocated arrays. */
typedef struct dab_synth_config {
  int32_t kind;          /* 0 BAL-shaped, 1 rig */
  int32_t num_cameras;   /* kind 0 */
  int32_t num_arcs;      /* kind 1 */
  int32_t num_rings;     /* kind 1 */
  int32_t num_points;
  int32_t obs_per_point;
  uint64_t seed;         /* cameras, intrinsics and their initial values */
  uint64_t point_seed;   /* points/observations stream; 0 = continue the `seed` stream.
                            Shards of one global problem share `seed` and differ here. */
  double pixel_noise;    /* 1.0 */
  double point_noise;    /* 0.01 */
  double rot_noise;      /* 1e-3 */
  double trans_noise;    /* 1e-3 */
} dab_synth_config;

int dab_synth_sizes(const dab_synth_config* cfg, int32_t* num_obs, int32_t* num_points,
                    int32_t* num_ext, int32_t* num_intr);
/* Fills the arrays of `p` (sizes must match dab_synth_sizes). ext_const gets the
 * gauge rule of sfm.cc:50-53. */
int dab_synth_fill(const dab_synth_config* cfg, dab_problem* p, uint8_t* ext_const);

#ifdef __cplusplus
}
#endif
#endif /* DAB_H_ */
