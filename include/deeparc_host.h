/*
 * deeparc_host.h — C ABI of the host adapter (deeparc-sfm_amd/host, libdeeparc_host.so).
 *
 * The C++ API in deeparc-sfm_amd/host mirrors the reference's host classes
 * (DeepArcManager, ParameterBlock, Point3d, Intrinsic, Extrinsic, Camera) and the driver
 * functions of src/sfm.cc (solve, the hemisphere fit, the solve -> filterPoint3d loop)
 * over libdab. This flat C layer exists for bindings and tests (ctypes); each function
 * names the reference call it wraps:
 *   dam_read / dam_write / dam_write_ply   DeepArcManager::read / write / writePly
 *                                          (DeepArcManager.cc:26-196, 426-499, 263-328)
 *   dam_solve                              solve(DeepArcManager&, ...), sfm.cc:31-75
 *   dam_filter                             DeepArcManager::filterPoint3d, DeepArcManager.cc:332-424
 *   dam_camera_centers                     DeepArcManager::getCameraCenter, DeepArcManager.cc:501-518
 *   dam_fit_hemisphere                     the HemisphereRadius fit, sfm.cc:83-101
 *   dam_run_pipeline                       main(), sfm.cc:79-129
 *   dam_covariance                         (no reference call: ceres::Covariance after Solve)
 *   dam_covariance_intrinsics              (the same with the free intrinsic groups as unknowns)
 * Return 0 on success, negative on error (message in dam_last_error; the C++ API throws
 * const char* like the reference).
 */
#ifndef DEEPARC_HOST_H_
#define DEEPARC_HOST_H_

#include <stdint.h>

#include "dab.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dam_manager dam_manager;

const char* dam_last_error(void);
int dam_create(dam_manager** out);
int dam_destroy(dam_manager* m);
int dam_read(dam_manager* m, const char* path);
int dam_write(dam_manager* m, const char* path);
int dam_write_ply(dam_manager* m, const char* path);
/* sizes of the current scene; shared = rig mode (n_ring != 0) */
int dam_sizes(dam_manager* m, int32_t* n_blocks, int32_t* n_points, int32_t* n_intr, int32_t* n_ext,
              int32_t* shared, int32_t* n_arc, int32_t* n_ring);
/* xyz [n_points][3], rgb [n_points][3] (either may be NULL) */
int dam_get_points(dam_manager* m, double* xyz, int32_t* rgb);
/* ext [n_ext][6] = (w, t); intr [n_intr][6] = (cx, cy, f0, f1, k0, k1) (either may be NULL) */
int dam_get_cameras(dam_manager* m, double* ext, double* intr);
/* per block: pos_arc, pos_ring, index of its point in the current point list, (x, y) */
int dam_get_blocks(dam_manager* m, int32_t* pos_arc, int32_t* pos_ring, int32_t* point_index, double* xy);
/* solve(m, max_iteration, max_second, freeze_camera) with the given linear solver;
 * summary may be NULL */
int dam_solve(dam_manager* m, int32_t max_iteration, int32_t max_second, int32_t freeze_camera,
              int32_t linear_solver_type, dab_summary* summary);
/* Robust loss (DAB_LOSS_*, scale; dab_set_loss in dab.h) of every later solve of this
 * manager; the default is the reference's NULL loss (sfm.cc:48-49). A bad type or scale
 * returns an error and leaves the loss as it was. dam_filter keeps the bare residual. */
int dam_set_loss(dam_manager* m, int32_t loss_type, double scale);
/* Intrinsic groups (DAB_INTR_* bits of dab.h, for every intrinsic) that every later solve of
 * this manager refines: the equivalent of deleting sfm.cc:60-62. The default 0 keeps them
 * constant as the reference does. The refined values are written back into the manager's
 * intrinsics untruncated, so dam_get_cameras and dam_write see them. Bits above 7 return an
 * error and leave the setting as it was. */
int dam_set_intrinsics_free(dam_manager* m, int32_t groups);
/* all != 0: every later solve of this manager holds every point constant and refines the cameras
 * alone (dab_set_points_constant with every point flagged: the reference's commented-out
 * sfm.cc:59, all or nothing as that line is). 0, the default, frees them again. Re-applied after
 * every re-set of the resident problem, like the loss and the intrinsic groups. */
int dam_set_points_constant(dam_manager* m, int32_t all);
/* Constant scalars of the extrinsics for every later solve of this manager
 * (dab_set_ext_scalars_constant in dab.h): bits [number of extrinsics], in the order of
 * dam_get_cameras' extrinsics, bit k = scalar k of (rotation, translation) is constant
 * (DAB_EXT_ROTATION 0x07, DAB_EXT_TRANSLATION 0x38); NULL clears it. A byte above 63 returns an
 * error and leaves the setting as it was. Re-applied after every re-set of the resident problem,
 * like the loss, the groups and the point flag; bits on a constant extrinsic are ignored. */
int dam_set_ext_scalars_constant(dam_manager* m, const uint8_t* bits);
/* Gaussian priors on extrinsics for every later solve of this manager (dab_set_ext_priors in
 * dab.h; Ceres: problem.AddResidualBlock(new NormalPrior(A, mu), NULL, ext)): ext_index [count]
 * in the order of dam_get_cameras' extrinsics, mean [count][6] = (rotation, translation),
 * sqrt_info [count][6][6] row-major = A of the residual A (x - mean). count = 0 clears them. An
 * index outside the manager's extrinsics, a negative count or a null array with count > 0 return an
 * error and leave the setting as it was; duplicates and non-finite entries are refused by the
 * solve that applies them. Re-applied after every re-set of the resident problem, like the loss,
 * the groups and the point flag; a prior on a constant extrinsic is ignored. */
int dam_set_ext_priors(dam_manager* m, int32_t count, const int32_t* ext_index, const double* mean,
                       const double* sqrt_info);
/* Gaussian priors on points for every later solve of this manager (dab_set_point_priors in dab.h;
 * ground-control points): point_index [count] into the manager's current point list (the order of
 * dam_get_points), mean [count][3], sqrt_info [count][3][3] row-major = A of the residual
 * A (X - mean). count = 0 clears them. An index outside the point list, a negative count or a null
 * array with count > 0 return an error and leave the setting as it was; duplicates and non-finite
 * entries are refused by the solve that applies them. Re-applied after every re-set of the resident
 * problem. dam_filter_point3d renumbers them with the point list: a surviving point keeps its prior
 * under its new index, a removed point's prior is dropped. dam_get_point_priors returns the current
 * setting (arrays nullable, sized by a first call for *count). */
int dam_set_point_priors(dam_manager* m, int32_t count, const int32_t* point_index, const double* mean,
                         const double* sqrt_info);
int dam_get_point_priors(dam_manager* m, int32_t* count, int32_t* point_index, double* mean, double* sqrt_info);
/* Gaussian priors on intrinsics for every later solve of this manager (dab_set_intr_priors in
 * dab.h; Ceres: NormalPrior(A, mu) with a NULL loss over the intrinsic's blocks [1] [2] [3]): a
 * calibration with its covariance for the groups dam_set_intrinsics_free frees. intr_index
 * [count] in the order of dam_get_cameras' intrinsics, mean [count][6] = (cx, cy, f0, f1, k0, k1),
 * sqrt_info [count][6][6] row-major = A of the residual A (x - mean). count = 0 clears them. An
 * index outside the manager's intrinsics, a negative count or a null array with count > 0 return
 * an error and leave the setting as it was; duplicates and non-finite entries are refused by the
 * solve that applies them. Re-applied after every re-set of the resident problem, like the other
 * priors; slots the model lacks or the groups leave constant take no part, and without free groups
 * the priors are ignored. */
int dam_set_intr_priors(dam_manager* m, int32_t count, const int32_t* intr_index, const double* mean,
                        const double* sqrt_info);
/* DeepArcManager::covariance: dab_covariance (dab.h) of the manager's current scene at its
 * current parameters, under the manager's loss. extra_const[n_extra]: extrinsic indices held
 * constant beside the gauge rule's; the reference's rule leaves the rig's global scale free
 * (status DAB_COV_RANK_DEFICIENT), one more constant extrinsic fixes it. point_cov [n_points][6]
 * in point order; ext_cov [nfe][21]; ext_full [6 nfe][6 nfe]; ext_label [nfe][3] = (index in the
 * extrinsic list, 0 arc | 1 ring, arc or ring position). Every array may be NULL: query
 * info->num_free_ext first. A rank-deficient scene returns 0 and writes no array. */
int dam_covariance(dam_manager* m, const int32_t* extra_const, int32_t n_extra, int32_t freeze_camera,
                   double* point_cov, double* ext_cov, double* ext_full, int32_t* ext_label,
                   dab_covariance_info* info);
/* DeepArcManager::covarianceIntrinsics: dab_covariance_intrinsics (dab.h) of the same scene with
 * the groups of dam_set_intrinsics_free as unknowns. As dam_covariance (no freeze_camera), plus
 * intr_cov [nfi][21], intr_index [nfi] (index in the intrinsic list) and cam_full [n'][n'], n' =
 * 6 nfe + 6 nfi; query info->num_free_ext and zinfo->num_free_intr first. */
int dam_covariance_intrinsics(dam_manager* m, const int32_t* extra_const, int32_t n_extra, double* point_cov,
                              double* ext_cov, double* intr_cov, double* cam_full, int32_t* ext_label,
                              int32_t* intr_index, dab_covariance_info* info, dab_covariance_intr_info* zinfo);
int dam_filter(dam_manager* m, double error_boundary, const double center[3], double radius);
/* out [capacity][3]; *count = number of centres (may exceed capacity) */
int dam_camera_centers(dam_manager* m, double* out, int32_t capacity, int32_t* count);
/* centres [n][3]; center/radius are the starting point on input, the fit on output */
int dam_fit_hemisphere(const double* centers, int32_t n, double center[3], double* radius,
                       int32_t max_iteration);
/* hemi_out = (cx, cy, cz, R); counts_out = (rounds, blocks, points); output / ply_prefix
 * may be empty strings */
int dam_run_pipeline(const char* input, const char* output, const char* ply_prefix, int32_t max_iteration,
                     int32_t max_second, double error_boundary, double hemi_out[4], int32_t counts_out[3]);
/* the same loop with a full report; quiet != 0 suppresses the per-iteration progress and
 * the per-solve summary lines the reference prints */
typedef struct dam_pipeline_report {
  double hemisphere_center[3], hemisphere_radius;
  int32_t rounds, final_blocks, final_points, solves;
  int32_t lm_iterations, reserved;  /* LM iterations summed over the solves */
  double final_cost;                /* the last solve's final cost */
  double solve_seconds, filter_seconds, total_seconds;
  /* breakdown, seconds summed over the loop: .deeparc read, hemisphere fit, PLY/output
   * writes; per libdab handle stage: marshal (manager -> SoA arrays), setup
   * (dab_set_problem), update (values-only refresh), prep (a solve's table build and graph
   * capture), lm (the LM iterations), writeback, filter device pass, filter host compaction */
  double read_seconds, fit_seconds, write_seconds, marshal_seconds, setup_seconds, update_seconds, prep_seconds,
      lm_seconds, writeback_seconds, filter_device_seconds, filter_host_seconds;
} dam_pipeline_report;
int dam_run_pipeline_report(const char* input, const char* output, const char* ply_prefix, int32_t max_iteration,
                            int32_t max_second, double error_boundary, int32_t quiet, dam_pipeline_report* out);

#ifdef __cplusplus
}
#endif
#endif
