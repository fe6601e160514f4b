// DeepArcManager.hh — host-side scene container with the reference's public interface
// (src/DeepArcManager.hh): .deeparc reader/writer, PLY export, camera centres and
// filterPoint3d. The numeric work behind filterPoint3d (a residual per observation) runs
// on the GPU through libdab (dab_filter); the object-graph edits stay on the host, in
// the reference's order, so the surviving blocks and points are the reference's.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "Geometry.hh"
#include "ParameterBlock.hh"

struct DabSession;  // DabScene.hh: the manager's resident libdab problem (handle reuse)

class DeepArcManager {
 public:
  DeepArcManager() = default;
  ~DeepArcManager();
  DeepArcManager(const DeepArcManager&) = delete;
  DeepArcManager& operator=(const DeepArcManager&) = delete;

  bool isShareExtrinsic() { return share_extrinsic_; }
  // DeepArcManager.cc:26-74. Throws const char* when the file cannot be read.
  bool read(std::string filename);
  // DeepArcManager.cc:263-328 (cameras first, then points; default stream format).
  void writePly(std::string filename);
  std::vector<ParameterBlock*>* parameters() { return &params_; }
  std::vector<Point3d*>* point3ds() { return &point3d_; }
  // DeepArcManager.cc:332-424 (quirk Q4: drops observations with mse < error_boundary).
  void filterPoint3d(double error_boundary, double* hemisphere_center, double hemisphere_radius);
  // DeepArcManager.cc:426-499 (std::fixed, 6 decimals, angle-axis rotations; quirk Q7).
  void write(std::string filename);
  // DeepArcManager.cc:501-518: arc x ring camera centres (empty in non-shared mode, Q6).
  std::vector<std::vector<double> > getCameraCenter();

  // accessors the reference keeps private, needed by the solver adapter
  std::vector<Intrinsic*>* intrinsics() { return &intrinsics_; }
  std::vector<Extrinsic*>* extrinsics() { return &extrinsics_; }
  int arcSize() const { return arc_size_; }
  int ringSize() const { return ring_size_; }
  // One libdab handle per manager, kept across solve() / filterPoint3d() (the sfm.cc loop,
  // sfm.cc:104-129): the problem stays resident on the device while the manager's
  // structure is unchanged, so a filter after a solve, or a solve of unchanged structure,
  // only refreshes the parameter values. structureVersion() changes whenever read() or
  // filterPoint3d() change the blocks or points.
  DabSession& dabSession();
  unsigned long long structureVersion() const { return structure_version_; }
  // Robust loss of every solve() of this manager (dab_set_loss: DAB_LOSS_* and Ceres' scale
  // a). The reference passes NULL and keeps `//new ceres::CauchyLoss(0.5)` beside it
  // (sfm.cc:48-49); the default here is that NULL (DAB_LOSS_TRIVIAL). Checked when the solve
  // applies it to the handle. filterPoint3d keeps using the bare residual, as the reference's.
  void setLoss(int loss_type, double scale) {
    loss_type_ = loss_type;
    loss_scale_ = scale;
  }
  int lossType() const { return loss_type_; }
  double lossScale() const { return loss_scale_; }
  // Intrinsic groups every solve() of this manager refines (DAB_INTR_* bits of dab.h, one value
  // for every intrinsic): the equivalent of deleting sfm.cc:60-62. Kept across the pipeline's
  // re-set-ups beside the loss and applied after every dab_set_problem. The refined doubles go
  // back into the Intrinsic objects untruncated (Ceres writes through ParameterBlock::get()'s
  // pointers; quirk Q1's truncation is the reader's), so write() and the accessors see them.
  void setIntrinsicsFree(int groups) { intr_free_ = groups; }
  int intrinsicsFree() const { return intr_free_; }
  // sfm.cc:59, `//problem.SetParameterBlockConstant(parameter_block[0]); //freeze point3d`,
  // uncommented: every later solve() of this manager holds all points constant
  // (dab_set_points_constant with an all-ones mask; all or nothing, as that line is) and refines
  // the cameras alone. Kept across the pipeline's re-set-ups beside the loss and the intrinsic
  // groups and applied after every dab_set_problem.
  void setPointsConstant(bool all) { points_const_ = all; }
  bool pointsConstant() const { return points_const_; }
  // Gaussian priors on extrinsics for every later solve() of this manager (dab_set_ext_priors in
  // dab.h; Ceres: problem.AddResidualBlock(new NormalPrior(A, mu), NULL, ext)): index in
  // extrinsics(), mean [n][6] = (rotation, translation) as the Extrinsic stores them, sqrt_info
  // [n][6][6] row-major = A of the residual A (x - mean). Empty vectors clear them. Kept across
  // the pipeline's re-set-ups beside the loss, the groups and the point flag and applied after
  // every dab_set_problem; checked when the solve applies them to the handle. A prior on a
  // constant extrinsic (the gauge rule's, or all of them under freeze_camera) is ignored.
  void setExtrinsicPriors(const std::vector<int>& index, const std::vector<double>& mean,
                          const std::vector<double>& sqrt_info) {
    prior_index_ = index;
    prior_mean_ = mean;
    prior_sqrt_info_ = sqrt_info;
  }
  const std::vector<int>& extrinsicPriorIndex() const { return prior_index_; }
  const std::vector<double>& extrinsicPriorMean() const { return prior_mean_; }
  const std::vector<double>& extrinsicPriorSqrtInfo() const { return prior_sqrt_info_; }
  // Constant scalars of the extrinsics for every later solve() of this manager
  // (dab_set_ext_scalars_constant in dab.h: one of sfm.cc:51-52 kept, or a SubsetManifold): bits
  // indexed as extrinsics(), bit k = scalar k of (rotation, translation) is constant
  // (DAB_EXT_ROTATION 0x07, DAB_EXT_TRANSLATION 0x38); an empty vector clears it. Kept across the
  // pipeline's re-set-ups beside the loss and the other switches and applied after every
  // dab_set_problem. A length other than extrinsics()->size() or a byte above 63 throws and
  // leaves the setting as it was; bits on a constant extrinsic are ignored.
  void setExtrinsicScalarsConstant(const std::vector<uint8_t>& bits) {
    if (!bits.empty() && bits.size() != extrinsics()->size())
      throw "constant extrinsic scalars: one byte per extrinsic";
    for (uint8_t b : bits)
      if (b > 63) throw "constant extrinsic scalars: bits above 63";
    ext_scalars_const_ = bits;
  }
  const std::vector<uint8_t>& extrinsicScalarsConstant() const { return ext_scalars_const_; }
  // Gaussian priors on points for every later solve() of this manager (dab_set_point_priors in
  // dab.h; Ceres: problem.AddResidualBlock(new NormalPrior(A, mu), NULL, point)): ground-control
  // points. index into the manager's current point list (point3ds()), mean [n][3], sqrt_info
  // [n][3][3] row-major = A of the residual A (X - mean). Empty vectors clear them. Kept across
  // the pipeline's re-set-ups and applied after every dab_set_problem; checked when the solve
  // applies them to the handle. filterPoint3d renumbers them with the point list: a surviving
  // point keeps its prior under its new index, a removed point's prior goes with it. clear() (and
  // so read() of another scene) drops them: their indices name points of the scene they were set
  // on. Arrays whose lengths do not match index throw and leave the setting as it was.
  void setPointPriors(const std::vector<int>& index, const std::vector<double>& mean,
                      const std::vector<double>& sqrt_info) {
    if (mean.size() != 3 * index.size() || sqrt_info.size() != 9 * index.size())
      throw "point priors: mean needs 3 and sqrt_info 9 values per index";
    pt_prior_index_ = index;
    pt_prior_mean_ = mean;
    pt_prior_sqrt_info_ = sqrt_info;
  }
  const std::vector<int>& pointPriorIndex() const { return pt_prior_index_; }
  const std::vector<double>& pointPriorMean() const { return pt_prior_mean_; }
  const std::vector<double>& pointPriorSqrtInfo() const { return pt_prior_sqrt_info_; }
  // Gaussian priors on intrinsics for every later solve() of this manager (dab_set_intr_priors in
  // dab.h; Ceres: NormalPrior(A, mu) with a NULL loss over the intrinsic's blocks [1] [2] [3]): a
  // calibration with its covariance, for the groups setIntrinsicsFree frees. index in
  // intrinsics(), mean [n][6] = (cx, cy, f0, f1, k0, k1), sqrt_info [n][6][6] row-major = A of the
  // residual A (x - mean). Empty vectors clear them. Kept across the pipeline's re-set-ups beside
  // the other priors and applied after every dab_set_problem; checked when the solve applies them
  // to the handle. Slots the model lacks or the groups leave constant take no part, and without
  // free groups (or under freeze_camera) the priors are ignored. Arrays whose lengths do not match
  // index throw and leave the setting as it was.
  void setIntrinsicPriors(const std::vector<int>& index, const std::vector<double>& mean,
                          const std::vector<double>& sqrt_info) {
    if (mean.size() != 6 * index.size() || sqrt_info.size() != 36 * index.size())
      throw "intrinsic priors: mean needs 6 and sqrt_info 36 values per index";
    intr_prior_index_ = index;
    intr_prior_mean_ = mean;
    intr_prior_sqrt_info_ = sqrt_info;
  }
  const std::vector<int>& intrinsicPriorIndex() const { return intr_prior_index_; }
  const std::vector<double>& intrinsicPriorMean() const { return intr_prior_mean_; }
  const std::vector<double>& intrinsicPriorSqrtInfo() const { return intr_prior_sqrt_info_; }

  // Covariance of the current scene at its current parameters (dab_covariance in dab.h: Sigma =
  // (J^T J)^-1 under this manager's loss, no sigma^2 factor; ceres::Covariance). The reference's
  // gauge rule (only the (0,0) block's extrinsic constant, sfm.cc:50-53) leaves the rig's global
  // scale free, and the call then reports rank deficiency instead of numbers: name one more
  // extrinsic in extra_const to fix the scale. Its own handle: the resident problem of solve() /
  // filterPoint3d() is not touched.
  struct Covariance {
    bool ok = false;                // false: rank deficient (see status), the arrays are empty
    int status = 0;                 // DAB_COV_*
    int first_deficient_point = -1, deficient_points = 0;  // index in point3ds()
    double point_pivot_ratio_min = 0, camera_pivot_ratio = 0;
    double cost = 0;
    int num_residuals = 0, num_parameters = 0;
    std::vector<double> point_cov;  // [point3ds()->size()][6] upper-packed, point3ds() order (NaN: no block)
    std::vector<double> ext_cov;    // [free extrinsics][21] upper-packed
    std::vector<double> ext_full;   // [6 nfe][6 nfe] when asked for
    std::vector<int> ext_index;     // per row of ext_cov: index in extrinsics()
    std::vector<char> ext_kind;     // 'a' arc (or a plain extrinsic in non-shared mode) | 'r' ring
    std::vector<int> ext_position;  // arc or ring position of that extrinsic
    // covarianceIntrinsics only
    int num_free_scalars = 0;       // active intrinsic scalars (counted in num_parameters)
    std::vector<double> intr_cov;   // [free intrinsics][21] upper-packed, slots cx cy f0 f1 k0 k1
    std::vector<int> intr_index;    // per row of intr_cov: index in intrinsics()
    std::vector<double> cam_full;   // [6 nfe + 6 nfi] square when asked for: extrinsics, then intrinsics
  };
  Covariance covariance(const std::vector<int>& extra_const = {}, bool freeze_camera = false, bool full = false);
  // The same with the intrinsic groups of setIntrinsicsFree as unknowns (dab_covariance_intrinsics
  // in dab.h), under this manager's loss: covariance() would report them as exactly known and
  // understate every other variance. Inactive slots have zero rows and columns in intr_cov and
  // cam_full. With no group set it is covariance(extra_const, false, full), cam_full = ext_full.
  Covariance covarianceIntrinsics(const std::vector<int>& extra_const = {}, bool full = false);

 private:
  std::unique_ptr<DabSession> session_;
  unsigned long long structure_version_ = 0;
  int loss_type_ = 0;  // DAB_LOSS_TRIVIAL
  double loss_scale_ = 1.0;
  int intr_free_ = 0;  // all constant (sfm.cc:60-62)
  bool points_const_ = false;  // all free (sfm.cc:59 commented out)
  std::vector<uint8_t> ext_scalars_const_;  // none (every scalar of a free extrinsic is free)
  std::vector<int> prior_index_;  // extrinsic priors (none)
  std::vector<double> prior_mean_, prior_sqrt_info_;
  std::vector<int> pt_prior_index_;  // point priors (none), indices into point3d_
  std::vector<double> pt_prior_mean_, pt_prior_sqrt_info_;
  std::vector<int> intr_prior_index_;  // intrinsic priors (none), indices into intrinsics_
  std::vector<double> intr_prior_mean_, intr_prior_sqrt_info_;
  int arc_size_ = 0, ring_size_ = 0;
  bool share_extrinsic_ = false;
  std::map<int, std::map<int, Camera*> > hemisphere_;
  std::vector<Intrinsic*> intrinsics_;
  std::vector<Extrinsic*> extrinsics_;
  std::vector<Camera*> camera_;
  std::vector<ParameterBlock*> params_;
  std::vector<Point3d*> point3d_;

  void clear();
  Covariance covarianceOf(const std::vector<int>& extra_const, bool freeze_camera, bool full, bool with_intr);
  static int ringExtrinsicIndex(int ring_position, int arc_size) {
    return ring_position == 0 ? 0 : ring_position + arc_size - 1;
  }
  std::vector<double> cameraPosition(Extrinsic* e);
  std::vector<double> cameraPosition(Extrinsic* arc, Extrinsic* ring);
};
