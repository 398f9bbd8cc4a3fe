// ar_slam_solver.hpp -- C++ host mirror of ar_slam's ArSlamSolver
// (ar_slam/include/ar_slam/ar_slam_util.hpp:361-497) with the MI355X solver
// behind it: the same data store (captures, arucos, blocks, handles, uid
// maps), the same incremental / BFS / localize drivers and initialisers, the
// same YAML map format, and ceres::Problem replaced by the C-ABI of
// include/arslam_lm.h (pointer-keyed residual blocks) and the batched
// localizer of include/arslam_localize.h.
//
// Not mirrored (out of scope): image loading / ArUco
// detection (loadImages, needs OpenCV), the debug display, ROS message types
// (Detections / TransformStamped / CameraInfo are plain structs here).
#pragma once

#include "arslam_lm.h"
#include "arslam_localize.h"

#include <array>
#include <cstdint>
#include <deque>
#include <memory>
#include <optional>
#include <ostream>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace arslam {

struct Point {   // ar_slam_util.hpp:56-63
  double x = 0.0;
  double y = 0.0;
};

struct ImageSize {
  int width = 0;
  int height = 0;
  bool operator==(const ImageSize &o) const { return width == o.width && height == o.height; }
  bool operator!=(const ImageSize &o) const { return !(*this == o); }
};

struct CameraParams {   // :66-78
  std::array<double, 3> params{3000.0, 0.0, 0.0};   // focal, l1, l2 (non-zero initial focal)
  std::optional<ImageSize> size;
};

struct PoseParams {   // :81-94 -- translation then angle-axis
  std::array<double, 6> params{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
};

struct CaptureHandle {
  unsigned idx = ~0u;
  bool operator==(const CaptureHandle &o) const { return idx == o.idx; }
};
struct CaptureHandleHash {   // std::hash<CaptureHandle>, ar_slam_util.hpp:140-145
  size_t operator()(const CaptureHandle &h) const { return h.idx; }
};
struct ArucoHandle { unsigned idx = ~0u; };
struct BlockHandle { unsigned idx = ~0u; };

struct ArucoRect {   // :265-293, centred pixel coordinates, TL TR BR BL
  std::array<Point, 4> corners;
};

struct Capture {   // :196-227
  std::string uid;
  CaptureHandle handle;
  std::string img_fn;
  std::vector<BlockHandle> blocks;
  std::optional<BlockHandle> init_block;
  PoseParams inv_pose;
  double *data() { return inv_pose.params.data(); }
  const double *data() const { return inv_pose.params.data(); }
};

struct Aruco {   // :229-240
  std::string id;
  ArucoHandle handle;
  bool initialized = false;
  std::vector<BlockHandle> blocks;
  PoseParams pose;
  double *data() { return pose.params.data(); }
  const double *data() const { return pose.params.data(); }
  // the tag's side in metres (the reference's one aruco_size, ar_slam_util.hpp:319,
  // per tag): setArucoSize / setDefaultArucoSize, the map file's optional key
  double size = ARSLAM_DEFAULT_TAG_SIZE;
};

struct Block {   // :296-315
  BlockHandle handle;
  ArucoRect aruco_rect;
  CaptureHandle capture;
  ArucoHandle aruco;
  bool added = false;
};

// ar_slam_interfaces/msg/Detection(s).msg without the ROS header and image
struct Detection {
  std::array<Point, 4> corners;
  std::string id;
};
struct Detections {
  std::string capture_uid;
  uint32_t image_height = 0;
  uint32_t image_width = 0;
  std::string image_path;
  std::vector<Detection> detections;
};

// geometry_msgs/TransformStamped subset (getTransforms, :1028-1075)
struct Transform {
  std::string frame_id, child_frame_id;
  double translation[3];
  double rotation[4];   // w, x, y, z
};

// sensor_msgs/CameraInfo subset (getCameraInfo, :1077-1110)
struct CameraInfo {
  uint32_t width = 0, height = 0;
  std::string distortion_model;
  std::array<double, 5> d{};
  std::array<double, 9> k{}, r{};
  std::array<double, 12> p{};
};

// Ceres summary of the last optimize() (the reference prints progress only)
struct SolveRecord {
  std::string capture_uid;
  unsigned capture_idx = ~0u;
  arslam_lm_summary summary;
};

class ArSlamSolver {
 public:
  explicit ArSlamSolver(const arslam_lm_options *opt = nullptr);
  ~ArSlamSolver();
  ArSlamSolver(const ArSlamSolver &) = delete;
  ArSlamSolver &operator=(const ArSlamSolver &) = delete;

  void loadYaml(const std::string &fn);                 // :304-384
  void loadYamlString(const std::string &text);
  void saveYaml(std::ostream &output) const;            // :387-465

  void solve();                                         // BFS from the best capture, :744-866
  void solveIncremental();                              // :629-678
  void localizeMany(unsigned first_loc_cap_idx);        // :888-901 (batched on the device)

  std::string genUniqueCaptureUid() const;              // :286-300
  unsigned getNextCaptureIndex() const { return (unsigned)captures_.size(); }

  std::optional<CaptureHandle> addDetections(const Detections &detections);   // :591-627
  std::vector<Transform> getTransforms() const;         // :1028-1075
  CameraInfo getCameraInfo() const;                     // :1077-1110

  Capture &at(CaptureHandle h) { return captures_.at(h.idx); }
  const Capture &at(CaptureHandle h) const { return captures_.at(h.idx); }
  Aruco &at(ArucoHandle h) { return arucos_.at(h.idx); }
  const Aruco &at(ArucoHandle h) const { return arucos_.at(h.idx); }
  Block &at(BlockHandle h) { return blocks_.at(h.idx); }
  const Block &at(BlockHandle h) const { return blocks_.at(h.idx); }

  size_t numCaptures() const { return captures_.size(); }
  size_t numArucos() const { return arucos_.size(); }
  size_t numBlocks() const { return blocks_.size(); }
  CameraParams &camera() { return camera_; }
  const CameraParams &camera() const { return camera_; }
  std::optional<CaptureHandle> findCapture(const std::string &uid) const;
  std::optional<ArucoHandle> findAruco(const std::string &id) const;
  const std::deque<SolveRecord> &solveLog() const { return solve_log_; }
  const std::unordered_set<CaptureHandle, CaptureHandleHash> &unsolvedCaptures() const { return unsolved_captures_; }
  void setVerbose(bool v) { verbose_ = v; }
  // The ceres::LossFunction of the residual blocks added from now on (the
  // reference passes nullptr, ar_slam_util.cpp:720-727): arslam_lm_set_loss on
  // the problem, so it holds for solve, solveIncremental and solveCapture.
  // localizeMany's batched kernel takes its own loss, setLocalizeLoss.  Returns
  // ARSLAM_OK or ARSLAM_E_INVALID_ARG (the loss is then unchanged).
  int setLoss(int kind, double a);
  // The ceres::LossFunction of every residual block localizeMany adds (the
  // reference passes nullptr, ar_slam_util.cpp:956-963): localizeMany then
  // runs through arslam_localize_many_loss.  Same return values as setLoss.
  int setLocalizeLoss(int kind, double a);
  // Tag sides in metres.  The default holds for the tags created afterwards
  // (by addDetections or loadYaml without the key).  setArucoSize names a tag
  // by its id string and may precede the tag's first detection; once the tag
  // is initialised or a residual block of it has been added its side is bound:
  // ARSLAM_E_STATE.  A side that is not finite or not > 0: ARSLAM_E_INVALID_ARG.
  // The sides reach the residual blocks (arslam_lm_add_residual_block_sized),
  // the initialisers and localizeMany's batch.
  int setDefaultArucoSize(double size);
  int setArucoSize(const std::string &id, double size);
  // The camera model (ARSLAM_CAMERA_*, PINHOLE initially) of the mapper handle
  // and of localizeMany's localizer; under RADIAL camera l1, l2 are a known
  // calibration the solves hold.  Once a residual block has been added the
  // model is bound: ARSLAM_E_STATE.  An unknown value: ARSLAM_E_INVALID_ARG.
  // The initialisers stay the pinhole's (they only seed the LM).  The map file
  // keeps it as `model: radial` inside `camera:`, written only under RADIAL.
  int setCameraModel(int model);
  int cameraModel() const { return camera_model_; }
  // the plumb_bob vector beside getCameraInfo's K and P: [l1, l2, 0, 0, 0]
  // under RADIAL, zeros under PINHOLE
  void cameraDistortion(double d[5]) const;
  // The 6x6 covariance (arslam_localizer_covariance: row-major, [t_c, w_c],
  // unit-variance residuals) and its ARSLAM_COV_* status of a capture the last
  // localizeMany localized, at the pose it was given -- ceres::Covariance on
  // the capture block after localizeOne's Solve.  localizeMany keeps its
  // batch on the device; the covariances of all its captures are computed by
  // the first request after it.  Returns ARSLAM_OK, or ARSLAM_E_STATE for a
  // capture the last localizeMany did not cover.  cov and cov_status nullable.
  int localizeCovariance(unsigned cap_idx, double cov[36], int *cov_status);
  // ceres::Problem::Evaluate on the mapper problem at the current poses
  // (arslam_lm_evaluate_blocks): *cost = 1/2 sum rho over the residual blocks
  // in the problem; per block of the data store (numBlocks entries, block
  // handle order) its |r|^2 and its loss weight rho' under the loss it was
  // added with, -1 in both for a block that is not in the problem (not yet
  // added, or localized by localizeMany, which adds none).  All nullable.
  // Returns arslam_lm_evaluate_blocks' code (ARSLAM_E_STATE: no block added yet).
  int evaluate(double *cost, double *sq_norm, double *weight);
  // The mapper problem's covariance in the gauge of one aruco (the reference
  // holds no block constant): SetParameterBlockConstant(anchor) +
  // ceres::Covariance::Compute over every block, without touching the problem
  // (arslam_lm_covariance_block_anchored, which works under the mixed e-block
  // set the solves run).  Valid after solve() or solveIncremental().
  // covariance() computes and keeps the 6x6 block of every capture and aruco
  // and the camera's 3x3; the getters serve the kept result.  anchor_aruco must
  // be an aruco with residual blocks in the problem: else ARSLAM_E_INVALID_ARG.
  // A capture or aruco that is not in the problem (not yet added, or localized
  // by localizeMany) is ARSLAM_COV_UNAVAILABLE, -1 in its values, as is the
  // anchor itself.  Whatever changes the problem or its values (addDetections,
  // a solve, localizeMany, a loss, the camera model, a map file, the pose
  // setters: dropCovariance) drops the kept result; the getters then return
  // ARSLAM_E_STATE.  covariancePair: block (a, b) in that gauge, kinds
  // ARSLAM_BLOCK_CAMERA (index 0), _CAPTURE, _TAG (an aruco), 36 values as
  // arslam_lm_covariance_pairs_anchored lays them out; computes on every call.
  int covariance(int anchor_aruco, arslam_lm_cov_info *info);
  int arucoCovariance(int a, double cov[36], int *status) const;
  int captureCovariance(int c, double cov[36], int *status) const;
  int cameraCovariance(double cov[9], int *status) const;
  int covariancePair(int anchor_aruco, int kind_a, int idx_a, int kind_b, int idx_b, double cov[36], int *status);
  void dropCovariance() { cov_valid_ = false; }

  // data-store builders (protected in the reference; public here so a host
  // or test can assemble a problem without ROS messages)
  Capture &addCapture(const std::string &cap_uid, const std::string &fn);   // :419-428
  Aruco &addAruco(const std::string &ar_id);                               // :430-436
  Aruco &getOrAddAruco(const std::string &ar_id);                          // :438-445
  Block &addBlock(const ArucoRect &rect, CaptureHandle cap, ArucoHandle ar);   // :447-457

 protected:
  void localizeOne(Capture &capture, unsigned first_loc_cap_idx);
  void addConnectedCaptures(const Capture &base, std::deque<CaptureHandle> &open);   // :868-886
  void solveCapture(Capture &capture, std::optional<BlockHandle> init_block);    // :680-742
  void addCaptureBlocks(Capture &capture);
  void optimize(const Capture &capture);                                         // :1001-1018
  void resetProblem();                                                           // :1021-1025

  arslam_lm_options options_;
  arslam_lm *problem_ = nullptr;   // was: ceres::Problem problem_ (:473)
  CameraParams camera_;
  std::deque<Capture> captures_;   // stable addresses: the solver keys blocks by pointer
  std::deque<Aruco> arucos_;
  std::vector<Block> blocks_;
  std::vector<unsigned> problem_blocks_;   // the blocks in problem_, in the order they were added (evaluate)
  std::unordered_map<std::string, unsigned> capture_map_;
  std::unordered_map<std::string, unsigned> aruco_map_;
  // the reference's container and hash (ar_slam_util.hpp:140-145, 492): solveIncremental
  // visits the unsolved captures in its iteration (bucket) order
  std::unordered_set<CaptureHandle, CaptureHandleHash> unsolved_captures_;
  std::deque<SolveRecord> solve_log_;   // (records are ~90 KB: no reallocation copies)
  bool verbose_ = false;
  int localize_loss_kind_ = ARSLAM_LOSS_NONE;   // setLocalizeLoss
  double localize_loss_a_ = 0.0;
  double default_aruco_size_ = ARSLAM_DEFAULT_TAG_SIZE;
  int camera_model_ = ARSLAM_CAMERA_PINHOLE;   // setCameraModel
  std::unordered_map<std::string, double> aruco_size_by_id_;   // setArucoSize before the tag exists
  // the last localizeMany: its resident batch, the captures it covered
  // (loc_first_ + q is query q) and their covariances once asked for
  void dropLocalizer();
  arslam_localizer *localizer_ = nullptr;
  unsigned loc_first_ = 0, loc_count_ = 0;
  std::vector<double> loc_cov_;
  std::vector<int> loc_cov_status_;
  // covariance(): the kept result, by capture and aruco index
  bool cov_valid_ = false;
  std::vector<double> cov_cap_, cov_aruco_;
  std::vector<int> cov_cap_status_, cov_aruco_status_;
  double cov_cam_[9] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};
  int cov_cam_status_ = ARSLAM_COV_UNAVAILABLE;
  // the captures and arucos with residual blocks in problem_ (1 per index)
  void problemMembers(std::vector<char> &caps, std::vector<char> &arucos) const;
};

// initialisers (ar_slam_util.cpp:41-128)
void composeAxisAngle(const double *rot1, const double *rot2, double *out);
// (aruco_size: the side of the tag the rectangle shows; the depth is proportional to it)
void calcInitValues(const ArucoRect &rect, double focal, double out[4], double aruco_size = ARSLAM_DEFAULT_TAG_SIZE);
void initCapturePose(const ArucoRect &rect, const double *camera, const double *ar_pose, double *inv_cap_pose,
                     double aruco_size = ARSLAM_DEFAULT_TAG_SIZE);
void initArPose(const ArucoRect &rect, const double *camera, const double *inv_cap_pose, double *ar_pose,
                double aruco_size = ARSLAM_DEFAULT_TAG_SIZE);

}  // namespace arslam
