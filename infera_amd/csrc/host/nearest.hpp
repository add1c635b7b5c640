// nearest.hpp -- squared Euclidean distances of each row to a constant reference set (KMeans, nearest centroid, k-NN search): load-time
// validation and the packed tables hip/nearest.hip runs on.  Semantics: INTEGRATION.md section 2.6; kernel design: the hip/nearest.hip header.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace infera_hip {

// caps (each rejected at load with its own message)
constexpr int64_t kNearestMaxF = 1024;                   // input width
constexpr int64_t kNearestMaxM = int64_t(1) << 20;       // reference vectors
constexpr int64_t kNearestMaxValues = int64_t(1) << 28;  // M * F (1 GB of f32 reference vectors)
constexpr int64_t kNearestMaxK = 16;                     // neighbours kept per row (also the TopK step's cap)
// reference tiles of 32 (one MFMA tile), cut into slices fixed by the model alone: at most kNearestTargetSlices slices of at least
// kNearestMinSliceTiles tiles (a slice stages its row tile once: short slices would only re-read the rows)
constexpr int64_t kNearestTile = 32, kNearestTargetSlices = 16, kNearestMinSliceTiles = 8;

// the width of the running best list that serves k neighbours (the kernels are instantiated for 1 and 16)
inline int nearest_list_width(int64_t k) { return k <= 1 ? 1 : 16; }

struct NearestError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// Nearest / NearestReduce output modes (Step::out_mode)
enum NearestOut : int {
  kNearestSelect = 0,   // Nearest: the per-slice best-k lists [rows][slices][k] of (value, index bits)
  kNearestMatrix = 1,   // Nearest: d2 [rows, M]
  kNearestMatrixSqrt = 2,  // Nearest: sqrt(d2) [rows, M]
  kNearestLabel = 3,    // NearestReduce: index of the nearest vector [rows]
  kNearestIndices = 4,  // NearestReduce: the k nearest, ascending distance [rows, k]
  kNearestValues = 5,   // NearestReduce: their d2 [rows, k]
  kNearestValuesSqrt = 6,
};

struct NearestPack {
  // [tiles][F_pad / 8][64 lanes][4]: lane (r, h), element j of k-group g holds (C - mu)[32 t + r][8 g + 4 h + j], the MFMA A-fragment
  // order of nearest.hip (the svm.hip / dense.hip k permutation); padding vectors and features are 0
  std::vector<float> ref;
  std::vector<float> ref_norm;  // |c - mu|^2 per padded vector [tiles * 32] (f64 sum of the rounded differences, rounded once)
  std::vector<float> center;    // mu: the mean of the reference vectors [F_pad] (f64 sum, rounded once)
  std::vector<uint32_t> slice_tile;  // first tile per slice (slices + 1)
  int64_t F = 0, F_pad = 0, M = 0, tiles = 0, slices = 1;
  std::string spelling;  // "gemm", "matmul_mul" or "cdist"
};

// Packs the reference set C [M, F] (row-major).  Throws NearestError with the reason when a cap is exceeded.
NearestPack pack_nearest(const float *C, int64_t M, int64_t F, const std::string &spelling);

// ---- the k-NN vote (KNeighborsClassifier / KNeighborsRegressor; definition: INTEGRATION.md section 2.6 "The k-NN vote") ----
// NearestVote output modes (Step::out_mode)
enum VoteOut : int {
  kVoteLabel = 0,  // class_value of the first maximum of the class totals [rows]
  kVoteProba = 1,  // the class totals over their sum [rows, C]
  kVoteValue = 2,  // the (weighted) mean of the neighbours' targets [rows, 1]
};
// Probability rows leave a wave through LDS, 64 rows x C floats at a time within the kernel's 64 KB: C <= 256 (rejected above it at
// load).  The label and the regression value are tallied in registers and have no class cap.
constexpr int64_t kVoteMaxProbaClasses = 256;
constexpr float kVoteMaxClassValue = 16777216.f;  // 2^24: labels are served as f32 values

struct VotePack {
  std::vector<int32_t> cls;        // class index of each reference vector [M] (classifier)
  std::vector<float> target;       // target of each reference vector [M] (regressor)
  std::vector<float> class_value;  // the served label of each class [C]
  int64_t classes = 0;
  float eps = 0.f;        // w = 1 / max(d, eps) (weighted)
  bool weighted = false;  // distance weights (else uniform)
  bool rooted = false;    // d = sqrt(d2) (else d2)
};

}  // namespace infera_hip
