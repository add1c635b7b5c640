// svm.hpp -- ai.onnx.ml SVMClassifier / SVMRegressor: load-time validation and the packed tables hip/svm.hip runs on.
// Semantics: INTEGRATION.md section 2.6; kernel design: the hip/svm.hip header.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "onnx_model.hpp"

namespace infera_hip {

// caps (each rejected at load with its own message)
constexpr int64_t kSvmMaxF = 1024;                   // input width
constexpr int64_t kSvmMaxSupport = 262144;           // support vectors
constexpr int64_t kSvmMaxValues = int64_t(1) << 28;  // n_SV * F (1 GB of f32 support vectors)
constexpr int64_t kSvmMaxClasses = 64;               // C
constexpr int64_t kSvmMaxProbClasses = 16;           // C with prob_a / prob_b (the pairwise coupling solve is C x C per row)
constexpr int64_t kSvmMaxDegree = 16;                // POLY degree
// SV tiles of 32 (one MFMA tile), padded per class; cut into slices fixed by the model alone: at most ~16 + C slices of at
// least kSvmMinSliceTiles tiles, each inside one class
constexpr int64_t kSvmTile = 32, kSvmTargetSlices = 16, kSvmMinSliceTiles = 2;
// stage 2: a VALU dot product for up to kSvmValuMaxQ coefficient rows, a second MFMA (32 rows per tile) above that
constexpr int64_t kSvmValuMaxQ = 8;

struct SvmError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

struct SvmPack {
  // [tiles][F_pad / 8][64 lanes][4]: lane (r, h), element j of k-group g holds S[32 t + r][8 g + 4 h + j] (centered for RBF), the
  // MFMA A-fragment order of svm.hip; padding SVs and features are 0
  std::vector<float> sv;
  std::vector<float> sv_norm;  // RBF: |s - center|^2 per padded SV [tiles * 32]
  std::vector<float> center;   // RBF: mean of the support vectors [F_pad]
  // stage-2 coefficients.  QW <= 8: [tiles][2 halves][16 registers][QW];  else [tiles][QW / 32][4][64 lanes][4] (MFMA A fragments).
  // Entry (register i, half h) belongs to SV 32 t + 8 (i >> 2) + 4 h + (i & 3), the stage-1 accumulator layout.
  std::vector<float> coef;
  std::vector<uint32_t> slice_tile;   // first tile per slice (slices + 1)
  std::vector<uint32_t> class_slice;  // first slice per class (classes + 1)
  std::vector<float> rho, prob_a, prob_b, labels;
  int kernel = 0, degree = 1;
  float gamma = 0.f, coef0 = 0.f;
  int64_t F = 0, F_pad = 0, n_sv = 0, tiles = 0, slices = 1;
  int64_t classes = 1;  // C (regressor: 1)
  int64_t Q = 1;        // coefficient rows per SV: C - 1, or 1 for the regressor
  int64_t QW = 1;       // stage-2 width: 1, 2, 4, 8 (VALU) or a multiple of 32 (MFMA)
  bool classifier = false, one_class = false;
  bool probabilities = false;  // the model has prob_a / prob_b
};

// Validates node `n` (input [rows, F]) and packs it.  Throws SvmError with the reason.
SvmPack pack_svm(const onnx::NodeDef &n, int64_t F);

}  // namespace infera_hip
