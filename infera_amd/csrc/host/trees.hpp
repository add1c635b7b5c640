// trees.hpp -- ai.onnx.ml TreeEnsembleRegressor / TreeEnsembleClassifier (opsets 1 and 3): load-time validation and the
// packed tables hip/trees.hip walks.  Semantics: INTEGRATION.md section 2.6.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "onnx_model.hpp"

namespace infera_hip {

// ---- packed node record: two 32-bit words, {threshold bits, meta} ------------------------------------------------------------
// The six ONNX modes are normalised to three compares (children swapped where needed); the left child is taken when the compare
// holds, the right one otherwise, and a NaN feature goes where kTreeNanRight says (decided from the ORIGINAL mode and
// nodes_missing_value_tracks_true before the swap).  Children of a node are adjacent: left = this + delta, right = left + 1.
//   internal: meta = kind << 30 | nan_right << 29 | feature << 17 | delta        (kind 0: x <= t, 1: x < t, 2: x == t)
//   leaf:     meta = 3 << 30 | leaf row (walk width > 1: row of the leaf table);  walk width 1: the leaf value is the threshold word
constexpr uint32_t kTreeLeaf = 3u;
constexpr uint32_t kTreeNanRight = 1u << 29;
constexpr int kTreeFeatureShift = 17;
constexpr uint32_t kTreeDeltaMask = (1u << 17) - 1;
constexpr uint32_t kTreeLeafRowMask = (1u << 29) - 1;

// caps (each rejected at load with its own message)
constexpr int64_t kTreeMaxFeature = 4096;              // feature ids below this (12 bits of the record)
constexpr int64_t kTreeMaxNodesPerTree = 131071;       // child offsets stay below 2^17
constexpr int64_t kTreeMaxNodes = int64_t(1) << 26;    // all trees together (512 MB of records)
constexpr int64_t kTreeMaxTargets = 1024;              // E: n_targets or the number of classes
constexpr int64_t kTreeMaxLeafFloats = int64_t(1) << 28;  // leaf table (1 GB)
// trees are cut into slices fixed by the ensemble alone: ceil(trees / 8) of them, at most 16 (results never depend on the call)
constexpr int64_t kTreeSliceTrees = 8, kTreeMaxSlices = 16;

struct TreeError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

struct TreePack {
  std::vector<uint32_t> tab;  // records (2 words per node) | root record per tree | first tree per slice (slices + 1)
  std::vector<float> leaves;  // [leaf rows][W] (W > 1 only)
  std::vector<float> base;    // W values or empty
  std::vector<float> labels;  // classifier: classlabels_int64s as f32 values
  int64_t trees = 0, nodes = 0, max_depth = 0, slices = 1;
  int64_t W = 1;  // columns accumulated per row: E, or 1 for the binary single-column form
  int64_t E = 1;  // scores per row served
  bool classifier = false, binary = false;
  bool is_signed = false;  // binary form with a negative weight ([-s, s], label s > 0)
  bool average = false;    // AVERAGE aggregation
};

// f32 threshold with the same decision as comparing an f32 x against the double d: mode 0 (<=, >) rounds toward -inf, 1 (<, >=)
// toward +inf; 2 (==, !=): d itself, or NaN when d has no exact f32 value (== never holds, != always does)
float tree_threshold_f32(double d, int dir);

// Validates node `n` (input [rows, F]) and packs it.  Throws TreeError with the reason.
TreePack pack_tree_ensemble(const onnx::NodeDef &n, int64_t F);

}  // namespace infera_hip
