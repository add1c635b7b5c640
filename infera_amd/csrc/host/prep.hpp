// prep.hpp -- ai.onnx.ml preprocessing (Imputer, Scaler, Binarizer, OneHotEncoder, LabelEncoder, FeatureVectorizer, ArrayFeatureExtractor,
// integer inputs): the symbolic per-output-column program lowering builds for a preprocessing region, the node validation, and the packed
// tables hip/prep.hip runs on.  Semantics: INTEGRATION.md section 2.6 ("Preprocessing"); kernel design: the hip/prep.hip header.
#pragma once

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "onnx_model.hpp"

namespace infera_hip {

// caps (each rejected at load with its own message)
constexpr int64_t kPrepMaxSource = 4096;           // columns of the buffer a Prep step reads
constexpr int64_t kPrepMaxOut = 8192;              // output columns of one Prep step
constexpr int64_t kPrepMaxCats = 65536;            // one-hot categories, all OneHotEncoder nodes together
constexpr int64_t kPrepMaxKeys = int64_t(1) << 20; // LabelEncoder keys, all nodes together
constexpr int64_t kPrepMaxExact = int64_t(1) << 24; // |integer| an f32 holds exactly
constexpr int64_t kPrepStageBytes = 32768;         // input tile staged in LDS per block (R rows of F_in floats)
constexpr int64_t kPrepMaxTileOut = 65536;         // output elements per block tile

// the last operation of a column (descriptor bits 16..17)
enum PrepFinal : uint32_t { kPrepNone = 0, kPrepBin = 1, kPrepOneHot = 2, kPrepLookup = 3 };
// descriptor word 0: bits 0..15 source column, 16..17 PrepFinal, then these flags, bits 27..31 the strict OneHotEncoder (1-based)
constexpr uint32_t kPrepKindShift = 16, kPrepTrunc = 1u << 20, kPrepImpute = 1u << 21, kPrepImputeNan = 1u << 22, kPrepAffine = 1u << 23,
                   kPrepStrict = 1u << 24, kPrepIntKey = 1u << 25, kPrepNanKey = 1u << 26, kPrepStrictShift = 27;
constexpr int kPrepMaxStrictIds = 31;

// A sorted key -> value table: a LabelEncoder's mapping, or (strict one-hot check) the categories of a zeros = 0 OneHotEncoder.
struct PrepTable {
  std::vector<float> keys, vals;  // ascending keys (no NaN, no duplicates; -0 is 0)
  bool int_keys = false;          // keys match trunc(x)
  bool has_nan = false;           // a NaN key (float keys only) maps NaN inputs to nan_val
  float nan_val = 0.f;
  float dflt = 0.f;               // a LabelEncoder's value for a miss
};

// One output column as lowering composes it: source column -> [trunc] -> [impute] -> [affine] -> [binarize | one-hot test | lookup].
struct PrepCol {
  int64_t src = 0;
  bool trunc = false, impute = false, imp_nan = false, affine = false;
  float repl = 0.f, imp = 0.f, off = 0.f, scale = 1.f;
  uint32_t kind = kPrepNone;
  float c = 0.f;      // Binarizer threshold / one-hot category / lookup default value
  int table = -1;     // lookup: its table; one-hot: the strict check's table (the first column of an input column's group only)
  int strict = 0;     // 1-based id of the zeros = 0 OneHotEncoder the strict check reports
  bool is_int = false;  // whole-valued by construction (an integer Cast behind it is a no-op)
  int stage() const { return kind != kPrepNone ? 4 : affine ? 3 : impute ? 2 : trunc ? 1 : 0; }
  bool plain() const { return stage() == 0; }
};

struct PrepError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// node validation (throw PrepError with the reason)
struct ImputerSpec {
  std::vector<float> imputed;  // 1 or F values
  float replaced = 0.f;
};
ImputerSpec parse_imputer(const onnx::NodeDef &n, int64_t F);
float parse_binarizer(const onnx::NodeDef &n);
struct OneHotSpec {
  std::vector<float> cats;  // in attribute order (output column order)
  bool zeros = true;
};
OneHotSpec parse_onehot(const onnx::NodeDef &n);
PrepTable parse_label_encoder(const onnx::NodeDef &n, bool *int_values);
// the sorted table of a strict one-hot check
PrepTable onehot_table(const std::vector<float> &cats);

// The device form of one Prep step.  desc: 4 words per output column {word 0, table offset (pairs), c bits, table count}; cst: 4 floats
// per output column {replaced, imputed, offset, scale}; tab: (key, value) pairs, each table's NaN-key pair after its sorted pairs.
struct PrepPack {
  std::vector<uint32_t> desc;
  std::vector<float> cst, tab;
  int64_t F_in = 0, F = 0, R = 1, onehot = 0, lookup = 0;  // R: rows per block tile
  bool strict = false;  // a zeros = 0 OneHotEncoder sets the call's failure word
};
PrepPack pack_prep(const std::vector<PrepCol> &cols, const std::vector<std::shared_ptr<PrepTable>> &tables, int64_t F_in);

}  // namespace infera_hip
