// onnx_model.hpp -- in-memory form of the ONNX ModelProto subset the backend understands, and
// the protobuf wire decoder that fills it.
//
// Replaces what `tract_onnx::onnx().model_for_path(path)` does for the reference
// (engine.rs:49-51); the decoder is hand-written because neither libprotobuf headers for
// onnx.proto nor the `onnx` package exist in the build image.
#pragma once

#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace infera_hip::onnx {

enum DataType : int { kFloat = 1, kUint8 = 2, kInt8 = 3, kInt32 = 6, kInt64 = 7, kBool = 9, kFloat16 = 10, kDouble = 11 };

// IEEE binary16 <-> binary32 on the host: widening is exact (subnormals, infinities, NaN); narrowing rounds to nearest, ties to even,
// keeps subnormal halves, sends |x| >= 65520 to +-inf and a NaN to a quiet NaN of the same sign
inline float half_to_float(uint16_t h) {
  const uint32_t sign = uint32_t(h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, f = h & 0x3FFu;
  uint32_t u;
  if (e == 0x1F) u = sign | 0x7F800000u | (f << 13);
  else if (e != 0) u = sign | ((e + 112) << 23) | (f << 13);
  else if (f == 0) u = sign;
  else {  // a subnormal half: f * 2^-24, exact in f32
    float v = float(f) * 5.9604644775390625e-8f;
    std::memcpy(&u, &v, 4);
    u |= sign;
  }
  float out;
  std::memcpy(&out, &u, 4);
  return out;
}
inline uint16_t float_to_half(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  const uint16_t sign = uint16_t((u >> 16) & 0x8000u);
  const uint32_t a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return uint16_t(sign | 0x7E00u | ((a >> 13) & 0x3FFu));
  if (a >= 0x477FF000u) return uint16_t(sign | 0x7C00u);  // |x| >= 65520 (and inf)
  if (a < 0x38800000u) {  // below the smallest normal half: a multiple of 2^-24 after rounding
    float v;
    std::memcpy(&v, &a, 4);
    // adding 0.5 places the value so that the f32 addition rounds it (ties to even) to a multiple of 2^-24: the low mantissa bits are the half
    v += 0.5f;
    uint32_t w;
    std::memcpy(&w, &v, 4);
    return uint16_t(sign | (w - 0x3F000000u));
  }
  const uint32_t r = a + 0xFFFu + ((a >> 13) & 1u);  // ties to even on the 13 dropped bits (a carry moves into the exponent, as it should)
  return uint16_t(sign | ((r - 0x38000000u) >> 13));
}
inline float round_to_half(float x) { return half_to_float(float_to_half(x)); }

struct TensorData {
  std::string name;
  int dtype = 0;  // kFloat or kInt64 after decoding (uint8 / int8 / int32 / bool widened, double narrowed, float16 widened exactly)
  int elem = 0;   // the data_type as the file declares it (quantised graphs tell uint8, int8 and int32 apart; kFloat16: a half tensor, its f32 values are halves)
  std::vector<int64_t> dims;
  std::vector<float> f32;
  std::vector<int64_t> i64;
  std::vector<double> f64;  // kDouble payloads as read (f32 above holds them narrowed): load-time conversions that must round their own way
  // An f32 constant folded from DequantizeLinear(q_data, q_scale, q_zp) along q_axis (one scale: per tensor) remembers what it came from, so
  // a MatMul / Gemm that reads it can run on the integers (host/lowering.cpp, QDense)
  std::shared_ptr<const TensorData> q_data;
  std::vector<float> q_scale;
  std::vector<int64_t> q_zp;
  int64_t q_axis = 0;
  // Element count = payload length.  The decoder has verified it equals Π dims (overflow-checked), so a
  // declared shape can never claim more elements than the file holds.
  size_t count() const { return dtype == kInt64 ? i64.size() : f32.size(); }
};

struct Attribute {
  std::string name;
  int type = 0;  // AttributeProto.AttributeType: 1 FLOAT 2 INT 3 STRING 4 TENSOR 6 FLOATS 7 INTS 8 STRINGS
  float f = 0.f;
  int64_t i = 0;
  std::string s;
  std::vector<int64_t> ints;
  std::vector<float> floats;
  std::vector<std::string> strings;
  std::shared_ptr<TensorData> t;
};

struct NodeDef {
  std::string op, name, domain;
  std::vector<std::string> inputs, outputs;
  std::map<std::string, Attribute> attrs;

  int64_t attr_i(const std::string &k, int64_t dflt) const {
    auto it = attrs.find(k);
    return it == attrs.end() ? dflt : it->second.i;
  }
  float attr_f(const std::string &k, float dflt) const {
    auto it = attrs.find(k);
    return it == attrs.end() ? dflt : it->second.f;
  }
  std::string attr_s(const std::string &k, const std::string &dflt) const {
    auto it = attrs.find(k);
    return it == attrs.end() ? dflt : it->second.s;
  }
  const std::vector<int64_t> *attr_ints(const std::string &k) const {
    auto it = attrs.find(k);
    return it == attrs.end() ? nullptr : &it->second.ints;
  }
  const Attribute *attr(const std::string &k) const {
    auto it = attrs.find(k);
    return it == attrs.end() ? nullptr : &it->second;
  }
};

struct ValueDef {
  std::string name;
  int elem_type = 0;
  bool has_shape = false;
  std::vector<int64_t> dims;  // -1 = symbolic (dim_param) or unknown
};

struct Model {
  int64_t ir_version = 0;
  int64_t opset = 1;  // default-domain ("" / "ai.onnx") opset
  std::string producer, graph_name;
  std::vector<NodeDef> nodes;
  std::map<std::string, std::shared_ptr<TensorData>> initializers;
  std::vector<ValueDef> inputs;  // graph.input minus initializers
  std::vector<ValueDef> outputs;
};

// Throws InferaError::onnx(...) on I/O or wire-format problems.
Model parse_file(const std::string &path);
Model parse_bytes(const uint8_t *data, size_t len);

}  // namespace infera_hip::onnx
