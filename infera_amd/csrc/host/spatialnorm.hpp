// spatialnorm.hpp -- InstanceNormalization / GroupNormalization as one step kind: what the lowering checks and
// folds, and which of the two plan shapes a layer gets once the scheduler knows the tensor's layout.
//   For row n and group k of G over the E = (C/G) * H * W elements of the group's channels, all f32:
//     mean = sum(x) / E;  d = x - mean;  resid = sum(d) / E;  d -= resid;  var = sum(d^2) / E;  y = act(d / sqrtf(var + eps) * gamma[c] + beta[c])
//   fused (one SpatialNorm step, in1 = -1): a work unit is held in the registers of its lanes, read once and written once;
//   general (SpatialStats -> SpatialNorm with in1 = the stats): [rows, G, 3] = (mean, resid, 1 / sqrtf(var + eps)), then
//     y = act(((x - mean) - resid) * inv * gamma[c] + beta[c]) -- a multiplication by inv where the fused form divides.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace infera_hip {

constexpr int64_t kSpatialNormFusedMaxE = 16384;          // floats of one fused work unit: 256 lanes x 16 quads
constexpr int64_t kSpatialNormMaxE = int64_t(1) << 24;    // elements per group: float(E) is exact up to here

// work units of the fused kernel
enum SpatialNormUnit : int {
  kSpatialUnitNone = -1,   // no fused form: the general plan
  kSpatialUnitGroup = 0,   // one group = one contiguous run of E floats (NCHW; channel quads with (C/G) % 4 == 0)
  kSpatialUnitPlane = 1,   // one quad plane [S][4] holding 4 groups (C/G = 1) or 2 groups of 2 channels: one set of sums per component
};
// the unit of a layer of C channels in G groups over S = H * W positions on an NCHW (cq = false) or channel-quad tensor
SpatialNormUnit spatialnorm_fused_unit(int64_t C, int64_t S, int64_t G, bool cq);

// why a layer cannot be served ("" = it can): x_shape = the ONNX shape [N, C, ...], n_scale / n_bias = the parameter lengths AFTER the
// opset-18 broadcast (both C)
std::string spatialnorm_refusal(const std::vector<int64_t> &x_shape, int64_t groups, int64_t n_scale, int64_t n_bias, float eps);

// scale / bias of `len` entries as per-channel vectors: len == C as they are, len == G (GroupNormalization-18) each repeated over its
// group's channels.  false: neither length
bool spatialnorm_per_channel(const std::vector<float> &v, int64_t C, int64_t G, bool allow_per_group, std::vector<float> *out);

// the exporter's spelling: InstanceNormalization(scale s[G], B b[G]) inside, Mul(gamma[C]) / Add(beta[C]) outside (either may be absent:
// empty) -> gamma'[c] = s_g gamma[c], beta'[c] = b_g gamma[c] + beta[c], in f64, each rounded once
void spatialnorm_fold_inner(const std::vector<float> &s, const std::vector<float> &b, const std::vector<float> &gamma, const std::vector<float> &beta,
                            int64_t C, std::vector<float> *scale, std::vector<float> *shift);

}  // namespace infera_hip
