// spatialnorm.cpp -- checks, parameter folds and the fused-unit rule of the SpatialNorm step (host/spatialnorm.hpp).
#include "spatialnorm.hpp"

#include <cmath>

namespace infera_hip {

SpatialNormUnit spatialnorm_fused_unit(int64_t C, int64_t S, int64_t G, bool cq) {
  const int64_t Cg = C / G, E = Cg * S;
  // (a [N,C,1,1] tensor is the same floats in either layout)
  if (!cq || S == 1 || Cg % 4 == 0) return E <= kSpatialNormFusedMaxE ? kSpatialUnitGroup : kSpatialUnitNone;
  if (Cg == 1 || Cg == 2) return 4 * S <= kSpatialNormFusedMaxE ? kSpatialUnitPlane : kSpatialUnitNone;
  return kSpatialUnitNone;  // groups that straddle quads
}

std::string spatialnorm_refusal(const std::vector<int64_t> &x_shape, int64_t groups, int64_t n_scale, int64_t n_bias, float eps) {
  const size_t rank = x_shape.size();
  if (rank != 3 && rank != 4) return "the input must be an [N,C,L] or [N,C,H,W] activation (rank 3 or 4), got rank " + std::to_string(rank);
  const int64_t C = x_shape[1];
  for (size_t i = 2; i < rank; i++)
    if (x_shape[i] <= 0) return "symbolic spatial extents (only the row axis may be symbolic)";
  if (C <= 0) return "a symbolic channel count";
  if (groups < 1 || C % groups != 0) return "num_groups = " + std::to_string(groups) + " does not divide C = " + std::to_string(C);
  if (n_scale != C || n_bias != C) return "scale / B must have C = " + std::to_string(C) + " entries (or num_groups under opset 18), got " + std::to_string(n_scale) + " and " + std::to_string(n_bias);
  int64_t E = C / groups;
  for (size_t i = 2; i < rank; i++) {
    if (x_shape[i] > kSpatialNormMaxE) return "spatial extent out of range";
    E *= x_shape[i];
    if (E > kSpatialNormMaxE) return "E = (C / groups) * H * W exceeds 2^24 elements per group (float(E) must be exact)";
  }
  if (!(eps >= 0.f) || !std::isfinite(eps)) return "epsilon must be a finite number >= 0";
  return "";
}

bool spatialnorm_per_channel(const std::vector<float> &v, int64_t C, int64_t G, bool allow_per_group, std::vector<float> *out) {
  if (int64_t(v.size()) == C) {
    *out = v;
    return true;
  }
  if (!allow_per_group || int64_t(v.size()) != G || G < 1 || C % G != 0) return false;
  out->resize(size_t(C));
  for (int64_t c = 0; c < C; c++) (*out)[size_t(c)] = v[size_t(c / (C / G))];
  return true;
}

void spatialnorm_fold_inner(const std::vector<float> &s, const std::vector<float> &b, const std::vector<float> &gamma, const std::vector<float> &beta,
                            int64_t C, std::vector<float> *scale, std::vector<float> *shift) {
  const int64_t Cg = C / int64_t(s.size());
  scale->resize(size_t(C));
  shift->resize(size_t(C));
  for (int64_t c = 0; c < C; c++) {
    const double g = gamma.empty() ? 1.0 : double(gamma[size_t(c)]), be = beta.empty() ? 0.0 : double(beta[size_t(c)]);
    (*scale)[size_t(c)] = float(double(s[size_t(c / Cg)]) * g);
    (*shift)[size_t(c)] = float(double(b[size_t(c / Cg)]) * g + be);
  }
}

}  // namespace infera_hip
