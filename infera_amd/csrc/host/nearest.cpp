// nearest.cpp -- the reference set of a distance model: caps, the load-time center, fragment-order tiles, slices.
#include "nearest.hpp"

#include <algorithm>

namespace infera_hip {

namespace {
[[noreturn]] void fail(const std::string &why) { throw NearestError("unsupported operator form: " + why); }
std::string num(int64_t v) { return std::to_string(v); }
}  // namespace

NearestPack pack_nearest(const float *C, int64_t M, int64_t F, const std::string &spelling) {
  if (F < 1 || M < 1) fail("an empty reference set");
  if (F > kNearestMaxF) fail("input width " + num(F) + " is above the cap of " + num(kNearestMaxF));
  if (M > kNearestMaxM) fail("M = " + num(M) + " reference vectors, above the cap of " + num(kNearestMaxM));
  if (M * F > kNearestMaxValues) fail("M x F = " + num(M * F) + " values, above the cap of " + num(kNearestMaxValues));
  NearestPack p;
  p.F = F;
  p.M = M;
  p.spelling = spelling;
  p.F_pad = (F + 7) / 8 * 8;
  p.tiles = (M + kNearestTile - 1) / kNearestTile;
  const int64_t L = std::max(kNearestMinSliceTiles, (p.tiles + kNearestTargetSlices - 1) / kNearestTargetSlices);
  p.slices = (p.tiles + L - 1) / L;
  for (int64_t i = 0; i < p.slices; i++) p.slice_tile.push_back(uint32_t(p.tiles * i / p.slices));
  p.slice_tile.push_back(uint32_t(p.tiles));

  std::vector<double> mean(size_t(F), 0.0);
  for (int64_t m = 0; m < M; m++)
    for (int64_t k = 0; k < F; k++) mean[size_t(k)] += double(C[m * F + k]);
  p.center.assign(size_t(p.F_pad), 0.f);
  for (int64_t k = 0; k < F; k++) p.center[size_t(k)] = float(mean[size_t(k)] / double(M));
  const int64_t npad = p.tiles * kNearestTile;
  auto cval = [&](int64_t m, int64_t k) -> float {  // centred f32 value of padded vector m, feature k
    if (k >= F || m >= M) return 0.f;
    return float(double(C[m * F + k]) - double(p.center[size_t(k)]));
  };
  const int64_t G = p.F_pad / 8;
  p.ref.assign(size_t(npad * p.F_pad), 0.f);
  for (int64_t t = 0; t < p.tiles; t++)
    for (int64_t g = 0; g < G; g++)
      for (int lane = 0; lane < 64; lane++)
        for (int j = 0; j < 4; j++)
          p.ref[size_t(((t * G + g) * 64 + lane) * 4 + j)] = cval(t * kNearestTile + (lane & 31), 8 * g + 4 * (lane >> 5) + j);
  p.ref_norm.assign(size_t(npad), 0.f);
  for (int64_t m = 0; m < M; m++) {
    double a = 0.0;
    for (int64_t k = 0; k < F; k++) a += double(cval(m, k)) * double(cval(m, k));
    p.ref_norm[size_t(m)] = float(a);
  }
  return p;
}

}  // namespace infera_hip
