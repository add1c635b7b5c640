// channelnorm.cpp -- checks and the work split of the ChannelNorm step (host/channelnorm.hpp).
#include "channelnorm.hpp"

#include <cmath>

namespace infera_hip {

ChannelNormSplit channelnorm_split(int64_t C, bool cq) {
  ChannelNormSplit sp;
  sp.units = int(cq ? C / 4 : C);
  sp.waves = C <= kChannelNormOneWaveMaxC ? 1 : 4;
  sp.per_wave = (sp.units + sp.waves - 1) / sp.waves;
  // the instantiated register sizes (channelnorm.hip): floats per lane on NCHW tensors, quads per lane on channel quads
  static const int nchw_sizes[] = {1, 2, 4, 8, 16, 32, 64, 128}, cq_sizes[] = {1, 2, 4, 8, 16, 32};
  if (C <= kChannelNormRegsMaxC)
    for (int r : nchw_sizes) {
      if (cq && r > cq_sizes[5]) break;
      // one wave: it holds all the units; four: whole slices of r units in at most three waves and a remainder, or in all four
      if (!sp.regs && (sp.waves == 1 ? r >= sp.units : (r >= (cq ? 4 : 16) && (sp.units + r - 1) / r <= 4))) sp.regs = r;
    }
  return sp;
}

std::string channelnorm_refusal(int64_t C, int64_t S, int64_t n_scale, int64_t n_bias, float eps) {
  if (C <= 0 || S <= 0) return "symbolic channel or spatial extents (only the row axis may be symbolic)";
  if (C > kChannelNormMaxC) return "C = " + std::to_string(C) + " is beyond the ChannelNorm kernel's cap of " + std::to_string(kChannelNormMaxC);
  if (S > kChannelNormMaxS) return "H * W = " + std::to_string(S) + " is beyond the ChannelNorm kernel's cap of " + std::to_string(kChannelNormMaxS);
  if (n_scale != C || (n_bias >= 0 && n_bias != C))
    return "Scale / B must have C = " + std::to_string(C) + " elements, got " + std::to_string(n_scale) + (n_bias >= 0 ? " and " + std::to_string(n_bias) : std::string());
  if (!(eps >= 0.f) || !std::isfinite(eps)) return "epsilon must be a finite number >= 0";
  return "";
}

}  // namespace infera_hip
