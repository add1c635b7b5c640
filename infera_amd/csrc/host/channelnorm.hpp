// channelnorm.hpp -- LayerNorm over the channel axis at each pixel of an [N,C,H,W] tensor (ConvNeXt's LayerNorm2d, Hugging Face's
// ConvNextLayerNorm) as one step kind: what the lowering checks and which of the kernel's two forms a layer gets once
// the scheduler knows the tensor's layout.
//   For row n and pixel s of S = H * W, over the C channels, all f32:
//     mean = sum(x) / C;  d = x - mean;  resid = sum(d) / C;  d -= resid;  var = sum(d^2) / C;  y = act(d / sqrtf(var + eps) * gamma[c] + beta[c])
//   Lanes run along the pixels; the waves of a workgroup share a tile of 64 pixels and split the channels (or, for C <= 32, each wave
//   takes a tile of its own and all the channels).
//   channelnorm_regs   (C <= 512): a lane keeps its slice of the pixel in registers: x is read once and written once;
//   channelnorm_reread (larger C, or INFERA_CHANNELNORM_REGS=0): a lane reads its slice again for each centring and for the write.
#pragma once

#include <cstdint>
#include <string>

namespace infera_hip {

constexpr int64_t kChannelNormMaxC = 4096;                 // = kLnMaxE (host/attention.hpp)
constexpr int64_t kChannelNormMaxS = int64_t(1) << 20;     // pixels per image
constexpr int64_t kChannelNormOneWaveMaxC = 32;            // up to here a wave holds all the channels of its pixels
constexpr int64_t kChannelNormRegsMaxC = 512;              // the largest C of the register form: 4 waves x 128 floats (32 quads) per lane

// How the kernel divides a layer of C channels on an NCHW (cq = false) or channel-quad tensor: units (channels, or quads of them) per
// pixel and the waves that share a pixel.  The re-read form: wave w takes units [w per_wave, (w + 1) per_wave).  The register form: `regs` =
// the units a lane has registers for (an instantiated size); one wave: regs >= units; four: wave w < units / regs holds units
// [w regs, (w + 1) regs) and the wave behind them reads the remainder again (regs = 0: C is beyond the register form)
struct ChannelNormSplit {
  int units = 0, waves = 1, per_wave = 0, regs = 0;
};
ChannelNormSplit channelnorm_split(int64_t C, bool cq);
// does a layer take the register form?  (`allowed`: INFERA_CHANNELNORM_REGS)
inline bool channelnorm_regs_form(int64_t C, bool allowed) { return allowed && C <= kChannelNormRegsMaxC; }

// why a layer cannot be served ("" = it can): C channels over S pixels, scale / B lengths (n_bias < 0: no B)
std::string channelnorm_refusal(int64_t C, int64_t S, int64_t n_scale, int64_t n_bias, float eps);

}  // namespace infera_hip
