// pixelshuffle.hpp -- DepthToSpace / SpaceToDepth and their Reshape -> Transpose -> Reshape spellings as one step kind:
// the four forms, the caps the lowering checks and which form of the kernel a layer gets once the scheduler knows the layouts of its two
// tensors.  Every value written is a bit copy of a value read.  With block size b, i, j in [0, b), k = i b + j:
//   depth to space, block-major (DepthToSpace DCR):     y[n, c, h b + i, w b + j] = x[n, k C' + c, h, w],   C' = C / b^2
//   depth to space, channel-major (CRD, pixel_shuffle): y[n, c, h b + i, w b + j] = x[n, c b^2 + k, h, w]
//   space to depth, block-major (SpaceToDepth):         y[n, k C + c, h, w] = x[n, c, h b + i, w b + j]
//   space to depth, channel-major (pixel_unshuffle):    y[n, c b^2 + k, h, w] = x[n, c, h b + i, w b + j]
#pragma once

#include <cstdint>

namespace infera_hip {

constexpr int64_t kPixelShuffleMaxC = 65536;                // channels of the wider side
constexpr int64_t kPixelShuffleMaxS = int64_t(1) << 20;     // pixels of the larger plane

// The forms of the kernel (pixelshuffle.hip), Step::out_mode of a scheduled PixelShuffle step
enum PixelShuffleKernel : int {
  kPixelShuffleGeneric = 0,    // any block, channel count and layout pairing: one output element (NCHW) or one gathered output quad per lane
  kPixelShuffleQuadCopy = 1,   // block-major, channel quads to channel quads: an output quad is an input quad -- one 16-byte load and store per lane
  kPixelShuffleTranspose = 2,  // channel-major with b = 2 or 4, channel quads to channel quads: four quads transposed 4 x 4 in registers
  kPixelShuffleCqToNchw = 3,   // channel quads in, NCHW out (the served output): one input quad per lane
  kPixelShuffleNchwToCq = 4,   // NCHW in (the caller's image), channel quads out: one output quad per lane
};
inline const char *pixelshuffle_kernel_name(int k) {
  static const char *names[] = {"pixelshuffle_generic", "pixelshuffle_quad_copy", "pixelshuffle_transpose", "pixelshuffle_cq_to_nchw", "pixelshuffle_nchw_to_cq"};
  return names[k];
}
// C = the input's channels; in_cq / out_cq: the tensor lies in channel-quad planes (its channel count is then whole quads);
// fast = false (INFERA_PIXELSHUFFLE_FAST=0): the generic form everywhere
inline int pixelshuffle_kernel(int64_t b, bool to_space, bool channel_major, int64_t C, bool in_cq, bool out_cq, bool fast) {
  if (!fast) return kPixelShuffleGeneric;
  const int64_t small = to_space ? C / (b * b) : C;  // the channels of the spatially larger tensor: what a block-major form keeps together
  if (in_cq && out_cq) {
    if (!channel_major && small % 4 == 0) return kPixelShuffleQuadCopy;
    if (channel_major && (b == 2 || b == 4)) return kPixelShuffleTranspose;
    return kPixelShuffleGeneric;
  }
  if (in_cq) return kPixelShuffleCqToNchw;
  if (out_cq) return kPixelShuffleNchwToCq;
  return kPixelShuffleGeneric;
}
inline const char *pixelshuffle_form_name(bool to_space, bool channel_major) {
  return to_space ? (channel_major ? "depth_to_space_crd" : "depth_to_space_dcr") : (channel_major ? "pixel_unshuffle" : "space_to_depth");
}

}  // namespace infera_hip
