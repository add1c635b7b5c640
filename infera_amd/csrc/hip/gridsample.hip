// gridsample.hip -- GridSample over an [N,C,H,W] tensor, and AffineGrid where its grid has to be written (host/gridsample.hpp has the coordinate
// function and the forms; INTEGRATION.md 2.6 "Grid sampling" the contract; DESIGN.md 3.26 the split).
//   work per block   kTile = 256 consecutive output positions of the flattened (image, oh, ow) index, one lane per position; a wave's 64 positions
//                    are consecutive along ow, so every store of a plane (NCHW) or of a quad plane (channel quads) is coalesced.
//   coordinates      the lane reads its (x, y) -- from the grid, from the two planes of a flow field, or from the image's six affine numbers --
//                    and computes its GridTaps ONCE: four (one) offsets inside a plane, the weights, the in-bounds mask.  They stay in registers
//                    while the lane walks the channels; an offset is always inside the plane (an absent tap has offset 0 and is not loaded).
//   the channel walk NCHW: plane by plane, four (one) scalar loads per channel.  Channel quads: one 16-byte load per corner serves four channels.
//                    The corners of neighbouring lanes are neighbours in the plane for any smooth warp, so they meet in L1 / L2; nothing is
//                    staged in LDS (conv3d.hip's direct form measured the same for taps contiguous along ow).
//   the two layouts  X and Y each lie in NCHW or in channel quads [N, C/4, H, W, 4], independently: four template forms per mode.
// The arithmetic is a fixed sequence of separately rounded f32 operations (contraction is off for this file): a position's bits depend on its
// own coordinate and samples only, whatever the batch, the tile or the layout.
#include "device_common.hpp"

#pragma clang fp contract(off)

#include "../host/gridsample.hpp"

#include <algorithm>

namespace infera_hip::kern {

namespace {

constexpr int kTile = 256;

// the normalised coordinate pair of position p = oh * OW + ow of image n
__device__ __forceinline__ void coords_of(const float *__restrict__ G, const GridSampleGeom &g, int64_t n, int p, float &gx, float &gy) {
  const int64_t OP = int64_t(g.OH) * g.OW;
  if (g.coords == kGridCoordsGrid) {
    const float *at = G + (n * OP + p) * 2;
    gx = at[0], gy = at[1];
  } else if (g.coords == kGridCoordsPlanar) {
    gx = G[(n * 2) * OP + p], gy = G[(n * 2 + 1) * OP + p];
  } else {
    const float *th = G + n * 6;
    const float theta[6] = {th[0], th[1], th[2], th[3], th[4], th[5]};
    affinegrid_point(theta, p / g.OW, p % g.OW, g.OH, g.OW, g.align_corners, &gx, &gy);
  }
}

__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7FC00000u); }

// one channel's sample from its plane
template <bool NEAREST>
__device__ __forceinline__ float sample_plane(const float *__restrict__ plane, const GridTaps &t) {
  if (t.nan) return quiet_nan();
  if constexpr (NEAREST) return (t.inside & 1u) ? plane[t.off[0]] : 0.f;
  const float v00 = (t.inside & 1u) ? plane[t.off[0]] : 0.f, v01 = (t.inside & 2u) ? plane[t.off[1]] : 0.f;
  const float v10 = (t.inside & 4u) ? plane[t.off[2]] : 0.f, v11 = (t.inside & 8u) ? plane[t.off[3]] : 0.f;
  return gridsample_blend(t, v00, v01, v10, v11);
}
// four channels' samples from their quad plane
template <bool NEAREST>
__device__ __forceinline__ f32x4 sample_quads(const f32x4 *__restrict__ plane, const GridTaps &t) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (t.nan) return f32x4{quiet_nan(), quiet_nan(), quiet_nan(), quiet_nan()};
  if constexpr (NEAREST) return (t.inside & 1u) ? plane[t.off[0]] : zero;
  const f32x4 v00 = (t.inside & 1u) ? plane[t.off[0]] : zero, v01 = (t.inside & 2u) ? plane[t.off[1]] : zero;
  const f32x4 v10 = (t.inside & 4u) ? plane[t.off[2]] : zero, v11 = (t.inside & 8u) ? plane[t.off[3]] : zero;
  f32x4 y;
#pragma unroll
  for (int k = 0; k < 4; k++) y[k] = gridsample_blend(t, v00[k], v01[k], v10[k], v11[k]);
  return y;
}

// total = rows * OH * OW positions.  A channel-quad side holds whole quads (the launcher checks)
template <bool NEAREST, bool IN_CQ, bool OUT_CQ>
__global__ __launch_bounds__(kTile) void gridsample_kernel(const float *__restrict__ X, const float *__restrict__ G, float *__restrict__ Y, int64_t total, GridSampleGeom g) {
  const int64_t e = int64_t(blockIdx.x) * kTile + threadIdx.x;
  if (e >= total) return;
  const int64_t OP = int64_t(g.OH) * g.OW, IP = int64_t(g.H) * g.W;
  const int64_t n = e / OP;
  const int p = int(e - n * OP);
  float gx, gy;
  coords_of(G, g, n, p, gx, gy);
  const GridTaps t = gridsample_taps(gx, gy, g.H, g.W, NEAREST ? kGridNearest : kGridBilinear, g.pad, g.align_corners);
  const int C = g.C;
  if constexpr (IN_CQ) {
    const f32x4 *x4 = reinterpret_cast<const f32x4 *>(X) + n * (C / 4) * IP;
    for (int q = 0; q < C / 4; q++) {
      const f32x4 v = sample_quads<NEAREST>(x4 + q * IP, t);
      if constexpr (OUT_CQ) {
        reinterpret_cast<f32x4 *>(Y)[(n * (C / 4) + q) * OP + p] = v;
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++) Y[(n * C + 4 * q + k) * OP + p] = v[k];
      }
    }
  } else {
    const float *x = X + n * C * IP;
    if constexpr (OUT_CQ) {
      for (int q = 0; q < C / 4; q++) {
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = sample_plane<NEAREST>(x + (4 * q + k) * IP, t);
        reinterpret_cast<f32x4 *>(Y)[(n * (C / 4) + q) * OP + p] = v;
      }
    } else {
      for (int c = 0; c < C; c++) Y[(n * C + c) * OP + p] = sample_plane<NEAREST>(x + c * IP, t);
    }
  }
}

// AffineGrid with a reader of its own: the grid [rows, OH, OW, 2], one position per lane
__global__ __launch_bounds__(kTile) void affinegrid_kernel(const float *__restrict__ theta, float *__restrict__ Y, int64_t total, int OH, int OW, bool align_corners) {
  const int64_t e = int64_t(blockIdx.x) * kTile + threadIdx.x;
  if (e >= total) return;
  const int64_t OP = int64_t(OH) * OW, n = e / OP;
  const int p = int(e - n * OP);
  const float *th = theta + n * 6;
  const float t6[6] = {th[0], th[1], th[2], th[3], th[4], th[5]};
  float gx, gy;
  affinegrid_point(t6, p / OW, p % OW, OH, OW, align_corners, &gx, &gy);
  Y[2 * e] = gx;
  Y[2 * e + 1] = gy;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool NEAREST>
void launch_form(hipStream_t s, const float *X, const float *G, float *Y, int64_t total, const GridSampleGeom &g, bool in_cq, bool out_cq) {
  const dim3 grid(unsigned((total + kTile - 1) / kTile)), block(kTile);
  if (in_cq && out_cq) hipLaunchKernelGGL((gridsample_kernel<NEAREST, true, true>), grid, block, 0, s, X, G, Y, total, g);
  else if (in_cq) hipLaunchKernelGGL((gridsample_kernel<NEAREST, true, false>), grid, block, 0, s, X, G, Y, total, g);
  else if (out_cq) hipLaunchKernelGGL((gridsample_kernel<NEAREST, false, true>), grid, block, 0, s, X, G, Y, total, g);
  else hipLaunchKernelGGL((gridsample_kernel<NEAREST, false, false>), grid, block, 0, s, X, G, Y, total, g);
}

}  // namespace

bool grid_sample(hipStream_t s, const float *X, const float *G, float *Y, int64_t rows, const GridSampleGeom &g, bool in_cq, bool out_cq) {
  // what the kernel relies on: extents the coordinate function takes, planes whose offsets stay in int, whole quads on a channel-quad side
  if (g.C < 1 || g.H < 1 || g.W < 1 || g.OH < 1 || g.OW < 1 || g.H > kGridSampleMaxExtent || g.W > kGridSampleMaxExtent ||
      int64_t(g.H) * g.W >= kGridSampleMaxPlane || int64_t(g.OH) * g.OW >= kGridSampleMaxPlane)
    return false;
  if (g.mode != kGridBilinear && g.mode != kGridNearest) return false;
  if (g.pad != kGridZeros && g.pad != kGridBorder && g.pad != kGridReflection) return false;
  if (g.coords != kGridCoordsGrid && g.coords != kGridCoordsPlanar && g.coords != kGridCoordsAffine) return false;
  if ((in_cq && (g.C % 4 != 0 || !aligned16(X))) || (out_cq && (g.C % 4 != 0 || !aligned16(Y)))) return false;
  const int64_t total = rows * g.OH * g.OW;
  if (total <= 0) return true;
  if ((total + kTile - 1) / kTile > int64_t(0x7FFFFFFF)) return false;
  if (g.mode == kGridNearest) launch_form<true>(s, X, G, Y, total, g, in_cq, out_cq);
  else launch_form<false>(s, X, G, Y, total, g, in_cq, out_cq);
  return true;
}

bool affine_grid(hipStream_t s, const float *theta, float *Y, int64_t rows, int OH, int OW, bool align_corners) {
  if (OH < 1 || OW < 1 || int64_t(OH) * OW >= kGridSampleMaxPlane) return false;
  const int64_t total = rows * OH * OW;
  if (total <= 0) return true;
  if ((total + kTile - 1) / kTile > int64_t(0x7FFFFFFF)) return false;
  hipLaunchKernelGGL(affinegrid_kernel, dim3(unsigned((total + kTile - 1) / kTile)), dim3(kTile), 0, s, theta, Y, total, OH, OW, align_corners);
  return true;
}

}  // namespace infera_hip::kern
