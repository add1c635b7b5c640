// gridsample.hpp -- GridSample and AffineGrid (INTEGRATION.md 2.6 "Grid sampling"): the forms, the caps the lowering checks and
// the coordinate function -- a sampling coordinate to source offsets, weights and in-bounds flags -- as one __host__ __device__ definition, so
// that hip/gridsample.hip and a host program (tests/native/gridsample_index.cpp) run the same code.  Everything here is a fixed sequence of
// separately rounded f32 operations: include it only where floating-point contraction is off (the kernel file says so itself).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define INFERA_GS_HD __host__ __device__ inline
#else
#define INFERA_GS_HD inline
#endif

namespace infera_hip {

enum GridSampleMode : int { kGridBilinear = 0, kGridNearest = 1 };
enum GridSamplePad : int { kGridZeros = 0, kGridBorder = 1, kGridReflection = 2 };
// where a position's (x, y) comes from: a [N,Ho,Wo,2] buffer, a [N,2,Ho,Wo] buffer (a flow field read through a channels-last view), or
// six numbers per image (AffineGrid absorbed: the grid is never written)
enum GridSampleCoords : int { kGridCoordsGrid = 0, kGridCoordsPlanar = 1, kGridCoordsAffine = 2 };

// An extent above 2^24 has pixel coordinates that are no f32 values any more; a plane of 2^31 pixels has offsets that leave int
constexpr int64_t kGridSampleMaxExtent = int64_t(1) << 24;
constexpr int64_t kGridSampleMaxPlane = int64_t(1) << 31;

inline const char *gridsample_mode_name(int m) { return m == kGridNearest ? "nearest" : "bilinear"; }
inline const char *gridsample_pad_name(int p) { return p == kGridBorder ? "border" : p == kGridReflection ? "reflection" : "zeros"; }
inline const char *gridsample_coords_name(int c) { return c == kGridCoordsPlanar ? "planar" : c == kGridCoordsAffine ? "affine" : "grid"; }
// the kernel variant of a scheduled step, by the layouts of X and Y
inline const char *gridsample_exec_name(int mode, bool in_cq, bool out_cq) {
  static const char *names[] = {"gridsample_bilinear_nchw", "gridsample_bilinear_cq_in", "gridsample_bilinear_cq_out", "gridsample_bilinear_cq",
                                "gridsample_nearest_nchw",  "gridsample_nearest_cq_in",  "gridsample_nearest_cq_out",  "gridsample_nearest_cq"};
  return names[(mode == kGridNearest ? 4 : 0) + (out_cq ? 2 : 0) + (in_cq ? 1 : 0)];
}

// What one output position reads: up to four taps of a plane [H, W].  Tap k = (dy, dx) = (k >> 1, k & 1) of the cell; `nearest` uses tap 0 alone.
// A tap whose bit in `inside` is clear is read as +0 and its offset is 0; `nan`: the coordinate was NaN before or after the padding rule and the
// result is NaN whatever the plane holds.  Every offset lies in [0, H * W).
struct GridTaps {
  int32_t off[4];
  float w[4];
  uint32_t inside;
  bool nan;
};

// a normalised coordinate g in [-1, 1] to pixels of an axis of `size`
INFERA_GS_HD float gridsample_unnormalize(float g, int size, bool align_corners) {
  const float t = g + 1.f;
  if (align_corners) {
    const float u = t * 0.5f;
    return u * float(size - 1);
  }
  const float u = t * float(size);
  const float v = u - 1.f;
  return v * 0.5f;
}

// reflection about the pixel centres 0 and size - 1 (align_corners) or the pixel edges -1/2 and size - 1/2.  fmodf is exact; +-inf gives NaN
INFERA_GS_HD float gridsample_reflect(float c, int size, bool align_corners) {
  const float lo = align_corners ? 0.f : -0.5f;
  const float span = align_corners ? float(size - 1) : float(size);
  if (span == 0.f) return 0.f;
  const float d = fabsf(c - lo);
  const float extra = fmodf(d, span);
  const float flips = floorf(d / span);
  const bool even = fmodf(flips, 2.f) == 0.f;
  return even ? extra + lo : (span - extra) + lo;
}

// the padding rule and the clamp that makes the conversion to an integer safe: the result is a number in [-2, size + 1] (never NaN);
// *was_nan: the coordinate was NaN on the way
INFERA_GS_HD float gridsample_pad_coord(float c, int size, int pad, bool align_corners, bool *was_nan) {
  bool nan = !(c == c);
  if (pad == kGridReflection) {
    c = gridsample_reflect(c, size, align_corners);
    nan = nan || !(c == c);
  }
  if (pad != kGridZeros) {  // border, and what reflection leaves outside by rounding
    c = c >= 0.f ? c : 0.f;
    c = c <= float(size - 1) ? c : float(size - 1);
  }
  // (zeros: everything at or below -2 or at or above size + 1 reads no pixel, as the clamped value does; NaN compares false and lands on -2)
  c = c >= -2.f ? c : -2.f;
  c = c <= float(size + 1) ? c : float(size + 1);
  *was_nan = *was_nan || nan;
  return c;
}

// normalised (gx, gy) -> the taps in a plane [H, W]
INFERA_GS_HD GridTaps gridsample_taps(float gx, float gy, int H, int W, int mode, int pad, bool align_corners) {
  GridTaps t;
  t.nan = false;
  t.inside = 0;
  const float ix = gridsample_pad_coord(gridsample_unnormalize(gx, W, align_corners), W, pad, align_corners, &t.nan);
  const float iy = gridsample_pad_coord(gridsample_unnormalize(gy, H, align_corners), H, pad, align_corners, &t.nan);
  for (int k = 0; k < 4; k++) t.off[k] = 0, t.w[k] = 0.f;
  if (mode == kGridNearest) {
    const int x = int(nearbyintf(ix)), y = int(nearbyintf(iy));  // (round half to even)
    if (x >= 0 && x < W && y >= 0 && y < H) t.inside = 1, t.off[0] = y * W + x;
    t.w[0] = 1.f;
    return t;
  }
  const float fx = floorf(ix), fy = floorf(iy);
  const float tx = ix - fx, ty = iy - fy;
  const float wx[2] = {1.f - tx, tx}, wy[2] = {1.f - ty, ty};
  const int x0 = int(fx), y0 = int(fy);
  for (int k = 0; k < 4; k++) {
    const int y = y0 + (k >> 1), x = x0 + (k & 1);
    t.w[k] = wy[k >> 1] * wx[k & 1];
    if (x >= 0 && x < W && y >= 0 && y < H) t.inside |= 1u << k, t.off[k] = y * W + x;
  }
  return t;
}

// the four products and three sums of a bilinear sample, in this order
INFERA_GS_HD float gridsample_blend(const GridTaps &t, float v00, float v01, float v10, float v11) {
  const float p0 = v00 * t.w[0], p1 = v01 * t.w[1], p2 = v10 * t.w[2], p3 = v11 * t.w[3];
  return ((p0 + p1) + p2) + p3;
}

// AffineGrid: the base coordinate of index j of an axis of `size` (pixel centres; align_corners: the end points are -1 and 1; one pixel: 0)
INFERA_GS_HD float affinegrid_base(int j, int size, bool align_corners) {
  if (align_corners) return size > 1 ? float(2 * j) / float(size - 1) - 1.f : 0.f;
  return float(2 * j + 1) / float(size) - 1.f;
}
// ... and the coordinate pair of (oh, ow) under theta = [[t0, t1, t2], [t3, t4, t5]]
INFERA_GS_HD void affinegrid_point(const float *theta, int oh, int ow, int OH, int OW, bool align_corners, float *gx, float *gy) {
  const float xb = affinegrid_base(ow, OW, align_corners), yb = affinegrid_base(oh, OH, align_corners);
  const float a0 = theta[0] * xb, a1 = theta[1] * yb, b0 = theta[3] * xb, b1 = theta[4] * yb;
  *gx = (a0 + a1) + theta[2];
  *gy = (b0 + b1) + theta[5];
}

}  // namespace infera_hip
