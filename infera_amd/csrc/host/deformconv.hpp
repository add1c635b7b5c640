// deformconv.hpp -- DeformConv (INTEGRATION.md 2.6 "Deformable convolutions"): the geometry of a DeformConv2d step, how the
// deformconv kernels split it, and the coordinate function -- a tap's base position and its offset pair to the four corner offsets, weights and
// in-bounds flags -- as one __host__ __device__ definition, so that both kernels of hip/deformconv.hip and a host program
// (tests/native/deformconv_index.cpp) run the same code.  The coordinate function is a fixed sequence of separately rounded f32 operations:
// include it only where floating-point contraction is off (the kernel file says so itself).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define INFERA_DC_HD __host__ __device__ inline
#else
#define INFERA_DC_HD inline
#endif

namespace infera_hip {

struct DeformGeom {
  int C = 0, H = 0, W = 0, M = 0, OH = 0, OW = 0;
  int kh = 1, kw = 1, sh = 1, sw = 1, pt = 0, pl = 0, dh = 1, dw = 1, groups = 1, ogroups = 1;
  bool has_mask = false;
};

constexpr int kDeformMaxKernel = 64;  // largest kernel extent on either axis
constexpr int kDeformTilePos = 32;    // output positions of one work group: one 32-column MFMA tile
constexpr int kDeformChunk = 8;       // channels whose deformed columns are sampled into LDS at a time
// deformconv_mfma's cap on kh * kw: the column tile of one chunk is kDeformChunk * taps rows of 32 floats, taps KiB -- 49 KiB at 7 x 7, the
// largest kernel of the DCN literature, inside the 64 KiB a work group gets without opting in
constexpr int kDeformMaxTaps = 49;

// StepSchedule::form of a DeformConv2d step: which tensors lie in channel quads, and the kernel
enum DeformForm : int { kDeformXcq = 1, kDeformYcq = 2, kDeformOffCq = 4, kDeformMaskCq = 8, kDeformMfma = 16 };

// deformconv_mfma's split: k = c * taps + tap runs over K = C * taps rows (Kp: K rounded up to the instruction's k-pairs), walked in chunks of
// kDeformChunk channels; Mp = M rounded up to whole 32-channel tiles, `waves` of them side by side in a work group, `per_wave` tiles each
struct DeformSplit {
  int taps = 0, chunks = 0, Mp = 0, waves = 0, per_wave = 0, zblocks = 0;
  int64_t K = 0, Kp = 0, lds_bytes = 0;
};
inline DeformSplit deform_split(const DeformGeom &g) {
  DeformSplit s;
  s.taps = g.kh * g.kw;
  s.chunks = (g.C + kDeformChunk - 1) / kDeformChunk;
  s.K = int64_t(g.C) * s.taps;
  s.Kp = (s.K + 1) / 2 * 2;
  s.Mp = (g.M + 31) / 32 * 32;
  const int mtiles = s.Mp / 32;
  s.waves = mtiles < 4 ? mtiles : 4;
  const int need = (mtiles + s.waves - 1) / s.waves;
  s.per_wave = need >= 3 ? 4 : need;
  s.zblocks = (mtiles + s.waves * s.per_wave - 1) / (s.waves * s.per_wave);
  s.lds_bytes = int64_t(kDeformChunk) * s.taps * kDeformTilePos * 4;
  return s;
}
// the kernel that serves the layer: the MFMA form takes group == 1 with kh * kw up to the cap, the generic one the rest (and everything
// under INFERA_DEFORMCONV_MFMA=0)
inline bool deform_takes_mfma(const DeformGeom &g, bool knob) { return knob && g.groups == 1 && g.kh * g.kw <= kDeformMaxTaps; }

// What one tap of one output position reads from a plane [H, W]: corner k = (dy, dx) = (k >> 1, k & 1) of the cell.  A corner whose bit in
// `inside` is clear is read as +0 and its offset is 0; `nan`: a coordinate was NaN and the sample is NaN whatever the plane holds.  Every
// offset lies in [0, H * W).
struct DeformTap {
  int32_t off[4];
  float w[4];
  uint32_t inside;
  bool nan;
};

// The clamp that makes the conversion to an integer safe: a number in [-2, size + 1].  Everything at or below -2 or at or above size + 1 reads
// no pixel, as the clamped value does (NaN compares false and lands on -2; the caller has flagged it).
INFERA_DC_HD float deform_clamp(float c, int size) {
  c = c >= -2.f ? c : -2.f;
  return c <= float(size + 1) ? c : float(size + 1);
}

// (by, bx) = (oh * sh - pt + i * dh, ow * sw - pl + j * dw), the tap's position on the fixed grid; (off_y, off_x) its learned offset
INFERA_DC_HD DeformTap deform_tap(int by, int bx, float off_y, float off_x, int H, int W) {
  DeformTap t;
  const float sy = float(by) + off_y, sx = float(bx) + off_x;
  t.nan = !(sy == sy) || !(sx == sx);
  t.inside = 0;
  const float cy = deform_clamp(sy, H), cx = deform_clamp(sx, W);
  const float fy = floorf(cy), fx = floorf(cx);
  const float ty = cy - fy, tx = cx - fx;
  const float wy[2] = {1.f - ty, ty}, wx[2] = {1.f - tx, tx};
  const int y0 = int(fy), x0 = int(fx);
  for (int k = 0; k < 4; k++) {
    const int y = y0 + (k >> 1), x = x0 + (k & 1);
    t.w[k] = wy[k >> 1] * wx[k & 1];
    t.off[k] = 0;
    if (x >= 0 && x < W && y >= 0 && y < H) t.inside |= 1u << k, t.off[k] = y * W + x;
  }
  return t;
}

// the four products and three sums of a sample, in this order, then the modulation mask
INFERA_DC_HD float deform_blend(const DeformTap &t, float v00, float v01, float v10, float v11, float mask) {
  const float p0 = v00 * t.w[0], p1 = v01 * t.w[1], p2 = v10 * t.w[2], p3 = v11 * t.w[3];
  const float v = ((p0 + p1) + p2) + p3;
  return v * mask;
}

}  // namespace infera_hip
