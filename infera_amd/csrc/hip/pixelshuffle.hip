// pixelshuffle.hip -- DepthToSpace / SpaceToDepth of an [N,C,H,W] tensor (host/pixelshuffle.hpp has the four index formulas): an HBM-bound
// copy, so the work is in the access pattern.  Every form is grid-stride with 64-bit element indices, one unit per lane, consecutive lanes
// along the fastest axis of whichever side the form reads or writes in 16-byte pieces; no LDS, no tables, no arithmetic on a value.
//   pixelshuffle_quad_copy   block-major, channel quads to channel quads: an output quad IS an input quad (one 16-byte load, one store)
//   pixelshuffle_transpose   channel-major, b = 2 or 4, channel quads to channel quads: a lane loads four quads along w, transposes them
//                            4 x 4 in registers and stores four quads, of which its b neighbouring pixels of an output row are adjacent
//   pixelshuffle_cq_to_nchw  one input quad per lane, stored as 2 x 8 bytes (channel-major b = 2: the quad is a 2 x 2 block of one output
//                            channel), 16 bytes (channel-major b = 4: four pixels of one output row) or four scalars
//   pixelshuffle_nchw_to_cq  one output quad per lane, from 2 x 8 bytes (channel-major b = 2) or four scalars
//   pixelshuffle_generic     one output element (NCHW) or one output quad gathered from four scalars (channel quads) per lane
#include "device_common.hpp"
#include "../host/pixelshuffle.hpp"

#include <algorithm>

namespace infera_hip::kern {

namespace {

constexpr int kBlock = 256;
using f32x2 = __attribute__((ext_vector_type(2))) float;

__device__ __forceinline__ int64_t nchw_at(int64_t n, int c, int y, int x, int C, int H, int W) { return ((n * C + c) * H + y) * W + x; }
__device__ __forceinline__ int64_t quad_at(int64_t n, int q, int y, int x, int Q, int H, int W) { return ((n * Q + q) * H + y) * W + x; }  // in f32x4 units
__device__ __forceinline__ int64_t cq_at(int64_t n, int c, int y, int x, int C, int H, int W) { return quad_at(n, c >> 2, y, x, C >> 2, H, W) * 4 + (c & 3); }

// the input element (c, y, x) that output element (oc, oh, ow) copies
__device__ __forceinline__ void source_of(const PixelShuffleGeom &g, int oc, int oh, int ow, int &c, int &y, int &x) {
  const int b = g.b;
  if (g.to_space) {
    const int k = (oh % b) * b + ow % b;
    c = g.channel_major ? oc * b * b + k : k * g.OC + oc;
    y = oh / b;
    x = ow / b;
  } else {
    const int k = g.channel_major ? oc % (b * b) : oc / g.C;
    c = g.channel_major ? oc / (b * b) : oc % g.C;
    y = oh * b + k / b;
    x = ow * b + k % b;
  }
}
// the output element (oc, oh, ow) that input element (c, y, x) is copied to
__device__ __forceinline__ void dest_of(const PixelShuffleGeom &g, int c, int y, int x, int &oc, int &oh, int &ow) {
  const int b = g.b;
  if (g.to_space) {
    const int k = g.channel_major ? c % (b * b) : c / g.OC;
    oc = g.channel_major ? c / (b * b) : c % g.OC;
    oh = y * b + k / b;
    ow = x * b + k % b;
  } else {
    const int k = (y % b) * b + x % b;
    oc = g.channel_major ? c * b * b + k : k * g.C + c;
    oh = y / b;
    ow = x / b;
  }
}

template <bool IN_CQ>
__device__ __forceinline__ float load_at(const float *__restrict__ X, const PixelShuffleGeom &g, int64_t n, int c, int y, int x) {
  return X[IN_CQ ? cq_at(n, c, y, x, g.C, g.H, g.W) : nchw_at(n, c, y, x, g.C, g.H, g.W)];
}

// total = rows * OC * OH * OW elements (NCHW out) or rows * OC / 4 * OH * OW quads (channel quads out)
template <bool IN_CQ, bool OUT_CQ>
__global__ __launch_bounds__(kBlock) void pixelshuffle_generic_kernel(const float *__restrict__ X, float *__restrict__ Y, int64_t total, PixelShuffleGeom g) {
  const int units = OUT_CQ ? g.OC / 4 : g.OC;
  for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < total; e += int64_t(gridDim.x) * kBlock) {
    const int ow = int(e % g.OW);
    int64_t t = e / g.OW;
    const int oh = int(t % g.OH);
    t /= g.OH;
    const int u = int(t % units);
    const int64_t n = t / units;
    int c, y, x;
    if constexpr (OUT_CQ) {
      f32x4 v;
      for (int k = 0; k < 4; k++) {
        source_of(g, 4 * u + k, oh, ow, c, y, x);
        v[k] = load_at<IN_CQ>(X, g, n, c, y, x);
      }
      reinterpret_cast<f32x4 *>(Y)[e] = v;
    } else {
      source_of(g, u, oh, ow, c, y, x);
      Y[e] = load_at<IN_CQ>(X, g, n, c, y, x);
    }
  }
}

// block-major, both tensors in channel quads, whole quads on the spatially larger side: total = rows * OC / 4 * OH * OW output quads
__global__ __launch_bounds__(kBlock) void pixelshuffle_quad_copy_kernel(const f32x4 *__restrict__ X, f32x4 *__restrict__ Y, int64_t total, PixelShuffleGeom g) {
  const int OQ = g.OC / 4, IQ = g.C / 4, b = g.b;
  for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < total; e += int64_t(gridDim.x) * kBlock) {
    const int ow = int(e % g.OW);
    int64_t t = e / g.OW;
    const int oh = int(t % g.OH);
    t /= g.OH;
    const int q = int(t % OQ);
    const int64_t n = t / OQ;
    int sq, y, x;
    if (g.to_space) {
      sq = ((oh % b) * b + ow % b) * OQ + q;  // channels k C' + 4 q ..
      y = oh / b;
      x = ow / b;
    } else {
      const int k = q / IQ;  // output channels 4 q .. = k C + 4 (q % IQ) ..
      sq = q % IQ;
      y = oh * b + k / b;
      x = ow * b + k % b;
    }
    Y[e] = X[quad_at(n, sq, y, x, IQ, g.H, g.W)];
  }
}

// channel-major with b = B (2 or 4), both tensors in channel quads.  L = the spatially larger tensor [LQ quads, b SH, b SW], S = the smaller one
// [b^2 LQ * 4 channels, SH, SW].  A unit is (n, q of LQ, h, w) for B = 2 and (n, q, i, h, w) for B = 4, w fastest: it pairs the four quads
// B^2 q + (B^2 / 4) r + i (r = 0..3; i = 0 for B = 2) of S at pixel (h, w) with quad q of L at the four pixels (B = 2) of the 2 x 2 block, or
// (B = 4) at the four pixels of row i of the 4 x 4 block: element r of L's quad at pixel p is element p of S's quad r.
template <int B, bool TO_SPACE>
__global__ __launch_bounds__(kBlock) void pixelshuffle_transpose_kernel(const f32x4 *__restrict__ X, f32x4 *__restrict__ Y, int64_t total, int LQ, int SH, int SW) {
  constexpr int I = B == 4 ? 4 : 1;
  const int LH = B * SH, LW = B * SW, SQ = B * B * LQ;
  for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < total; e += int64_t(gridDim.x) * kBlock) {
    const int w = int(e % SW);
    int64_t t = e / SW;
    const int h = int(t % SH);
    t /= SH;
    const int i = int(t % I);
    t /= I;
    const int q = int(t % LQ);
    const int64_t n = t / LQ;
    int64_t s_at[4], l_at[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      s_at[r] = quad_at(n, B * B * q + (B * B / 4) * r + i, h, w, SQ, SH, SW);
      l_at[r] = B == 2 ? quad_at(n, q, 2 * h + (r >> 1), 2 * w + (r & 1), LQ, LH, LW) : quad_at(n, q, 4 * h + i, 4 * w + r, LQ, LH, LW);
    }
    f32x4 m[4];
#pragma unroll
    for (int r = 0; r < 4; r++) m[r] = X[TO_SPACE ? s_at[r] : l_at[r]];
#pragma unroll
    for (int p = 0; p < 4; p++) Y[TO_SPACE ? l_at[p] : s_at[p]] = f32x4{m[0][p], m[1][p], m[2][p], m[3][p]};
  }
}

// channel quads in, NCHW out: total = rows * C / 4 * H * W input quads.  MODE 2 / 4: depth to space, channel-major, b = 2 / 4; 0: any form
template <int MODE>
__global__ __launch_bounds__(kBlock) void pixelshuffle_cq_to_nchw_kernel(const f32x4 *__restrict__ X, float *__restrict__ Y, int64_t total, PixelShuffleGeom g) {
  const int IQ = g.C / 4;
  for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < total; e += int64_t(gridDim.x) * kBlock) {
    const int x = int(e % g.W);
    int64_t t = e / g.W;
    const int y = int(t % g.H);
    t /= g.H;
    const int q = int(t % IQ);
    const int64_t n = t / IQ;
    const f32x4 v = X[e];
    if constexpr (MODE == 2) {  // channels 4 q + 2 i + j: the 2 x 2 block of output channel q
      const int64_t o = nchw_at(n, q, 2 * y, 2 * x, g.OC, g.OH, g.OW);
      *reinterpret_cast<f32x2 *>(Y + o) = f32x2{v[0], v[1]};
      *reinterpret_cast<f32x2 *>(Y + o + g.OW) = f32x2{v[2], v[3]};
    } else if constexpr (MODE == 4) {  // channels 16 c + 4 i + j with 4 c + i = q: row i of the 4 x 4 block of output channel c
      *reinterpret_cast<f32x4 *>(Y + nchw_at(n, q >> 2, 4 * y + (q & 3), 4 * x, g.OC, g.OH, g.OW)) = v;
    } else {
      for (int k = 0; k < 4; k++) {
        int oc, oh, ow;
        dest_of(g, 4 * q + k, y, x, oc, oh, ow);
        Y[nchw_at(n, oc, oh, ow, g.OC, g.OH, g.OW)] = v[k];
      }
    }
  }
}

// NCHW in, channel quads out, space to depth, channel-major, b = 2: output quad q at (oh, ow) is the 2 x 2 block of input channel q.
// total = rows * OC / 4 * OH * OW output quads.  (Every other form of this crossing is the generic kernel's gather.)
__global__ __launch_bounds__(kBlock) void pixelshuffle_nchw_to_cq2_kernel(const float *__restrict__ X, f32x4 *__restrict__ Y, int64_t total, PixelShuffleGeom g) {
  const int OQ = g.OC / 4;
  for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < total; e += int64_t(gridDim.x) * kBlock) {
    const int ow = int(e % g.OW);
    int64_t t = e / g.OW;
    const int oh = int(t % g.OH);
    t /= g.OH;
    const int q = int(t % OQ);
    const int64_t n = t / OQ;
    const int64_t o = nchw_at(n, q, 2 * oh, 2 * ow, g.C, g.H, g.W);
    const f32x2 a = *reinterpret_cast<const f32x2 *>(X + o), c = *reinterpret_cast<const f32x2 *>(X + o + g.W);
    Y[e] = f32x4{a[0], a[1], c[0], c[1]};
  }
}

inline bool aligned(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

}  // namespace

bool pixel_shuffle(hipStream_t s, const float *X, float *Y, int64_t rows, const PixelShuffleGeom &g, int kernel, bool in_cq, bool out_cq) {
  const int b = g.b;
  // what every form relies on: the two shapes belong to one another, channel-quad tensors hold whole quads and their planes start on 16 bytes
  if (b < 1 || g.C < 1 || g.H < 1 || g.W < 1 || (g.to_space ? g.C != int64_t(g.OC) * b * b || g.OH != g.H * b || g.OW != g.W * b
                                                            : g.OC != int64_t(g.C) * b * b || g.H != g.OH * b || g.W != g.OW * b))
    return false;
  if ((in_cq && (g.C % 4 != 0 || !aligned(X, 16))) || (out_cq && (g.OC % 4 != 0 || !aligned(Y, 16)))) return false;
  const int64_t in_units = rows * (in_cq ? g.C / 4 : g.C) * g.H * g.W, out_units = rows * (out_cq ? g.OC / 4 : g.OC) * g.OH * g.OW;
  if (out_units <= 0) return true;
  auto grid_of = [](int64_t total) { return dim3(unsigned(std::min<int64_t>((total + kBlock - 1) / kBlock, 65536))); };
  auto *X4 = reinterpret_cast<const f32x4 *>(X);
  auto *Y4 = reinterpret_cast<f32x4 *>(Y);
  const int small = g.to_space ? g.OC : g.C;  // the channels of the spatially larger tensor
  if (kernel == kPixelShuffleQuadCopy && in_cq && out_cq && !g.channel_major && small % 4 == 0) {
    hipLaunchKernelGGL(pixelshuffle_quad_copy_kernel, grid_of(out_units), dim3(kBlock), 0, s, X4, Y4, out_units, g);
  } else if (kernel == kPixelShuffleTranspose && in_cq && out_cq && g.channel_major && (b == 2 || b == 4)) {
    const int LQ = small / 4, SH = g.to_space ? g.H : g.OH, SW = g.to_space ? g.W : g.OW;
    const int64_t total = rows * LQ * (b == 4 ? 4 : 1) * SH * SW;
    if (b == 2 && g.to_space) hipLaunchKernelGGL((pixelshuffle_transpose_kernel<2, true>), grid_of(total), dim3(kBlock), 0, s, X4, Y4, total, LQ, SH, SW);
    else if (b == 2) hipLaunchKernelGGL((pixelshuffle_transpose_kernel<2, false>), grid_of(total), dim3(kBlock), 0, s, X4, Y4, total, LQ, SH, SW);
    else if (g.to_space) hipLaunchKernelGGL((pixelshuffle_transpose_kernel<4, true>), grid_of(total), dim3(kBlock), 0, s, X4, Y4, total, LQ, SH, SW);
    else hipLaunchKernelGGL((pixelshuffle_transpose_kernel<4, false>), grid_of(total), dim3(kBlock), 0, s, X4, Y4, total, LQ, SH, SW);
  } else if (kernel == kPixelShuffleCqToNchw && in_cq && !out_cq) {
    const bool crd = g.to_space && g.channel_major;
    if (crd && b == 2 && aligned(Y, 8)) hipLaunchKernelGGL(pixelshuffle_cq_to_nchw_kernel<2>, grid_of(in_units), dim3(kBlock), 0, s, X4, Y, in_units, g);
    else if (crd && b == 4 && aligned(Y, 16)) hipLaunchKernelGGL(pixelshuffle_cq_to_nchw_kernel<4>, grid_of(in_units), dim3(kBlock), 0, s, X4, Y, in_units, g);
    else hipLaunchKernelGGL(pixelshuffle_cq_to_nchw_kernel<0>, grid_of(in_units), dim3(kBlock), 0, s, X4, Y, in_units, g);
  } else if (kernel == kPixelShuffleNchwToCq && !in_cq && out_cq && !g.to_space && g.channel_major && b == 2 && aligned(X, 8)) {
    hipLaunchKernelGGL(pixelshuffle_nchw_to_cq2_kernel, grid_of(out_units), dim3(kBlock), 0, s, X, Y4, out_units, g);
  } else if (kernel == kPixelShuffleGeneric || kernel == kPixelShuffleNchwToCq) {
    if (in_cq && out_cq) hipLaunchKernelGGL((pixelshuffle_generic_kernel<true, true>), grid_of(out_units), dim3(kBlock), 0, s, X, Y, out_units, g);
    else if (in_cq) hipLaunchKernelGGL((pixelshuffle_generic_kernel<true, false>), grid_of(out_units), dim3(kBlock), 0, s, X, Y, out_units, g);
    else if (out_cq) hipLaunchKernelGGL((pixelshuffle_generic_kernel<false, true>), grid_of(out_units), dim3(kBlock), 0, s, X, Y, out_units, g);
    else hipLaunchKernelGGL((pixelshuffle_generic_kernel<false, false>), grid_of(out_units), dim3(kBlock), 0, s, X, Y, out_units, g);
  } else {
    return false;  // (a form chosen for other layouts than these)
  }
  return true;
}

}  // namespace infera_hip::kern
