// deconv.hip -- transposed convolution (ONNX ConvTranspose) by stride phases.
//
// Output pixel (oh, ow) belongs to phase (ph, pw) = ((oh + pt) mod sh, (ow + pl) mod sw).  Only the taps with ky * dh == ph (mod sh) and
// kx * dw == pw (mod sw) reach it, from input pixel ih = (oh + pt - ky * dh) / sh, iw likewise: each phase is a stride-1 convolution of the
// input with a sub-filter, so no multiply is spent on the zeros a "dilate the input, then convolve" formulation inserts.  The per-axis tap
// lists are built at load (host/deconv.cpp) and read here as one int table:
//     row phase ph   : tab[ph * h_stride + ...]                  = out0, count, taps, (ky, q) x taps     (ih = index in phase + q)
//     column phase pw: tab[sh * h_stride + pw * w_stride + ...]  = the same with kx
//     (phase kernel only) behind both: the float offset of each phase's weight fragments, in units of 256 floats
//
//   * convt2d_phase_kernel   -- groups == 1, channel-quad input: the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32 in the transposed
//     form of conv.hip, Out^T[m, p] = sum_k Wt[m, k] * col[k, p], with p the pixels of ONE phase (over all rows of the pass) and
//     k = (tap of the phase ascending in (ky, kx), channel group of 8 ascending).  A workgroup = 4 waves = 128 pixels of a phase x MT * 32
//     features; the phase is blockIdx.y, so one launch covers the layer.  Weights are packed fragment-major per phase at load (C padded to 8,
//     M to 32 with zero weights): every A operand is one coalesced 16-byte load per lane, shared by the workgroup's waves through L1 / L2.  A tap
//     that leaves the image is not branched on: its gather is redirected to the tensor's first quad and the value replaced by zero.
//     The order of the sum of an output element is (tap, channel group, the four k pairs of the group): it depends on the model alone, so
//     a row gives the bits it gives in any batch, and the two output layouts give the same bits.
//   * convt2d_generic_kernel -- any group count, NCHW or channel-quad on either side, any C: one output element per thread on the VALU,
//     an fmaf chain over (tap ascending, channel ascending).  The correctness floor, and what serves the forms the phase kernel excludes.
#include "device_common.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace infera_hip::kern {

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ int64_t act_index(bool cq, int64_t n, int c, int y, int x, int C, int H, int W) {
  return cq ? (((n * (C >> 2) + (c >> 2)) * H + y) * W + x) * 4 + (c & 3) : ((n * C + c) * H + y) * int64_t(W) + x;
}

__global__ __launch_bounds__(kBlock) void convt2d_generic_kernel(const float *__restrict__ X, const float *__restrict__ Wg, const float *__restrict__ bias,
                                                                float *__restrict__ Y, const int *__restrict__ tab, int64_t total, ConvTGeom g,
                                                                ActParam act, bool in_cq, bool out_cq) {
  const int Cg = g.C / g.groups, Mg = g.M / g.groups;
  for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < total; e += int64_t(gridDim.x) * kBlock) {
    int64_t n, t;
    int m, oh, ow;
    if (out_cq) {  // [N][M/4][OH][OW][4]
      t = e >> 2;
      ow = int(t % g.OW), t /= g.OW;
      oh = int(t % g.OH), t /= g.OH;
      m = int(t % (g.M >> 2)) * 4 + int(e & 3);
      n = t / (g.M >> 2);
    } else {
      ow = int(e % g.OW), t = e / g.OW;
      oh = int(t % g.OH), t /= g.OH;
      m = int(t % g.M);
      n = t / g.M;
    }
    const int grp = m / Mg, ml = m - grp * Mg;
    const int *hr = tab + ((oh + g.pt) % g.sh) * g.h_stride;
    const int *wr = tab + g.sh * g.h_stride + ((ow + g.pl) % g.sw) * g.w_stride;
    const int jh = (oh - hr[0]) / g.sh, jw = (ow - wr[0]) / g.sw;
    float acc = 0.f;
    for (int a = 0; a < hr[2]; a++) {
      const int ky = hr[3 + 2 * a], ih = jh + hr[4 + 2 * a];
      if (ih < 0 || ih >= g.H) continue;
      for (int b = 0; b < wr[2]; b++) {
        const int kx = wr[3 + 2 * b], iw = jw + wr[4 + 2 * b];
        if (iw < 0 || iw >= g.W) continue;
        const float *w = Wg + (int64_t(ky * g.kw + kx) * g.C + grp * Cg) * Mg + ml;
        for (int c = 0; c < Cg; c++) acc = fmaf(X[act_index(in_cq, n, grp * Cg + c, ih, iw, g.C, g.H, g.W)], w[int64_t(c) * Mg], acc);
      }
    }
    acc += bias ? bias[m] : 0.f;
    Y[e] = apply_act(acc, act);
  }
}

// packed weights of the phase kernel: [phase][tap of the phase][c8 = channel group of 8][mt = M / 32 tiles][lane (64)][j (4)]
//   = W[c = 8 c8 + 4 (lane >> 5) + j][m = 32 mt + (lane & 31)][ky][kx]     (zero beyond C and M)
template <int MT>
__global__ __launch_bounds__(kBlock) void convt2d_phase_kernel(const float *__restrict__ X, const float *__restrict__ Wp, const float *__restrict__ bias,
                                                              float *__restrict__ Y, const int *__restrict__ tab, int64_t rows, ConvTGeom g, ActParam act,
                                                              bool out_cq) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int ph = int(blockIdx.y) / g.sw, pw = int(blockIdx.y) % g.sw;
  const int *hr = tab + ph * g.h_stride;
  const int *wr = tab + g.sh * g.h_stride + pw * g.w_stride;
  const int ohp = hr[1], owp = wr[1], nth = hr[2], ntw = wr[2];
  const int64_t phase_pix = int64_t(ohp) * owp, total = rows * phase_pix;
  if (int64_t(blockIdx.x) * 128 >= total) return;  // (the grid is sized for the largest phase)
  const int64_t p = (int64_t(blockIdx.x) * 4 + wave) * 32 + r;
  const bool pvalid = p < total;
  const int64_t n = pvalid ? p / phase_pix : 0;
  const int prem = pvalid ? int(p % phase_pix) : 0;
  const int jh = prem / owp, jw = prem - jh * owp;
  const int C8 = (g.C + 7) >> 3, MTall = (g.M + 31) >> 5, CQ = g.C >> 2;
  const int mt0 = int(blockIdx.z) * MT;
  const float *xn = X + n * int64_t(g.C) * g.H * g.W;
  const float *wl = Wp + int64_t(tab[g.sh * g.h_stride + g.sw * g.w_stride + int(blockIdx.y)]) * 256 + (int64_t(mt0) * 64 + lane) * 4;

  f32x16 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc[t][i] = 0.f;

  for (int a = 0; a < nth; a++) {
    const int ih = jh + hr[4 + 2 * a];
    const bool hok = pvalid && ih >= 0 && ih < g.H;
    for (int b = 0; b < ntw; b++) {
      const int iw = jw + wr[4 + 2 * b];
      const bool ok = hok && iw >= 0 && iw < g.W;
      const int64_t pix_off = ok ? (int64_t(ih) * g.W + iw) * 4 : 0;
      const float *wt = wl + int64_t(a * ntw + b) * C8 * MTall * 256;
      for (int c8 = 0; c8 < C8; c8++) {
        const int q = 2 * c8 + h;  // this lane half's channel quad
        const bool qok = ok && q < CQ;
        f32x4 bv = *reinterpret_cast<const f32x4 *>(qok ? xn + int64_t(q) * g.H * g.W * 4 + pix_off : X);
        if (!qok) bv = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 av[MT];
#pragma unroll
        for (int t = 0; t < MT; t++) av[t] = *reinterpret_cast<const f32x4 *>(wt + (int64_t(c8) * MTall + t) * 256);
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
          for (int t = 0; t < MT; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t][j], bv[j], acc[t], 0, 0, 0);
      }
    }
  }
  if (!pvalid) return;
  const int oh = hr[0] + jh * g.sh, ow = wr[0] + jw * g.sw;
  // lane (r, h) holds its pixel's channels 32 (mt0 + t) + 8 q + 4 h + j in acc[t][4 q + j]
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int ml = 32 * (mt0 + t) + 8 * (i >> 2) + 4 * h + (i & 3);
      acc[t][i] += (bias && ml < g.M) ? bias[ml] : 0.f;
    }
  dispatch_act(act.kind, [&](auto kind_tag) {
    constexpr int KIND = decltype(kind_tag)::value;
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[t][i] = apply_act_c<KIND>(acc[t][i], act.a, act.b);
  });
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int ml = 32 * (mt0 + t) + 8 * q + 4 * h;
      if (out_cq) {  // (M is whole quads: one 16-byte store per channel quad)
        if (ml + 3 < g.M) {
          f32x4 v;
#pragma unroll
          for (int j = 0; j < 4; j++) v[j] = acc[t][4 * q + j];
          *reinterpret_cast<f32x4 *>(Y + act_index(true, n, ml, oh, ow, g.M, g.OH, g.OW)) = v;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (ml + j < g.M) Y[act_index(false, n, ml + j, oh, ow, g.M, g.OH, g.OW)] = acc[t][4 * q + j];
      }
    }
}

int phase_mt(int M) {
  const int mp = (M + 31) / 32 * 32;
  return mp % 128 == 0 ? 4 : mp % 64 == 0 ? 2 : 1;
}

}  // namespace

void convt2d_generic_pack(const ConvTGeom &g, const float *W, float *packed) {
  const int Mg = g.M / g.groups;
  for (int c = 0; c < g.C; c++)
    for (int ml = 0; ml < Mg; ml++)
      for (int ky = 0; ky < g.kh; ky++)
        for (int kx = 0; kx < g.kw; kx++)
          packed[(size_t(ky * g.kw + kx) * g.C + c) * Mg + ml] = W[((size_t(c) * Mg + ml) * g.kh + ky) * g.kw + kx];
}

void convt2d_generic(hipStream_t s, const float *X, const float *Wg, const float *bias, float *Y, const int *tab, int64_t rows, const ConvTGeom &g,
                     ActParam act, bool in_cq, bool out_cq) {
  const int64_t total = rows * g.M * g.OH * g.OW;
  if (total <= 0) return;
  const int64_t blocks = std::min<int64_t>((total + kBlock - 1) / kBlock, 65536);
  hipLaunchKernelGGL(convt2d_generic_kernel, dim3(unsigned(blocks)), dim3(kBlock), 0, s, X, Wg, bias, Y, tab, total, g, act, in_cq, out_cq);
}

bool convt2d_phase_supported(const ConvTGeom &g, const int32_t *tab) {
  if (g.groups != 1 || g.C % 4 != 0 || g.sh * g.sw > 65535) return false;
  if (int64_t(g.C) * g.H * g.W >= (int64_t(1) << 29) || int64_t(g.M) * g.OH * g.OW >= (int64_t(1) << 29)) return false;
  return convt2d_phase_packed_floats(g, tab) < (size_t(1) << 30);
}

size_t convt2d_phase_packed_floats(const ConvTGeom &g, const int32_t *tab) {
  const size_t C8 = size_t(g.C + 7) / 8, MTall = size_t(g.M + 31) / 32;
  size_t taps = 0;
  for (int ph = 0; ph < g.sh; ph++)
    for (int pw = 0; pw < g.sw; pw++) taps += size_t(tab[ph * g.h_stride + 2]) * size_t(tab[g.sh * g.h_stride + pw * g.w_stride + 2]);
  return std::max<size_t>(taps, 1) * C8 * MTall * 256;
}

void convt2d_phase_pack(const ConvTGeom &g, const int32_t *tab, const float *W, float *packed, int32_t *phase_off) {
  const int C8 = (g.C + 7) / 8, MTall = (g.M + 31) / 32;
  std::memset(packed, 0, convt2d_phase_packed_floats(g, tab) * sizeof(float));
  size_t unit = 0;  // 256-float fragments so far
  for (int ph = 0; ph < g.sh; ph++)
    for (int pw = 0; pw < g.sw; pw++) {
      const int32_t *hr = tab + ph * g.h_stride, *wr = tab + g.sh * g.h_stride + pw * g.w_stride;
      phase_off[ph * g.sw + pw] = int32_t(unit);
      for (int a = 0; a < hr[2]; a++)
        for (int b = 0; b < wr[2]; b++) {
          const int ky = hr[3 + 2 * a], kx = wr[3 + 2 * b];
          for (int c8 = 0; c8 < C8; c8++)
            for (int mt = 0; mt < MTall; mt++, unit++)
              for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 4; j++) {
                  const int c = 8 * c8 + 4 * (lane >> 5) + j, m = 32 * mt + (lane & 31);
                  if (c < g.C && m < g.M) packed[unit * 256 + size_t(lane) * 4 + j] = W[((size_t(c) * g.M + m) * g.kh + ky) * g.kw + kx];
                }
        }
    }
}

void convt2d_phase(hipStream_t s, const float *X, const float *Wp, const float *bias, float *Y, const int *tab, int64_t rows, const ConvTGeom &g,
                   int64_t max_phase_pixels, ActParam act, bool out_cq) {
  const int64_t tiles = (rows * max_phase_pixels + 127) / 128;
  if (tiles <= 0) return;
  const int mt = phase_mt(g.M), mtall = (g.M + 31) / 32;
  const dim3 grid(unsigned(tiles), unsigned(g.sh * g.sw), unsigned(mtall / mt));
  if (mt == 4) hipLaunchKernelGGL(convt2d_phase_kernel<4>, grid, dim3(kBlock), 0, s, X, Wp, bias, Y, tab, rows, g, act, out_cq);
  else if (mt == 2) hipLaunchKernelGGL(convt2d_phase_kernel<2>, grid, dim3(kBlock), 0, s, X, Wp, bias, Y, tab, rows, g, act, out_cq);
  else hipLaunchKernelGGL(convt2d_phase_kernel<1>, grid, dim3(kBlock), 0, s, X, Wp, bias, Y, tab, rows, g, act, out_cq);
}

}  // namespace infera_hip::kern
