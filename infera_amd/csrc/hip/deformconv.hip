// deformconv.hip -- deformable convolutions (DeformConv, DCNv1 and the modulated DCNv2) on [N,C,H,W] tensors (DeformConv2d steps,
// host/plan.hpp; host/deformconv.hpp has the coordinate function and the split; INTEGRATION.md 2.6 "Deformable convolutions" the contract;
// DESIGN.md 3.27 the design).
//
//   * deformconv_mfma_kernel -- group == 1, kh * kw <= kDeformMaxTaps.  A deformable convolution is an im2col whose column is SAMPLED: the
//     column of an output position does not depend on the output channel, so it is sampled once and multiplied against all M filters.
//     A work group owns ONE image and a tile of kDeformTilePos = 32 output positions; its waves (up to four) own 32-wide tiles of M, PW
//     tiles each, so one sampled column feeds up to 512 output channels (blockIdx.y walks M beyond that).
//     k = c * taps + tap is walked in chunks of kDeformChunk = 8 channels x all taps, two phases per chunk:
//       sample    the lanes cover the (channel quad, tap, position) items of the chunk, position fastest.  A lane reads its tap's offset
//                 pair and mask, computes the DeformTap -- four corner offsets, in-bounds flags, weights -- ONCE (again only where the
//                 offset group changes inside its quad) and walks the quad's channels with it: NCHW one scalar load per corner and
//                 channel, channel quads one 16-byte load per corner for all four.  It writes col[(c, tap)][position] into LDS: k-major
//                 rows of 32 positions, so 32 neighbouring lanes write one row, and the multiply phase's B operand -- lane (r, h) reads
//                 row 2 kp + h, column r -- is 64 consecutive floats per instruction: no bank conflicts either way.
//       multiply  A = the weights in lane order (deformconv_pack: one coalesced 256-byte fragment per k-pair and M tile, zero beyond K
//                 and M), B from LDS, on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation).
//     Every output is ONE chain of fmas in k order from 0, then + bias, then the activation; its bits depend on its own image alone.
//     The column tile is single-buffered (DESIGN.md 3.27 says why the double-buffered form was not kept).
//   * deformconv_generic_kernel -- everything else (group > 1, more taps than the cap, INFERA_DEFORMCONV_MFMA=0): one lane per output
//     element, an fmaf chain in (c, i, j) order over the same coordinate function; every sample is repeated for each output channel.
// X and Y lie in NCHW or in channel quads [N, C/4, H, W, 4] independently (template forms); the offset and mask tensors in either, by a
// launch flag.  Contraction is off for the whole file: a sample is the contract's sequence of separately rounded operations.
#pragma clang fp contract(off)  // (before every include: kernels.hpp brings host/deformconv.hpp in with it)

#include "device_common.hpp"

#include "../host/deformconv.hpp"

namespace infera_hip::kern {

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7FC00000u); }

// element (n, ch, p) of an [N, CH, OH, OW] tensor with OP = OH * OW positions per plane, in either layout
__device__ __forceinline__ int64_t at(bool cq, int64_t n, int CH, int ch, int64_t OP, int64_t p) {
  return cq ? ((n * (CH >> 2) + (ch >> 2)) * OP + p) * 4 + (ch & 3) : (n * CH + ch) * OP + p;
}

// what one (offset group, tap, position) reads: the offset pair, the mask, the corners
struct TapRead {
  DeformTap t;
  float mask;
};
__device__ __forceinline__ TapRead read_tap(const float *__restrict__ Off, const float *__restrict__ Mask, const DeformGeom &g, int flags, int64_t n, int og,
                                           int tap, int oh, int ow, int64_t OP, int64_t p) {
  const int taps = g.kh * g.kw, i = tap / g.kw, j = tap - i * g.kw;
  const int ch = (og * taps + tap) * 2, CH = g.ogroups * taps * 2;
  const bool ocq = (flags & kDeformOffCq) != 0;
  const float oy = Off[at(ocq, n, CH, ch, OP, p)], ox = Off[at(ocq, n, CH, ch + 1, OP, p)];
  TapRead r;
  r.t = deform_tap(oh * g.sh - g.pt + i * g.dh, ow * g.sw - g.pl + j * g.dw, oy, ox, g.H, g.W);
  r.mask = g.has_mask ? Mask[at((flags & kDeformMaskCq) != 0, n, g.ogroups * taps, og * taps + tap, OP, p)] : 1.f;
  return r;
}

// one channel's sample; `x` = the channel's plane (NCHW) or its quad plane + the lane inside the quad, stride 4 (channel quads)
template <bool X_CQ>
__device__ __forceinline__ float sample(const float *__restrict__ x, const TapRead &r) {
  if (r.t.nan) return quiet_nan();
  constexpr int S = X_CQ ? 4 : 1;
  const float v00 = (r.t.inside & 1u) ? x[int64_t(r.t.off[0]) * S] : 0.f, v01 = (r.t.inside & 2u) ? x[int64_t(r.t.off[1]) * S] : 0.f;
  const float v10 = (r.t.inside & 4u) ? x[int64_t(r.t.off[2]) * S] : 0.f, v11 = (r.t.inside & 8u) ? x[int64_t(r.t.off[3]) * S] : 0.f;
  return deform_blend(r.t, v00, v01, v10, v11, r.mask);
}

template <int PW, bool X_CQ, bool Y_CQ>
__global__ __launch_bounds__(kBlock) void deformconv_mfma_kernel(const float *__restrict__ X, const float *__restrict__ Off, const float *__restrict__ Mask,
                                                                const float *__restrict__ Wp, const float *__restrict__ bias, float *__restrict__ Y, int tiles,
                                                                DeformGeom g, DeformSplit sp, int flags, ActParam act) {
  extern __shared__ __attribute__((aligned(16))) float col[];  // [kDeformChunk * taps][32]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = blockDim.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t n = blockIdx.x / tiles;
  const int p0 = int(blockIdx.x - n * tiles) * kDeformTilePos;
  const int64_t OP = int64_t(g.OH) * g.OW, IP = int64_t(g.H) * g.W;
  const int taps = sp.taps, Cog = g.C / g.ogroups, mtiles = sp.Mp / 32;
  const int64_t pairs = sp.Kp / 2;
  const int mt0 = (blockIdx.y * nwaves + wave) * PW;  // this wave's first M tile

  f32x16 acc[PW];
#pragma unroll
  for (int t = 0; t < PW; t++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc[t][i] = 0.f;

  for (int chunk = 0; chunk < sp.chunks; chunk++) {
    const int c0 = chunk * kDeformChunk, nch = g.C - c0 < kDeformChunk ? g.C - c0 : kDeformChunk, rows = nch * taps;
    if (chunk) __syncthreads();  // (everyone has read the previous chunk's columns)
    // ---- sample: item = (quad of the chunk, tap, position), position fastest ----
    const int quads = (nch + 3) >> 2;
    for (int q = threadIdx.x; q < quads * taps * 32; q += blockDim.x) {
      const int pos = q & 31, rest = q >> 5, hq = rest / taps, tap = rest - hq * taps;
      const int64_t p = int64_t(p0) + pos;
      const int cq0 = c0 + 4 * hq, nq = g.C - cq0 < 4 ? g.C - cq0 : 4;
      float *dst = col + ((4 * hq) * taps + tap) * 32 + pos;
      if (p >= OP) {
        for (int j = 0; j < nq; j++) dst[j * taps * 32] = 0.f;
        continue;
      }
      const int oh = int(p / g.OW), ow = int(p - int64_t(oh) * g.OW);
      int og = cq0 / Cog;
      TapRead tr = read_tap(Off, Mask, g, flags, n, og, tap, oh, ow, OP, p);
      if (X_CQ && (cq0 + 3) / Cog == og) {  // the whole quad under one offset group: one 16-byte load per corner
        const f32x4 *x4 = reinterpret_cast<const f32x4 *>(X) + (n * (g.C >> 2) + (cq0 >> 2)) * IP;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const f32x4 v00 = (tr.t.inside & 1u) ? x4[tr.t.off[0]] : zero, v01 = (tr.t.inside & 2u) ? x4[tr.t.off[1]] : zero;
        const f32x4 v10 = (tr.t.inside & 4u) ? x4[tr.t.off[2]] : zero, v11 = (tr.t.inside & 8u) ? x4[tr.t.off[3]] : zero;
#pragma unroll
        for (int j = 0; j < 4; j++) dst[j * taps * 32] = tr.t.nan ? quiet_nan() : deform_blend(tr.t, v00[j], v01[j], v10[j], v11[j], tr.mask);
        continue;
      }
      for (int j = 0; j < nq; j++) {
        const int c = cq0 + j;
        if (c / Cog != og) og = c / Cog, tr = read_tap(Off, Mask, g, flags, n, og, tap, oh, ow, OP, p);
        const float *x = X_CQ ? X + (n * (g.C >> 2) + (c >> 2)) * IP * 4 + (c & 3) : X + (n * g.C + c) * IP;
        dst[j * taps * 32] = sample<X_CQ>(x, tr);
      }
    }
    if ((rows & 1) && threadIdx.x < 32) col[rows * 32 + threadIdx.x] = 0.f;  // (the last k-pair's second row: K is odd)
    __syncthreads();
    // ---- multiply: this wave's PW tiles of M against the chunk's columns ----
    if (mt0 >= mtiles) continue;
    const int64_t kp0 = int64_t(c0) * taps / 2;
    const int npairs = (rows + 1) >> 1;
    const float *b = col + h * 32 + r;
    for (int kp = 0; kp < npairs; kp++) {
      const float bv = b[kp * 64];
#pragma unroll
      for (int t = 0; t < PW; t++) {
        const int mt = mt0 + t < mtiles ? mt0 + t : mtiles - 1;  // (a tile beyond the last repeats it and is not stored)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(Wp[(mt * pairs + kp0 + kp) * 64 + lane], bv, acc[t], 0, 0, 0);
      }
    }
  }
  // lane (r, h) holds position p0 + r, channels 32 mt + 8 q + 4 h + j of each of its tiles: bias, the activation resolved once, the stores
  const int64_t p = int64_t(p0) + r;
#pragma unroll
  for (int t = 0; t < PW; t++) {
    const int mt = mt0 + t;
    if (mt >= mtiles) break;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[t][i] += bias[mt * 32 + 8 * (i >> 2) + 4 * h + (i & 3)];  // (Mp entries)
    dispatch_act(act.kind, [&](auto kind_tag) {
      constexpr int KIND = decltype(kind_tag)::value;
#pragma unroll
      for (int i = 0; i < 16; i++) acc[t][i] = apply_act_c<KIND>(acc[t][i], act.a, act.b);
    });
    if (p >= OP) continue;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int m = mt * 32 + 8 * q + 4 * h;
      if constexpr (Y_CQ) {  // (M is whole quads: a quad is inside M or beyond it)
        if (m < g.M) reinterpret_cast<f32x4 *>(Y)[(n * (g.M >> 2) + (m >> 2)) * OP + p] = f32x4{acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]};
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (m + j < g.M) Y[(n * g.M + m + j) * OP + p] = acc[t][4 * q + j];
      }
    }
  }
}

template <bool X_CQ>
__global__ __launch_bounds__(kBlock) void deformconv_generic_kernel(const float *__restrict__ X, const float *__restrict__ Off, const float *__restrict__ Mask,
                                                                   const float *__restrict__ W, const float *__restrict__ bias, float *__restrict__ Y, int64_t total,
                                                                   DeformGeom g, int flags, ActParam act) {
  const int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= total) return;
  const int64_t OP = int64_t(g.OH) * g.OW, IP = int64_t(g.H) * g.W;
  const int Cg = g.C / g.groups, Mg = g.M / g.groups, Cog = g.C / g.ogroups, taps = g.kh * g.kw;
  const int64_t nm = e / OP, n = nm / g.M, p = e - nm * OP;
  const int m = int(nm - n * g.M), oh = int(p / g.OW), ow = int(p - int64_t(oh) * g.OW);
  const float *w = W + int64_t(m) * Cg * taps;
  float acc = 0.f;
  for (int cl = 0; cl < Cg; cl++) {
    const int c = (m / Mg) * Cg + cl;
    const float *x = X_CQ ? X + (n * (g.C >> 2) + (c >> 2)) * IP * 4 + (c & 3) : X + (n * g.C + c) * IP;
    for (int tap = 0; tap < taps; tap++) {
      const TapRead tr = read_tap(Off, Mask, g, flags, n, c / Cog, tap, oh, ow, OP, p);
      acc = fmaf(sample<X_CQ>(x, tr), w[cl * taps + tap], acc);
    }
  }
  Y[at((flags & kDeformYcq) != 0, n, g.M, m, OP, p)] = apply_act(acc + (bias ? bias[m] : 0.f), act);
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// what both kernels rely on: extents whose base positions and plane offsets stay in int and are f32 values, whole groups, whole quads on a
// channel-quad tensor
bool served(const DeformGeom &g, int flags, const float *X, const float *Off, const float *Mask, const float *Y) {
  const int64_t lim = int64_t(1) << 20, lim31 = int64_t(1) << 31;
  if (g.C < 1 || g.M < 1 || g.H < 1 || g.W < 1 || g.OH < 1 || g.OW < 1 || g.kh < 1 || g.kw < 1 || g.sh < 1 || g.sw < 1 || g.dh < 1 || g.dw < 1 || g.pt < 0 || g.pl < 0) return false;
  if (g.kh > kDeformMaxKernel || g.kw > kDeformMaxKernel || g.H > lim || g.W > lim || g.sh > lim || g.sw > lim || g.dh > lim || g.dw > lim || g.pt > lim || g.pl > lim) return false;
  if (int64_t(g.OH - 1) * g.sh > 3 * lim || int64_t(g.OW - 1) * g.sw > 3 * lim || int64_t(g.kh - 1) * g.dh > 3 * lim || int64_t(g.kw - 1) * g.dw > 3 * lim) return false;
  if (g.groups < 1 || g.ogroups < 1 || g.C % g.groups || g.M % g.groups || g.C % g.ogroups) return false;
  const int64_t taps = int64_t(g.kh) * g.kw;
  if (int64_t(g.C) * g.H * g.W >= lim31 || int64_t(g.M) * g.OH * g.OW >= lim31 || g.ogroups * taps * 2 * g.OH * g.OW >= lim31) return false;
  if ((flags & kDeformXcq) && (g.C % 4 || !aligned16(X))) return false;
  if ((flags & kDeformYcq) && (g.M % 4 || !aligned16(Y))) return false;
  if ((flags & kDeformOffCq) && ((g.ogroups * taps * 2) % 4 || !aligned16(Off))) return false;
  if ((flags & kDeformMaskCq) && g.has_mask && ((g.ogroups * taps) % 4 || !aligned16(Mask))) return false;
  return !g.has_mask || Mask != nullptr;
}

template <int PW>
void launch_mfma(hipStream_t s, dim3 grid, dim3 block, const DeformSplit &sp, const float *X, const float *Off, const float *Mask, const float *Wp, const float *bias,
                 float *Y, int tiles, const DeformGeom &g, int flags, ActParam act) {
  const size_t lds = size_t(sp.lds_bytes);
  const bool xq = flags & kDeformXcq, yq = flags & kDeformYcq;
  if (xq && yq) hipLaunchKernelGGL((deformconv_mfma_kernel<PW, true, true>), grid, block, lds, s, X, Off, Mask, Wp, bias, Y, tiles, g, sp, flags, act);
  else if (xq) hipLaunchKernelGGL((deformconv_mfma_kernel<PW, true, false>), grid, block, lds, s, X, Off, Mask, Wp, bias, Y, tiles, g, sp, flags, act);
  else if (yq) hipLaunchKernelGGL((deformconv_mfma_kernel<PW, false, true>), grid, block, lds, s, X, Off, Mask, Wp, bias, Y, tiles, g, sp, flags, act);
  else hipLaunchKernelGGL((deformconv_mfma_kernel<PW, false, false>), grid, block, lds, s, X, Off, Mask, Wp, bias, Y, tiles, g, sp, flags, act);
}

}  // namespace

size_t deformconv_packed_floats(const DeformGeom &g) {
  const DeformSplit sp = deform_split(g);
  return size_t(sp.Mp) * size_t(sp.Kp);
}
void deformconv_pack(const DeformGeom &g, const float *W, float *packed) {
  const DeformSplit sp = deform_split(g);
  const int64_t pairs = sp.Kp / 2;
  for (int mt = 0; mt < sp.Mp / 32; mt++)
    for (int64_t kp = 0; kp < pairs; kp++)
      for (int lane = 0; lane < 64; lane++) {
        const int m = mt * 32 + (lane & 31);
        const int64_t k = 2 * kp + (lane >> 5);  // (= c * taps + tap: the order of the ONNX weights [M, C, kh, kw])
        packed[(mt * pairs + kp) * 64 + lane] = m < g.M && k < sp.K ? W[int64_t(m) * sp.K + k] : 0.f;
      }
}

bool deformconv_mfma(hipStream_t s, const float *X, const float *Off, const float *Mask, const float *Wp, const float *bias, float *Y, int64_t rows, const DeformGeom &g,
                     int flags, ActParam act) {
  if (!served(g, flags, X, Off, Mask, Y) || !deform_takes_mfma(g, true)) return false;
  if (rows < 1) return true;
  const DeformSplit sp = deform_split(g);
  const int64_t tiles = (int64_t(g.OH) * g.OW + kDeformTilePos - 1) / kDeformTilePos;
  if (tiles * rows > INT32_MAX || sp.zblocks > 65535) return false;
  const dim3 grid(unsigned(tiles * rows), unsigned(sp.zblocks)), block(unsigned(64 * sp.waves));
  if (sp.per_wave == 1) launch_mfma<1>(s, grid, block, sp, X, Off, Mask, Wp, bias, Y, int(tiles), g, flags, act);
  else if (sp.per_wave == 2) launch_mfma<2>(s, grid, block, sp, X, Off, Mask, Wp, bias, Y, int(tiles), g, flags, act);
  else launch_mfma<4>(s, grid, block, sp, X, Off, Mask, Wp, bias, Y, int(tiles), g, flags, act);
  return true;
}

bool deformconv_generic(hipStream_t s, const float *X, const float *Off, const float *Mask, const float *W, const float *bias, float *Y, int64_t rows,
                        const DeformGeom &g, int flags, ActParam act) {
  if (!served(g, flags, X, Off, Mask, Y)) return false;
  const int64_t total = rows * g.M * g.OH * g.OW;
  if (total <= 0) return true;
  const int64_t blocks = (total + kBlock - 1) / kBlock;
  if (blocks > INT32_MAX) return false;
  if (flags & kDeformXcq) hipLaunchKernelGGL(deformconv_generic_kernel<true>, dim3(unsigned(blocks)), dim3(kBlock), 0, s, X, Off, Mask, W, bias, Y, total, g, flags, act);
  else hipLaunchKernelGGL(deformconv_generic_kernel<false>, dim3(unsigned(blocks)), dim3(kBlock), 0, s, X, Off, Mask, W, bias, Y, total, g, flags, act);
  return true;
}

}  // namespace infera_hip::kern
