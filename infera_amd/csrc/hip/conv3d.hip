// conv3d.hip -- 3-D convolutions and pooling on NCDHW tensors (Conv3d / Pool3d steps, host/plan.hpp).
//
//   * conv3d_mfma_kernel   -- groups == 1: an implicit GEMM on the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32.  The A operand
//     is the weights (32 rows = 32 output channels), the B operand the input (32 columns = 32 consecutive output positions of the
//     flattened (image, od, oh, ow) index), so a lane's results of one channel lie side by side in NCDHW and a wave's store of one
//     channel is one contiguous run.  A work group owns kConv3dTilePos = 64 consecutive positions (two position tiles per wave: every
//     weight fragment feeds two MFMAs) and up to four 32-channel tiles, one per wave (every input value feeds up to four waves); the
//     grid's y axis walks the channel tiles beyond 128.
//     k runs over (channel chunk, kz, ky, kx, channel inside the chunk); a k-pair of the instruction is two neighbouring channels of a
//     chunk at one tap, lane half h takes channel 2j + h.  The weights are packed at load in exactly that order, one coalesced 256-byte
//     fragment per MFMA row ([channel tile][k-pair][lane]), zero beyond K and M.
//     STAGED: per channel chunk the work group stages its input window in LDS once: for every output row (n, od, oh) its positions
//     touch -- counted straight through planes and images, so a tile that straddles them only has more rows -- and every (kz, ky) one
//     padded input line of Wpad floats, zero at the padding, beyond C and beyond the last image.  A tap is then ONE ds_read at
//     lane base + (wave-uniform) tap offset: no bounds test, no division.  Lines that neighbouring output rows share are staged once per
//     row (the price of the flat row count; the window of the 3x3x3 layers is 3.4 to 6 KB per channel chunk row).
//     Direct (!STAGED): the same loop with the B value fetched from global memory under a bounds test per tap.  This is the DEFAULT: it
//     measured 1.5 to 2.7 times faster than the staged form on every 3x3x3 layer of R3D-18 (profiles/r28_conv3d.txt; DESIGN.md 3.25 says
//     why).  INFERA_CONV3D_STAGE=1 stages wherever the window fits kConv3dLdsBudget (the 3x7x7 stem at 112 x 112 does not).
//     Every output value is ONE chain of fmas in k order starting from 0 (zero-padded terms add +0), then + bias, then the activation:
//     its bits depend on its own image's samples alone, and are the same in both variants.
//   * conv3d_generic_kernel -- everything else (groups > 1, depthwise): one output value per thread, taps in (c, kz, ky, kx) order.
//   * pool3d_kernel         -- MaxPool / AveragePool: one output value per thread, taps outside the volume are ignored.
#include <cmath>

#include "../host/conv3d.hpp"
#include "device_common.hpp"

namespace infera_hip::kern {

namespace {

constexpr int kBlock = 256;
inline int grid_for(int64_t work_items) {
  const int64_t b = (work_items + kBlock - 1) / kBlock;
  return int(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

template <int CC, bool STAGED>
__global__ __launch_bounds__(kBlock) void conv3d_mfma_kernel(const float *__restrict__ X, const float *__restrict__ Wp, const float *__restrict__ bias,
                                                            float *__restrict__ Y, int64_t total_pos, int64_t total_rows, Conv3dGeom g, Conv3dSplit sp,
                                                            ActParam act) {
  extern __shared__ __attribute__((aligned(16))) float win[];  // STAGED: [CC][E]
  constexpr int PT = kConv3dTilePos / 32, KP = CC / 2;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = blockDim.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int mt = blockIdx.y * nwaves + wave;
  const bool live = mt * 32 < sp.Mp;  // (a wave beyond the last channel tile only helps staging)
  const int64_t p0 = int64_t(blockIdx.x) * kConv3dTilePos;
  const int OS = g.OD * g.OH * g.OW, DHW = g.D * g.H * g.W;
  const int64_t in_img = int64_t(g.C) * DHW;
  const int64_t R0 = p0 / g.OW;
  const int E = int(sp.E), Wpad = sp.Wpad, kdh = g.kd * g.kh;

  // this lane's two positions: where their taps start in the window (STAGED) or in the image (direct)
  bool pvalid[PT];
  int base[PT], iz0[PT], iy0[PT], ix0[PT];
  const float *xb[PT];
#pragma unroll
  for (int t = 0; t < PT; t++) {
    const int64_t p = p0 + t * 32 + r;
    pvalid[t] = p < total_pos;
    const int64_t R = p / g.OW;
    const int ow = int(p - R * g.OW);
    base[t] = int(R - R0) * kdh * Wpad + ow * g.sw;  // (R - R0 < nR also for p >= total_pos)
    const int64_t n = R / (g.OD * g.OH);
    const int ro = int(R - n * (g.OD * g.OH)), od = ro / g.OH, oh = ro - od * g.OH;
    iz0[t] = od * g.sd - g.pf, iy0[t] = oh * g.sh - g.pt, ix0[t] = ow * g.sw - g.pl;
    xb[t] = X + (pvalid[t] ? n : 0) * in_img;
  }

  f32x16 acc[PT];
#pragma unroll
  for (int t = 0; t < PT; t++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc[t][i] = 0.f;

  for (int chunk = 0; chunk < sp.chunks; chunk++) {
    if constexpr (STAGED) {
      if (chunk) __syncthreads();  // (everyone has read the previous chunk's window)
      const int lines = sp.nR * kdh;
      for (int L = wave; L < lines; L += nwaves) {  // one (output row, kz, ky) line per wave and step: its coordinates are wave-uniform
        const int rr = L / kdh, rem = L - rr * kdh, kz = rem / g.kh, ky = rem - kz * g.kh;
        const int64_t R = R0 + rr;
        const int64_t n = R / (g.OD * g.OH);
        const int ro = int(R - n * (g.OD * g.OH)), od = ro / g.OH, oh = ro - od * g.OH;
        const int iz = od * g.sd - g.pf + kz * g.dd, iy = oh * g.sh - g.pt + ky * g.dh;
        const bool ok = R < total_rows && iz >= 0 && iz < g.D && iy >= 0 && iy < g.H;
        const float *src = X + (ok ? n * in_img + (int64_t(iz) * g.H + iy) * g.W : 0);
#pragma unroll
        for (int cc = 0; cc < CC; cc++) {
          const int c = chunk * CC + cc;
          const bool okc = ok && c < g.C;
          for (int x = lane; x < Wpad; x += 64) {
            const int ix = x - g.pl;
            win[cc * E + L * Wpad + x] = okc && ix >= 0 && ix < g.W ? src[int64_t(c) * DHW + ix] : 0.f;
          }
        }
      }
      __syncthreads();
    }
    if (!live) continue;
    const float *wt = Wp + (int64_t(mt) * (sp.Kp / 2) + int64_t(chunk) * sp.taps * KP) * 64 + lane;
    const int c0 = chunk * CC + h;
    for (int kz = 0; kz < g.kd; kz++)
      for (int ky = 0; ky < g.kh; ky++)
        for (int kx = 0; kx < g.kw; kx++) {
          float a[KP], b[PT][KP];
#pragma unroll
          for (int j = 0; j < KP; j++) a[j] = wt[j * 64];
          wt += KP * 64;
          if constexpr (STAGED) {
            const int toff = (kz * g.kh + ky) * Wpad + kx * g.dw + h * E;
#pragma unroll
            for (int t = 0; t < PT; t++)
#pragma unroll
              for (int j = 0; j < KP; j++) b[t][j] = win[base[t] + toff + 2 * j * E];
          } else {
#pragma unroll
            for (int t = 0; t < PT; t++) {
              const int iz = iz0[t] + kz * g.dd, iy = iy0[t] + ky * g.dh, ix = ix0[t] + kx * g.dw;
              const bool ok = pvalid[t] && iz >= 0 && iz < g.D && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
              const int off = (iz * g.H + iy) * g.W + ix;
#pragma unroll
              for (int j = 0; j < KP; j++) b[t][j] = ok && c0 + 2 * j < g.C ? xb[t][int64_t(c0 + 2 * j) * DHW + off] : 0.f;
            }
          }
#pragma unroll
          for (int j = 0; j < KP; j++)
#pragma unroll
            for (int t = 0; t < PT; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[t][j], acc[t], 0, 0, 0);
        }
  }
  if (!live) return;
  // lane (r, h) holds position p0 + 32 t + r, channels 32 mt + 8 q + 4 h + j: bias, the activation resolved once, then the stores
  float bv[16];
#pragma unroll
  for (int i = 0; i < 16; i++) bv[i] = bias[mt * 32 + 8 * (i >> 2) + 4 * h + (i & 3)];  // (Mp entries)
#pragma unroll
  for (int t = 0; t < PT; t++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc[t][i] += bv[i];
  dispatch_act(act.kind, [&](auto kind_tag) {
    constexpr int KIND = decltype(kind_tag)::value;
#pragma unroll
    for (int t = 0; t < PT; t++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[t][i] = apply_act_c<KIND>(acc[t][i], act.a, act.b);
  });
#pragma unroll
  for (int t = 0; t < PT; t++) {
    if (!pvalid[t]) continue;
    const int64_t p = p0 + t * 32 + r, n = p / OS;
    float *y = Y + n * int64_t(g.M) * OS + (p - n * OS);
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int m = mt * 32 + 8 * (i >> 2) + 4 * h + (i & 3);
      if (m < g.M) y[int64_t(m) * OS] = acc[t][i];
    }
  }
}

__global__ __launch_bounds__(kBlock) void conv3d_generic_kernel(const float *__restrict__ X, const float *__restrict__ W, const float *__restrict__ bias,
                                                               float *__restrict__ Y, int64_t total, Conv3dGeom g, ActParam act) {
  const int Cg = g.C / g.groups, Mg = g.M / g.groups, OS = g.OD * g.OH * g.OW, DHW = g.D * g.H * g.W, taps = g.kd * g.kh * g.kw;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t o = int64_t(blockIdx.x) * kBlock + threadIdx.x; o < total; o += stride) {
    const int64_t nm = o / OS, n = nm / g.M;
    const int s = int(o - nm * OS), m = int(nm - n * g.M);
    const int od = s / (g.OH * g.OW), so = s - od * (g.OH * g.OW), oh = so / g.OW, ow = so - oh * g.OW;
    const float *x = X + (n * g.C + int64_t(m / Mg) * Cg) * DHW;
    const float *w = W + int64_t(m) * Cg * taps;
    float acc = 0.f;
    for (int c = 0; c < Cg; c++)
      for (int kz = 0; kz < g.kd; kz++) {
        const int iz = od * g.sd - g.pf + kz * g.dd;
        for (int ky = 0; ky < g.kh; ky++) {
          const int iy = oh * g.sh - g.pt + ky * g.dh;
          for (int kx = 0; kx < g.kw; kx++) {
            const int ix = ow * g.sw - g.pl + kx * g.dw;
            if (iz < 0 || iz >= g.D || iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) continue;
            acc = fmaf(x[int64_t(c) * DHW + (iz * g.H + iy) * g.W + ix], w[(c * g.kd + kz) * g.kh * g.kw + ky * g.kw + kx], acc);
          }
        }
      }
    Y[o] = apply_act(acc + (bias ? bias[m] : 0.f), act);
  }
}

__global__ __launch_bounds__(kBlock) void pool3d_kernel(const float *__restrict__ X, float *__restrict__ Y, int64_t total, Conv3dGeom g, bool is_max,
                                                       bool count_pad) {
  const int OS = g.OD * g.OH * g.OW, DHW = g.D * g.H * g.W;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t o = int64_t(blockIdx.x) * kBlock + threadIdx.x; o < total; o += stride) {
    const int64_t nc = o / OS;
    const int s = int(o - nc * OS);
    const int od = s / (g.OH * g.OW), so = s - od * (g.OH * g.OW), oh = so / g.OW, ow = so - oh * g.OW;
    const float *x = X + nc * DHW;
    float acc = is_max ? -INFINITY : 0.f;
    int cnt = 0;
    for (int kz = 0; kz < g.kd; kz++)
      for (int ky = 0; ky < g.kh; ky++)
        for (int kx = 0; kx < g.kw; kx++) {
          const int iz = od * g.sd - g.pf + kz * g.dd, iy = oh * g.sh - g.pt + ky * g.dh, ix = ow * g.sw - g.pl + kx * g.dw;
          if (iz < 0 || iz >= g.D || iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) continue;
          const float v = x[(iz * g.H + iy) * g.W + ix];
          acc = is_max ? fmaxf(acc, v) : acc + v;
          cnt++;
        }
    if (!is_max) acc = acc / float(count_pad ? g.kd * g.kh * g.kw : (cnt ? cnt : 1));
    Y[o] = acc;
  }
}

template <int CC>
void launch_mfma(hipStream_t s, dim3 grid, dim3 block, bool staged, const Conv3dSplit &sp, const float *X, const float *Wp, const float *bias, float *Y,
                 int64_t total_pos, int64_t total_rows, const Conv3dGeom &g, ActParam act) {
  if (staged) hipLaunchKernelGGL((conv3d_mfma_kernel<CC, true>), grid, block, size_t(sp.lds_bytes), s, X, Wp, bias, Y, total_pos, total_rows, g, sp, act);
  else hipLaunchKernelGGL((conv3d_mfma_kernel<CC, false>), grid, block, 0, s, X, Wp, bias, Y, total_pos, total_rows, g, sp, act);
}

}  // namespace

size_t conv3d_packed_floats(const Conv3dGeom &g) {
  const Conv3dSplit sp = conv3d_split(g);
  return size_t(sp.Mp) * size_t(sp.Kp);
}
void conv3d_pack(const Conv3dGeom &g, const float *W, float *packed) {
  const Conv3dSplit sp = conv3d_split(g);
  const int64_t pairs = sp.Kp / 2;
  for (int mt = 0; mt < sp.Mp / 32; mt++)
    for (int64_t kp = 0; kp < pairs; kp++)
      for (int lane = 0; lane < 64; lane++) {
        const int m = mt * 32 + (lane & 31);
        const int64_t k = 2 * kp + (lane >> 5), chunk = k / (int64_t(sp.taps) * sp.CC), rem = k - chunk * sp.taps * sp.CC;
        const int64_t tap = rem / sp.CC, c = chunk * sp.CC + rem % sp.CC;
        packed[(mt * pairs + kp) * 64 + lane] = m < g.M && c < g.C ? W[(int64_t(m) * g.C + c) * sp.taps + tap] : 0.f;
      }
}

bool conv3d_mfma(hipStream_t s, const float *X, const float *Wp, const float *bias, float *Y, int64_t rows, const Conv3dGeom &g, bool staged, ActParam act) {
  const Conv3dSplit sp = conv3d_split(g);
  const int64_t total_pos = rows * g.OD * g.OH * g.OW, tiles = (total_pos + kConv3dTilePos - 1) / kConv3dTilePos;
  if (g.groups != 1 || (staged && !sp.fits) || tiles > INT32_MAX || rows < 1) return false;
  const int mtiles = sp.Mp / 32, waves = mtiles < 4 ? mtiles : 4;
  const dim3 grid(unsigned(tiles), unsigned((mtiles + waves - 1) / waves)), block(unsigned(64 * waves));
  const int64_t total_rows = rows * g.OD * g.OH;
  if (sp.CC == 8) launch_mfma<8>(s, grid, block, staged, sp, X, Wp, bias, Y, total_pos, total_rows, g, act);
  else if (sp.CC == 4) launch_mfma<4>(s, grid, block, staged, sp, X, Wp, bias, Y, total_pos, total_rows, g, act);
  else launch_mfma<2>(s, grid, block, staged, sp, X, Wp, bias, Y, total_pos, total_rows, g, act);
  return true;
}

void conv3d_generic(hipStream_t s, const float *X, const float *W, const float *bias, float *Y, int64_t rows, const Conv3dGeom &g, ActParam act) {
  const int64_t total = rows * g.M * g.OD * g.OH * g.OW;
  hipLaunchKernelGGL(conv3d_generic_kernel, dim3(grid_for(total)), dim3(kBlock), 0, s, X, W, bias, Y, total, g, act);
}

void pool3d(hipStream_t s, const float *X, float *Y, int64_t rows, const Conv3dGeom &g, bool is_max, bool count_pad) {
  const int64_t total = rows * g.C * g.OD * g.OH * g.OW;
  hipLaunchKernelGGL(pool3d_kernel, dim3(grid_for(total)), dim3(kBlock), 0, s, X, Y, total, g, is_max, count_pad);
}

}  // namespace infera_hip::kern
