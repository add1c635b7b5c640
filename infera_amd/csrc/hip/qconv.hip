// qconv.hip -- the QConv2d step (host/plan.hpp): a statically quantised convolution (groups == 1) as an implicit GEMM
// on v_mfma_i32_16x16x64_i8.  Per output pixel it is the QDense definition (qdense.hip) with K = C * kh * kw; a tap that falls in the
// padding reads real 0, i.e. the quantised value x_zp, and so contributes (x_zp - x_zp) * (wq - w_zp) = 0.
//
// Rows of the 16 x 16 result tile: 16 consecutive output pixels of the flattened (image, oh, ow) index (a tile may straddle images);
// columns: output channels.  k runs (channel chunk of 16, tap, channel) with the channel fastest: lane l = (c = l & 15, g = l >> 4) of
// k step (cc, tg) holds, in byte j of BOTH fragments, tap 4 tg + g and channel 16 cc + j -- of pixel c on the A side, of output channel
// 16 mt + c on the B side (qconv_pack lays the weights out in exactly the order the lanes load them, 1 KB per fragment).  The integer
// sum is exact and commutative, so this order gives the bits of any other.  Channels beyond C and taps beyond kh * kw are zero bytes on
// both sides.
//
// Signed bytes and zero points, as in qdense.hip: a = xq - shift_x, w = wq - shift_w, xz / wz[m] the zero points shifted alike, and
//   acc = sum a w  -  xz * colsum_w[m]  -  wz[m] * rowsum_a[r]  +  K * xz * wz[m]          (K = C * kh * kw, the real one)
// holds when every one of the K real (tap, channel) pairs of a pixel carries a byte with (a - xz) = its true contribution.  For a tap
// in the padding that byte is xz itself -- NOT zero: with x_zp != 0 a zero byte would stand for the real value -x_zp * x_scale and every
// border pixel would be off by xz * (sum of the weights under the padding).  rowsum_a (only when some wz[m] != 0) comes from one more
// MFMA against a matrix of ones and so counts the padding bytes too, as the formula needs.
//
// Quantising once: a workgroup owns 64 consecutive output pixels (4 waves x 16) and up to 128 output channels.  Per channel chunk it
// quantises the input footprint of its pixels ONCE into LDS -- 16 bytes (the chunk's channels) per position of a [rows][Wp] window of
// the zero-padded input, padding positions filled with xz -- and every tap then is one 16-byte LDS read with no bounds check and no
// division (an element is read by up to kh * kw taps; quantise() is a true f32 division).  Rows are counted in G = image * Hp + padded
// row, so a tile that straddles images just sees a taller window.  A footprint beyond the LDS budget (very wide images) takes the
// direct variant, which quantises per tap from global memory: the same bytes, slower.
// Steps 3..6 of the definition are separately rounded f32 operations, written with operators under contract(off) (see qdense.hip).
#include "device_common.hpp"

#include <algorithm>
#include <cstring>

#pragma clang fp contract(off)

namespace infera_hip::kern {

namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
constexpr int kCBlock = 256, kCWaves = 4, kCPix = kCWaves * 16;
constexpr int kLdsBudget = 48 * 1024;  // bytes of staged input per workgroup (three workgroups per CU keep their windows resident)

// the 16 signed bytes of channels c0 .. c0 + 15 at input position (n, ih, iw): quantised values, xz in the padding, 0 beyond C
__device__ __forceinline__ i32x4 input_bytes(const QConvLaunch &p, int64_t n, int ih, int iw, int c0) {
  i32x4 a = {0, 0, 0, 0};
  if (n >= p.rows) return a;
  const int nc = p.C - c0 < 16 ? p.C - c0 : 16;
  const bool inside = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
  if (!inside) {
    const int b = (p.x_zp - p.x_shift) & 0xFF;
#pragma unroll
    for (int j = 0; j < 16; j++)
      if (j < nc) a[j >> 2] |= b << (8 * (j & 3));
    return a;
  }
  const float xzp = float(p.x_zp), xlo = float(p.x_min), xhi = float(p.x_max);
  const int64_t HW = int64_t(p.H) * p.W, pos = int64_t(ih) * p.W + iw;
  if (p.in_cq) {  // [N][C/4][HW][4]: four channels per 16-byte load (C % 4 == 0)
    const f32x4 *x4 = reinterpret_cast<const f32x4 *>(p.X) + (n * (p.C >> 2) + (c0 >> 2)) * HW + pos;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (4 * q >= nc) break;
      const f32x4 v = x4[q * HW];
      int w = 0;
#pragma unroll
      for (int e = 0; e < 4; e++) w |= ((int(quantise(v[e], p.x_scale, xzp, xlo, xhi)) - p.x_shift) & 0xFF) << (8 * e);
      a[q] = w;
    }
    return a;
  }
  const float *x = p.X + (n * p.C + c0) * HW + pos;
#pragma unroll
  for (int j = 0; j < 16; j++)
    if (j < nc) a[j >> 2] |= ((int(quantise(x[j * HW], p.x_scale, xzp, xlo, xhi)) - p.x_shift) & 0xFF) << (8 * (j & 3));
  return a;
}

template <int NT, bool WZ, bool STAGED>
__global__ __launch_bounds__(kCBlock) void qconv_kernel(QConvLaunch p) {
  extern __shared__ i32x4 tile[];  // STAGED: [window rows][Wp] positions x 16 channel bytes
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int64_t S = int64_t(p.OH) * p.OW, npix = p.rows * S;
  const int64_t pix_first = int64_t(blockIdx.x) * kCPix, pix_last = (pix_first + kCPix < npix ? pix_first + kCPix : npix) - 1;
  const int64_t row0 = pix_first + wave * 16;  // this wave's 16 pixels
  // the pixel whose A rows this lane loads
  const int64_t pix = row0 + c;
  const bool pix_ok = pix < npix;
  const int64_t pn = pix_ok ? pix / S : 0;
  const int prem = pix_ok ? int(pix - pn * S) : 0;
  const int poh = prem / p.OW, pow_ = prem - poh * p.OW;
  // window rows G = image * Hp + padded row, from the first pixel's first tap to the last pixel's last one
  const int64_t n_first = pix_first / S, n_last = pix_last / S;
  const int64_t G0 = n_first * p.Hpad + int((pix_first - n_first * S) / p.OW) * p.sh;
  const int64_t G1 = n_last * p.Hpad + int((pix_last - n_last * S) / p.OW) * p.sh + (p.kh - 1) * p.dh;
  const int64_t window = (G1 - G0 + 1) * p.Wpad;
  const int entries = window < p.lds_entries ? int(window) : p.lds_entries;
  const int lbase = int(pn * p.Hpad + poh * p.sh - G0) * p.Wpad + pow_ * p.sw;  // this lane's pixel, tap (0, 0), in the window
  const int mt0 = int(blockIdx.y) * NT;
  const int taps = p.kh * p.kw;
  const i32x4 *wp = reinterpret_cast<const i32x4 *>(p.Wfrag);
  i32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = i32x4{0, 0, 0, 0};
  i32x4 rs = {0, 0, 0, 0};
  const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
  for (int cc = 0; cc < p.CT; cc++) {
    if (STAGED) {
      if (cc) __syncthreads();  // (every wave is done with the previous chunk's window)
      for (int e = threadIdx.x; e < entries; e += kCBlock) {
        const int wr = e / p.Wpad, wc = e - wr * p.Wpad;
        const int64_t G = G0 + wr, n = G / p.Hpad;
        tile[e] = input_bytes(p, n, int(G - n * p.Hpad) - p.pt, wc - p.pl, cc * 16);
      }
      __syncthreads();
    }
    for (int tg = 0; tg < p.TG; tg++) {
      const int tap = tg * 4 + g;
      i32x4 a = {0, 0, 0, 0};
      if (pix_ok && tap < taps) {
        const int ky = tap / p.kw, kx = tap - ky * p.kw;
        if (STAGED) a = tile[lbase + ky * p.dh * p.Wpad + kx * p.dw];
        else a = input_bytes(p, pn, poh * p.sh + ky * p.dh - p.pt, pow_ * p.sw + kx * p.dw - p.pl, cc * 16);
      }
      const i32x4 *w = wp + ((int64_t(cc) * p.TG + tg) * p.MTp + mt0) * 64 + lane;
#pragma unroll
      for (int t = 0; t < NT; t++) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, w[t * 64], acc[t], 0, 0, 0);
      if (WZ) rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, ones, rs, 0, 0, 0);
    }
  }
  // C/D: column l & 15 (output channel), row 4 (l >> 4) + register (pixel)
  const float yzp = float(p.y_zp), ylo = float(p.y_min), yhi = float(p.y_max);
  int64_t on[4];
  int opos[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int64_t r = row0 + g * 4 + i;
    on[i] = r < npix ? r / S : -1;
    opos[i] = r < npix ? int(r - on[i] * S) : 0;
  }
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int col = (mt0 + t) * 16 + c;
    if (col >= p.M) continue;
    const float mult = p.mult[col];
    const unsigned c0 = unsigned(p.c0[col]);
    const unsigned wz = WZ ? unsigned(p.wz[col]) : 0u;
    const float bias = p.bias ? p.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (on[i] < 0) continue;
      const int sum = int(unsigned(acc[t][i]) + c0 - wz * unsigned(rs[i]));
      float real = float(sum) * mult;
      if (p.bias) real = real + bias;
      if (p.act == 1) real = fmaxf(real, 0.f);
      else if (p.act == 5) real = fminf(fmaxf(real, p.act_a), p.act_b);
      float out = real;
      if (p.y_on) {
        const float q = quantise(real, p.y_scale, yzp, ylo, yhi);
        out = (q - yzp) * p.y_scale;
      }
      if (p.out_cq) p.Y[((on[i] * (p.M >> 2) + (col >> 2)) * S + opos[i]) * 4 + (col & 3)] = out;
      else p.Y[(on[i] * p.M + col) * S + opos[i]] = out;
    }
  }
}

int conv_tiles_per_wave(int M) {
  const int mt = (M + 15) / 16;
  int nt = 1;
  while (nt < mt && nt < 8) nt *= 2;
  return nt;
}

// window positions the most demanding workgroup stages: the largest (G1 - G0 + 1) * Wp over the distinct tile offsets inside an image
int64_t window_entries(const QConvLaunch &p) {
  const int64_t S = int64_t(p.OH) * p.OW;
  int64_t g = S, b = kCPix;
  while (b) std::swap(g %= b, b);  // gcd(S, 64): tile starts repeat with period S / gcd
  const int64_t distinct = S / g;
  const int64_t span_cap = (int64_t(kCPix - 1) / p.OW + 2) * p.sh + int64_t(kCPix - 1) / S * p.Hpad + p.Hpad + int64_t(p.kh - 1) * p.dh + 1;
  if (distinct > (int64_t(1) << 20)) return span_cap * p.Wpad;
  int64_t most = 0;
  for (int64_t t = 0; t < distinct; t++) {
    const int64_t first = (t * kCPix) % S, last = first + kCPix - 1;
    const int64_t n1 = last / S;
    const int64_t G0 = (first / p.OW) * p.sh, G1 = n1 * p.Hpad + ((last - n1 * S) / p.OW) * p.sh + int64_t(p.kh - 1) * p.dh;
    most = std::max(most, G1 - G0 + 1);
  }
  return most * p.Wpad;
}

template <int NT>
void launch(hipStream_t s, const QConvLaunch &p, dim3 grid, bool staged) {
  const size_t lds = staged ? size_t(p.lds_entries) * 16 : 0;
  if (staged) {
    if (p.wz) hipLaunchKernelGGL((qconv_kernel<NT, true, true>), grid, dim3(kCBlock), lds, s, p);
    else hipLaunchKernelGGL((qconv_kernel<NT, false, true>), grid, dim3(kCBlock), lds, s, p);
  } else {
    if (p.wz) hipLaunchKernelGGL((qconv_kernel<NT, true, false>), grid, dim3(kCBlock), 0, s, p);
    else hipLaunchKernelGGL((qconv_kernel<NT, false, false>), grid, dim3(kCBlock), 0, s, p);
  }
}

}  // namespace

int qconv_padded_m(int M) {
  const int nt = conv_tiles_per_wave(M), mt = (M + 15) / 16;
  return (mt + nt - 1) / nt * nt * 16;
}

size_t qconv_packed_floats(int C, int taps, int M) { return size_t((C + 15) / 16) * size_t((taps + 3) / 4) * size_t(qconv_padded_m(M) / 16) * 64 * 4; }

void qconv_pack(int C, int taps, int M, const int8_t *W, float *packed) {
  const int CT = (C + 15) / 16, TG = (taps + 3) / 4, MTp = qconv_padded_m(M) / 16;
  std::vector<int8_t> out(size_t(CT) * TG * MTp * 64 * 16, 0);
  for (int cc = 0; cc < CT; cc++)
    for (int tg = 0; tg < TG; tg++)
      for (int mt = 0; mt < MTp; mt++)
        for (int lane = 0; lane < 64; lane++)
          for (int j = 0; j < 16; j++) {
            const int ch = cc * 16 + j, tap = tg * 4 + (lane >> 4), col = mt * 16 + (lane & 15);
            if (ch < C && tap < taps && col < M)
              out[(((size_t(cc) * TG + tg) * MTp + mt) * 64 + lane) * 16 + j] = W[(size_t(ch) * taps + tap) * M + col];
          }
  std::memcpy(packed, out.data(), out.size());
}

bool qconv_stages_in_lds(QConvLaunch p) {
  p.Hpad = (p.OH - 1) * p.sh + (p.kh - 1) * p.dh + 1;
  p.Wpad = (p.OW - 1) * p.sw + (p.kw - 1) * p.dw + 1;
  return window_entries(p) * 16 <= kLdsBudget;
}

void qconv(hipStream_t s, QConvLaunch p) {
  if (p.rows <= 0) return;
  const int nt = conv_tiles_per_wave(p.M);
  p.CT = (p.C + 15) / 16;
  p.TG = (p.kh * p.kw + 3) / 4;
  p.MTp = qconv_padded_m(p.M) / 16;
  // the extent of the zero-padded image that the taps reach (<= H + pt + pb, W + pl + pr)
  p.Hpad = (p.OH - 1) * p.sh + (p.kh - 1) * p.dh + 1;
  p.Wpad = (p.OW - 1) * p.sw + (p.kw - 1) * p.dw + 1;
  const int64_t entries = window_entries(p);
  const bool staged = !p.force_direct && entries * 16 <= kLdsBudget;
  p.lds_entries = staged ? int(entries) : 0;
  const int64_t npix = p.rows * p.OH * p.OW;
  const dim3 grid(unsigned((npix + kCPix - 1) / kCPix), unsigned(p.MTp / nt));
  switch (nt) {
    case 1: launch<1>(s, p, grid, staged); break;
    case 2: launch<2>(s, p, grid, staged); break;
    case 4: launch<4>(s, p, grid, staged); break;
    default: launch<8>(s, p, grid, staged); break;
  }
}

}  // namespace infera_hip::kern
