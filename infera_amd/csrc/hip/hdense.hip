// hdense.hip -- the HDense step (host/plan.hpp): a float16 MatMul / Gemm on the f16 matrix cores.
//
//   xh = half_rne(x) (an f32 input buffer; a half buffer holds xh itself);  acc = sum_k xh * wh in f32 (products of two halves are exact
//   in f32; the order of the sum is the instruction's and the loop's);
//   r = half(acc + b) (Gemm) | half(float(half(acc)) + b) (MatMul -> Add) | half(acc);  act: r = half(act(float(r)))
//
// v_mfma_f32_16x16x32_f16 computes D = A . B + C with A [16 rows, 32 k], B [32 k, 16 cols]: lane l holds A[l & 15][8 (l >> 4) + j] and
// B[8 (l >> 4) + j][l & 15], j = 0..7, and D[4 (l >> 4) + i][l & 15] in register i (the lane maps of the bf16 twin).  The kernel
// computes the TRANSPOSED tile: A = W^T (row = output column), B = X^T (column = table row).  A lane then loads 8 consecutive k of ITS
// table row (l & 15) -- 32 contiguous bytes of f32, 16 of halves -- and ends with 4 CONSECUTIVE output columns 4 (l >> 4) + i of that
// row in its accumulator: one 16-byte store of f32 results (8 bytes of halves).
//
// One wavefront owns 16 table rows and up to NT * 16 output columns; per K step of 32 it rounds / loads one X fragment and multiplies it
// with NT weight fragments that lie in the order the lanes load them (hdense_pack: 1 KB per fragment, L2-resident).  K is padded with
// zero halves on both sides, rows and columns beyond the table are masked at the loads and at the stores.
// A step streams 4 (or 2) bytes per input and per output element against 2 K M half operations: HBM-bound for every tabular shape.
#include "device_common.hpp"

#include <cstring>

// The roundings of the definition are separate operations: acc + b must not be contracted with anything around it (qdense.hip explains
// what the default contraction did to two separately rounded operations).
#pragma clang fp contract(off)

namespace infera_hip::kern {

namespace {

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;
constexpr int kHBlock = 256, kHWaves = 4;

// float(half_rne(v)): v_cvt_f16_f32 under the default rounding mode (nearest even) with f16 subnormals kept
__device__ __forceinline__ float to_half_value(float v) { return float(_Float16(v)); }

// the X fragment of K step kt for this lane's row: 8 halves, zeros beyond K and beyond the last row
__device__ __forceinline__ f16x8 load_x(const HDenseLaunch &p, int64_t row, bool row_ok, int k0) {
  f16x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!row_ok || k0 >= p.K) return a;
  if (p.in_half) {
    const _Float16 *xr = reinterpret_cast<const _Float16 *>(p.X) + row * p.K;
    if (p.x_vec && k0 + 8 <= p.K) return *reinterpret_cast<const f16x8 *>(xr + k0);
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (k0 + j < p.K) a[j] = xr[k0 + j];
    return a;
  }
  const float *xr = reinterpret_cast<const float *>(p.X) + row * p.K;
  if (p.x_vec && k0 + 8 <= p.K) {
    const f32x4 lo = *reinterpret_cast<const f32x4 *>(xr + k0), hi = *reinterpret_cast<const f32x4 *>(xr + k0 + 4);
#pragma unroll
    for (int j = 0; j < 4; j++) a[j] = _Float16(lo[j]), a[4 + j] = _Float16(hi[j]);
    return a;
  }
#pragma unroll
  for (int j = 0; j < 8; j++)
    if (k0 + j < p.K) a[j] = _Float16(xr[k0 + j]);
  return a;
}

template <int NT>
__global__ __launch_bounds__(kHBlock) void hdense_kernel(HDenseLaunch p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t(blockIdx.x) * kHWaves + wave) * 16;
  if (row0 >= p.rows) return;
  const int c = lane & 15, g = lane >> 4;
  const int64_t row = row0 + c;  // the table row this lane loads and stores
  const bool row_ok = row < p.rows;
  const int mt0 = int(blockIdx.y) * NT;
  const f16x8 *wp = reinterpret_cast<const f16x8 *>(p.Wp);
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  f16x8 next = load_x(p, row, row_ok, g * 8);
  for (int kt = 0; kt < p.KT; kt++) {
    const f16x8 x = next;
    if (kt + 1 < p.KT) next = load_x(p, row, row_ok, (kt + 1) * 32 + g * 8);
    const f16x8 *w = wp + (int64_t(kt) * p.MTp + mt0) * 64 + lane;
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[t * 64], x, acc[t], 0, 0, 0);
  }
  if (!row_ok) return;
  dispatch_act(p.act, [&](auto kind) {
    constexpr int ACT = decltype(kind)::value;
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const int col = (mt0 + t) * 16 + g * 4;  // this lane's four columns: col .. col + 3
      if (col >= p.M) continue;
      f32x4 b = {0.f, 0.f, 0.f, 0.f};
      if (p.bias_mode) b = *reinterpret_cast<const f32x4 *>(p.bias + col);  // (padded to MTp * 16 entries)
      f32x4 r;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        float v = acc[t][i];
        if (p.bias_mode == 2) v = to_half_value(v);
        if (p.bias_mode) v = v + b[i];
        v = to_half_value(v);
        if (ACT != 0) v = to_half_value(apply_act_c<ACT>(v, p.act_a, p.act_b));
        r[i] = v;
      }
      if (p.out_half) {
        _Float16 *y = reinterpret_cast<_Float16 *>(p.Y) + row * p.M + col;
        if (p.y_vec) {
          *reinterpret_cast<f16x4 *>(y) = f16x4{_Float16(r[0]), _Float16(r[1]), _Float16(r[2]), _Float16(r[3])};
        } else {
#pragma unroll
          for (int i = 0; i < 4; i++)
            if (col + i < p.M) y[i] = _Float16(r[i]);
        }
      } else {
        float *y = reinterpret_cast<float *>(p.Y) + row * p.M + col;
        if (p.y_vec) {
          *reinterpret_cast<f32x4 *>(y) = r;
        } else {
#pragma unroll
          for (int i = 0; i < 4; i++)
            if (col + i < p.M) y[i] = r[i];
        }
      }
    }
  });
}

int tiles_per_wave(int M) {
  const int mt = (M + 15) / 16;
  int nt = 1;
  while (nt < mt && nt < 16) nt *= 2;
  return nt;
}

}  // namespace

int hdense_padded_m(int M) {
  const int nt = tiles_per_wave(M), mt = (M + 15) / 16;
  return (mt + nt - 1) / nt * nt * 16;
}

size_t hdense_packed_floats(int K, int M) { return size_t((K + 31) / 32) * size_t(hdense_padded_m(M) / 16) * 64 * 4; }

void hdense_pack(int K, int M, const uint16_t *W, float *packed) {
  const int KT = (K + 31) / 32, MTp = hdense_padded_m(M) / 16;
  std::vector<uint16_t> out(size_t(KT) * MTp * 64 * 8, 0);
  for (int kt = 0; kt < KT; kt++)
    for (int mt = 0; mt < MTp; mt++)
      for (int lane = 0; lane < 64; lane++)
        for (int j = 0; j < 8; j++) {
          const int k = kt * 32 + (lane >> 4) * 8 + j, col = mt * 16 + (lane & 15);
          if (k < K && col < M) out[((size_t(kt) * MTp + mt) * 64 + lane) * 8 + j] = W[size_t(k) * M + col];
        }
  std::memcpy(packed, out.data(), out.size() * 2);
}

void hdense(hipStream_t s, HDenseLaunch p) {
  if (p.rows <= 0) return;
  const int nt = tiles_per_wave(p.M);
  p.KT = (p.K + 31) / 32;
  p.MTp = hdense_padded_m(p.M) / 16;
  // 16-byte loads of a row's fragment and wide stores of a lane's four results: every row starts on such a boundary
  p.x_vec = reinterpret_cast<uintptr_t>(p.X) % 16 == 0 && (p.in_half ? p.K % 8 == 0 : p.K % 4 == 0);
  p.y_vec = reinterpret_cast<uintptr_t>(p.Y) % 16 == 0 && p.M % 4 == 0;
  const int64_t tiles = (p.rows + 15) / 16;
  const dim3 grid(unsigned((tiles + kHWaves - 1) / kHWaves), unsigned(p.MTp / nt));
  switch (nt) {
    case 1: hipLaunchKernelGGL(hdense_kernel<1>, grid, dim3(kHBlock), 0, s, p); break;
    case 2: hipLaunchKernelGGL(hdense_kernel<2>, grid, dim3(kHBlock), 0, s, p); break;
    case 4: hipLaunchKernelGGL(hdense_kernel<4>, grid, dim3(kHBlock), 0, s, p); break;
    case 8: hipLaunchKernelGGL(hdense_kernel<8>, grid, dim3(kHBlock), 0, s, p); break;
    default: hipLaunchKernelGGL(hdense_kernel<16>, grid, dim3(kHBlock), 0, s, p); break;
  }
}

}  // namespace infera_hip::kern
