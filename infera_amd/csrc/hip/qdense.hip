// qdense.hip -- the QDense step (host/plan.hpp): a statically quantised MatMul / Gemm on the int8 matrix cores.
//
//   xq = sat(rne(x / x_scale) + x_zp);  acc = sum_k (xq - x_zp)(wq - w_zp[m]) [+ int32 bias];  real = float(acc) * mult[m] [+ f32 bias];
//   act;  q = sat(rne(real / y_scale) + y_zp);  out = (q - y_zp) * y_scale
//
// v_mfma_i32_16x16x64_i8 reads SIGNED bytes, so uint8 data is shifted by 128 (a = xq - shift_x, w = wq - shift_w, zero points shifted
// alike: xz, wz[m]) and the zero-point terms are put back exactly:
//   acc = sum a w  -  xz * colsum_w[m]  -  wz[m] * rowsum_a[r]  +  K * xz * wz[m]
// colsum_w is computed at load (c0[m] below holds every term that does not depend on the row, the int32 bias included); rowsum_a only
// when some wz[m] != 0, by one more MFMA per K step against a matrix of ones -- it lands in the accumulator's own row map.  All of it
// is unsigned 32-bit arithmetic: the true result fits int32 (the load-time cap on K), so wrapped partial terms cancel.
//
// One wavefront owns 16 table rows and up to NT * 16 output columns.  Per K step of 64 it quantises 16 consecutive floats per lane (the
// lanes of one row cover 256 contiguous bytes) into the A fragment and multiplies it with NT weight fragments that lie in the order the
// lanes load them (qdense_pack: 1 KB per fragment, L2-resident).  Lane l = (c = l & 15, g = l >> 4) holds k = 64 kt + 16 g + j in byte j
// of BOTH fragments: the instruction's own k order inside a fragment does not matter, the integer sum is exact and commutative.
// C/D: column l & 15, row 4 (l >> 4) + register.  Padded k are zero bytes on both sides.
// With f32 input and output the step streams 4 (K + M) bytes per row against 2 K M int8 operations: HBM-bound for every tabular shape.
#include "device_common.hpp"

#include <cstring>

// Every product and sum below is rounded on its own (the step's definition).  The compiler contracts a * b + c by default, and the
// headers' __fmul_rn / __fadd_rn are plain operators compiled under that default (a product and a sum spelled with them came back as one
// v_fma_f32), so the arithmetic is written with operators HERE, under this pragma.
#pragma clang fp contract(off)

namespace infera_hip::kern {

namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
constexpr int kQBlock = 256, kQWaves = 4;

template <int NT, bool WZ>
__global__ __launch_bounds__(kQBlock) void qdense_kernel(QDenseLaunch p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t(blockIdx.x) * kQWaves + wave) * 16;
  if (row0 >= p.rows) return;
  const int c = lane & 15, g = lane >> 4;
  const int64_t row = row0 + c;  // the row this lane quantises
  const bool row_ok = row < p.rows;
  const int mt0 = int(blockIdx.y) * NT;
  const i32x4 *wp = reinterpret_cast<const i32x4 *>(p.Wp);
  const float xzp = float(p.x_zp), xlo = float(p.x_min), xhi = float(p.x_max);
  i32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = i32x4{0, 0, 0, 0};
  i32x4 rs = {0, 0, 0, 0};
  const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
  for (int kt = 0; kt < p.KT; kt++) {
    const int k0 = kt * 64 + g * 16;
    i32x4 a = {0, 0, 0, 0};
    if (row_ok && k0 < p.K) {
      if (p.in_bytes) {
        const signed char *xr = reinterpret_cast<const signed char *>(p.X) + row * p.K;
        if (p.x_vec && k0 + 16 <= p.K) {
          a = *reinterpret_cast<const i32x4 *>(xr + k0);
        } else {
#pragma unroll
          for (int j = 0; j < 16; j++) {
            const int b = k0 + j < p.K ? int(xr[k0 + j]) : 0;
            a[j >> 2] |= (b & 0xFF) << (8 * (j & 3));
          }
        }
      } else {
        const float *xr = reinterpret_cast<const float *>(p.X) + row * p.K;
        float v[16];
        if (p.x_vec && k0 + 16 <= p.K) {
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const f32x4 q = *reinterpret_cast<const f32x4 *>(xr + k0 + 4 * j);
            v[4 * j] = q[0], v[4 * j + 1] = q[1], v[4 * j + 2] = q[2], v[4 * j + 3] = q[3];
          }
        } else {
#pragma unroll
          for (int j = 0; j < 16; j++) v[j] = k0 + j < p.K ? xr[k0 + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 16; j++) {
          const int b = k0 + j < p.K ? int(quantise(v[j], p.x_scale, xzp, xlo, xhi)) - p.x_shift : 0;
          a[j >> 2] |= (b & 0xFF) << (8 * (j & 3));
        }
      }
    }
    const i32x4 *w = wp + (int64_t(kt) * p.MTp + mt0) * 64 + lane;
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, w[t * 64], acc[t], 0, 0, 0);
    if (WZ) rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, ones, rs, 0, 0, 0);
  }
  const float yzp = float(p.y_zp), ylo = float(p.y_min), yhi = float(p.y_max);
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
      const int64_t r = row0 + g * 4 + i;
      if (r >= p.rows) continue;
      const int sum = int(unsigned(acc[t][i]) + c0 - wz * unsigned(rs[i]));
      float real = float(sum) * mult;
      if (p.bias) real = real + bias;
      if (p.act == 1) real = fmaxf(real, 0.f);
      else if (p.act == 5) real = fminf(fmaxf(real, p.act_a), p.act_b);
      if (!p.y_on) {
        reinterpret_cast<float *>(p.Y)[r * p.M + col] = real;
        continue;
      }
      const float q = quantise(real, p.y_scale, yzp, ylo, yhi);
      if (p.out_bytes) reinterpret_cast<signed char *>(p.Y)[r * p.M + col] = (signed char)(int(q) - p.y_shift);
      else reinterpret_cast<float *>(p.Y)[r * p.M + col] = (q - yzp) * p.y_scale;
    }
  }
}

int tiles_per_wave(int M) {
  const int mt = (M + 15) / 16;
  int nt = 1;
  while (nt < mt && nt < 16) nt *= 2;
  return nt;
}

template <int NT>
void launch(hipStream_t s, const QDenseLaunch &p, dim3 grid) {
  if (p.wz) hipLaunchKernelGGL((qdense_kernel<NT, true>), grid, dim3(kQBlock), 0, s, p);
  else hipLaunchKernelGGL((qdense_kernel<NT, false>), grid, dim3(kQBlock), 0, s, p);
}

}  // namespace

int qdense_padded_m(int M) {
  const int nt = tiles_per_wave(M), mt = (M + 15) / 16;
  return (mt + nt - 1) / nt * nt * 16;
}

size_t qdense_packed_floats(int K, int M) { return size_t((K + 63) / 64) * size_t(qdense_padded_m(M) / 16) * 64 * 4; }

void qdense_pack(int K, int M, const int8_t *W, float *packed) {
  const int KT = (K + 63) / 64, MTp = qdense_padded_m(M) / 16;
  std::vector<int8_t> out(size_t(KT) * MTp * 64 * 16, 0);
  for (int kt = 0; kt < KT; kt++)
    for (int mt = 0; mt < MTp; mt++)
      for (int lane = 0; lane < 64; lane++)
        for (int j = 0; j < 16; j++) {
          const int k = kt * 64 + (lane >> 4) * 16 + j, col = mt * 16 + (lane & 15);
          if (k < K && col < M) out[((size_t(kt) * MTp + mt) * 64 + lane) * 16 + j] = W[size_t(k) * M + col];
        }
  std::memcpy(packed, out.data(), out.size());
}

void qdense(hipStream_t s, QDenseLaunch p) {
  if (p.rows <= 0) return;
  const int nt = tiles_per_wave(p.M);
  p.KT = (p.K + 63) / 64;
  p.MTp = qdense_padded_m(p.M) / 16;
  // 16-byte loads of a row's fragment: every row starts on a 16-byte boundary
  p.x_vec = reinterpret_cast<uintptr_t>(p.X) % 16 == 0 && (p.in_bytes ? p.K % 16 == 0 : p.K % 4 == 0);
  const int64_t tiles = (p.rows + 15) / 16;
  const dim3 grid(unsigned((tiles + kQWaves - 1) / kQWaves), unsigned(p.MTp / nt));
  switch (nt) {
    case 1: launch<1>(s, p, grid); break;
    case 2: launch<2>(s, p, grid); break;
    case 4: launch<4>(s, p, grid); break;
    case 8: launch<8>(s, p, grid); break;
    default: launch<16>(s, p, grid); break;
  }
}

}  // namespace infera_hip::kern
