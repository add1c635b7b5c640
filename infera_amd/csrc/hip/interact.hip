// interact.hip -- feature interactions of recommender models on gfx950 (semantics: INTEGRATION.md section 2.6 "Feature interactions";
// tables: host/interact.hpp).  Both kernels read T [rows, k, d] once and give one wave (fm: one lane group) a whole row, so a row's bits
// depend on the model and the row alone: no atomics, nothing that depends on the grid, and a NaN or Inf never leaves its row.
//
// interact_dot_kernel<KT>: Z = T . T^T on the exact-f32 matrix instructions (every entry an fmaf chain over the columns in one fixed order).
//   A Gram matrix has ONE operand: for v_mfma_f32_32x32x2_f32 the A fragment is lane (m, h) -> T[m][2 s + h] and the B fragment is lane
//   (n, h) -> T^T[2 s + h][n] = T[n][2 s + h], the same register, so one load feeds both sides.
//     KT = 16 (k <= 16): v_mfma_f32_16x16x4_f32, lane (m = l & 15, q = l >> 4) loads T[m][16 g + 4 q .. + 3]; k-step j of group g multiplies
//                        columns 16 g + 4 q + j.
//     KT = 32 (k <= 32): v_mfma_f32_32x32x2_f32, lane (m = l & 31, h = l >> 5) loads T[m][8 g + 4 h .. + 3]; k-step j multiplies columns
//                        8 g + j and 8 g + 4 + j (the dense.hip / nearest.hip permutation).
//     KT = 64 (k <= 64): two such fragments (fields m and 32 + m) and the four 32 x 32 tiles of Z.
//   One 16-byte load per lane and group where d is a multiple of 4 (every field then starts on 16 bytes), else four guarded scalar loads;
//   fields >= k and columns >= d are zeros in registers and nothing past a row's k * d floats is read.
//   Epilogue: the wave stages Z in LDS (KT * KT floats, its own region) and lane l writes out[r, c] for c = l, l + 64, ...: map[c] >= 0 is
//   the staged address of a selected entry, map[c] < 0 a column of T's own row (a pass-through bit copy).  The stores of a wave are
//   consecutive floats.  The [k, k] matrix itself reaches memory only where the model reads all of it (map = every entry in order).
//   The other epilogue the design named -- no LDS, every accumulator entry stored straight to the output columns that want it through a
//   Z entry -> columns list (a selection may name an entry several times), the pass-through columns copied by a short list of their own
//   -- was built as a template flag of this kernel, gave the same bits, was measured and was taken out again.  2026-10-19, one MI355X,
//   131,072 rows, strict triangle of k = 27 (profiles/r21_interact.txt; step = a model's time minus the same model without the step):
//   d = 16 staged 0.123 ms, scattered 0.186 ms; d = 128 staged 0.525 ms, scattered 0.618 ms; with pass-through 0.116 / 0.195 ms and
//   0.601 / 0.672 ms.  Staged wins all four: its stores are consecutive floats, the scattered ones 4-byte stores a lane apart in no order,
//   issued from a divergent loop.  Against torch-ROCm float32 bmm + index (+ cat) on the same tensors the staged step takes 0.10 (d = 16)
//   and 0.22 (d = 128) of the time.
//
// interact_fm_kernel: the bi-interaction term h * ((sum_f v)^2 - sum_f v^2) on the VALU, as written: one pass over the fields in order
//   with the running pair (sum, sum of squares) of each column in registers, products and sums rounded separately (no contraction), then
//   the optional sum over the columns (a lane's columns ascending, then a fixed butterfly over the group's lanes).  A group of L lanes
//   (L = the power of two >= d, at most 64) owns a row, so a wave holds 64 / L rows.
#include "device_common.hpp"
#include "kernels.hpp"

#include "../host/interact.hpp"

namespace infera_hip::kern {

namespace {

// the four columns c0 .. c0 + 3 of field m of the row at `t` (zeros beyond k and d)
__device__ __forceinline__ f32x4 load_quad(const float *__restrict__ t, int m, int c0, int k, int d, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (m >= k || c0 >= d) return v;
  const float *p = t + int64_t(m) * d + c0;
  if (vec) return *reinterpret_cast<const f32x4 *>(p);  // (d % 4 == 0: c0 + 3 < d, 16-byte aligned)
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (c0 + j < d) v[j] = p[j];
  return v;
}

template <int KT>
struct DotShape {
  static constexpr int kWaves = KT == 64 ? 2 : 4;
};

template <int KT>
__global__ __launch_bounds__(DotShape<KT>::kWaves * 64) void interact_dot_kernel(const float *__restrict__ T, int k, int d, const int32_t *__restrict__ map,
                                                                                 int F, float *__restrict__ out, int64_t nr, bool vec) {
  constexpr int kWaves = DotShape<KT>::kWaves;
  __shared__ __attribute__((aligned(16))) float lds[kWaves * KT * KT];
  const int wave = int(threadIdx.x >> 6), lane = int(threadIdx.x & 63);
  const int64_t row = int64_t(blockIdx.x) * kWaves + wave;
  const bool live = row < nr;
  const float *t = T + (live ? row : 0) * int64_t(k) * d;
  float *z = lds + wave * KT * KT;
  if (live) {
    if constexpr (KT == 16) {
      const int m = lane & 15, q = lane >> 4;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int g = 0; 16 * g < d; g++) {  // (the trip count is the wave's: a lane past d loads zeros)
        const f32x4 a = load_quad(t, m, 16 * g + 4 * q, k, d, vec);
#pragma unroll
        for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], a[j], acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; i++) z[(4 * q + i) * KT + m] = acc[i];
    } else {
      const int m = lane & 31, h = lane >> 5;
      if constexpr (KT == 32) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] = 0.f;
        for (int g = 0; 8 * g < d; g++) {
          const f32x4 a = load_quad(t, m, 8 * g + 4 * h, k, d, vec);
#pragma unroll
          for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], a[j], acc, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; i++) z[(8 * (i >> 2) + 4 * h + (i & 3)) * KT + m] = acc[i];
      } else {
        f32x16 z00, z01, z10, z11;
#pragma unroll
        for (int i = 0; i < 16; i++) z00[i] = z01[i] = z10[i] = z11[i] = 0.f;
        for (int g = 0; 8 * g < d; g++) {
          const f32x4 a = load_quad(t, m, 8 * g + 4 * h, k, d, vec);
          const f32x4 b = load_quad(t, 32 + m, 8 * g + 4 * h, k, d, vec);
#pragma unroll
          for (int j = 0; j < 4; j++) {
            z00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], a[j], z00, 0, 0, 0);
            z01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], z01, 0, 0, 0);
            z10 = __builtin_amdgcn_mfma_f32_32x32x2f32(b[j], a[j], z10, 0, 0, 0);
            z11 = __builtin_amdgcn_mfma_f32_32x32x2f32(b[j], b[j], z11, 0, 0, 0);
          }
        }
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const int zr = 8 * (i >> 2) + 4 * h + (i & 3);
          z[zr * KT + m] = z00[i];
          z[zr * KT + 32 + m] = z01[i];
          z[(32 + zr) * KT + m] = z10[i];
          z[(32 + zr) * KT + 32 + m] = z11[i];
        }
      }
    }
  }
  __syncthreads();
  if (!live) return;
  float *o = out + row * int64_t(F);
  for (int c = lane; c < F; c += 64) {
    const int32_t a = map[c];
    o[c] = a >= 0 ? z[a] : t[-(a + 1)];
  }
}

// L lanes per row (a power of two, <= 64); a lane holds the running pairs of columns lane, lane + L, ... (at most kFmPairs of them)
constexpr int kFmPairs = int(kInteractMaxD / 64);

__global__ __launch_bounds__(256) void interact_fm_kernel(const float *__restrict__ T, int k, int d, float h, bool has_h, bool h_after, bool sum_last, int L,
                                                          float *__restrict__ out, int64_t nr) {
  const int per_block = 256 / L;
  const int sub = int(threadIdx.x) / L, c0 = int(threadIdx.x) % L;
  const int64_t row = int64_t(blockIdx.x) * per_block + sub;
  const bool live = row < nr;
  const float *t = T + (live ? row : 0) * int64_t(k) * d;
  float s[kFmPairs], q[kFmPairs];
#pragma unroll
  for (int i = 0; i < kFmPairs; i++) s[i] = q[i] = 0.f;
  if (live)
    for (int f = 0; f < k; f++) {
#pragma unroll
      for (int i = 0; i < kFmPairs; i++) {
        const int c = c0 + i * L;
        if (c < d) {
          const float v = t[int64_t(f) * d + c];
          s[i] = __fadd_rn(s[i], v);
          q[i] = __fadd_rn(q[i], __fmul_rn(v, v));
        }
      }
    }
  float part = 0.f;
#pragma unroll
  for (int i = 0; i < kFmPairs; i++) {
    const int c = c0 + i * L;
    if (c < d) {
      float v = __fsub_rn(__fmul_rn(s[i], s[i]), q[i]);
      if (has_h && !h_after) v = __fmul_rn(v, h);
      if (sum_last) part = __fadd_rn(part, v);
      else if (live) out[row * int64_t(d) + c] = v;
    }
  }
  if (!sum_last) return;
  for (int w = 1; w < L; w <<= 1) part = __fadd_rn(part, __shfl_xor(part, w));  // (every lane of the wave takes part: a group is a run of L lanes)
  if (has_h && h_after) part = __fmul_rn(part, h);
  if (live && c0 == 0) out[row] = part;
}

}  // namespace

bool interact_dot(hipStream_t s, const float *T, int k, int d, int tile, const int32_t *map, int64_t F, float *out, int64_t rows) {
  if (rows <= 0 || F <= 0) return true;
  if (k < 1 || k > kInteractMaxK || d < 1 || d > kInteractMaxD || F >= (int64_t(1) << 31) - 4096 || k > tile) return false;
  const bool vec = d % 4 == 0 && reinterpret_cast<uintptr_t>(T) % 16 == 0;
  auto blocks = [&](int waves) { return (rows + waves - 1) / waves; };
  if (blocks(2) > 0x7fffffff) return false;
  if (tile == 16)
    hipLaunchKernelGGL((interact_dot_kernel<16>), dim3(unsigned(blocks(4))), dim3(256), 0, s, T, k, d, map, int(F), out, rows, vec);
  else if (tile == 32)
    hipLaunchKernelGGL((interact_dot_kernel<32>), dim3(unsigned(blocks(4))), dim3(256), 0, s, T, k, d, map, int(F), out, rows, vec);
  else if (tile == 64)
    hipLaunchKernelGGL((interact_dot_kernel<64>), dim3(unsigned(blocks(2))), dim3(128), 0, s, T, k, d, map, int(F), out, rows, vec);
  else
    return false;
  return true;
}

bool interact_fm(hipStream_t s, const float *T, int k, int d, float h, bool has_h, bool h_after, bool sum_last, float *out, int64_t rows) {
  if (rows <= 0) return true;
  if (k < 1 || k > kInteractMaxK || d < 1 || d > kInteractMaxD) return false;
  int L = 1;
  while (L < d && L < 64) L <<= 1;
  const int64_t per_block = 256 / L, blocks = (rows + per_block - 1) / per_block;
  if (blocks > 0x7fffffff) return false;
  hipLaunchKernelGGL(interact_fm_kernel, dim3(unsigned(blocks)), dim3(256), 0, s, T, k, d, h, has_h, h_after && sum_last, sum_last, L, out, rows);
  return true;
}

}  // namespace infera_hip::kern
