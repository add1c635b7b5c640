// rotary.hip -- the Rotary step (INTEGRATION.md section 2.6 "Rotary position embeddings"): rotary position embedding of a
// window x [rows, T, h * dh], read through a (ld, off) view -- a cut of a packed projection is read where it lies -- into a dense
// [rows, T, h * dh] window.  For step t, head g and column j < rd of the head
//     y[j] = fl(fl(x[j] * A[t, j]) + fl(x[partner(j)] * B[t, j]))       three separately rounded f32 operations (contraction is off)
// with partner(j) = j +- rd / 2 (half) or j ^ 1 (interleaved); columns j >= rd are bit copies.  A, B: [T, rd] f32 tables built at load.
// One read and one write of the window; the tables (at most 1024 * 128 * 8 bytes) stay in cache.  HBM-bound, no LDS, no atomics.
//
// rotary_kernel<VEC, INTER>: the window is a list of units, 64-bit index i = vec * UV + k over the rows * T vectors of a call and the UV
//   units of a vector.  A grid of at most kMaxBlocks work groups of 256 threads strides over it; the stride's quotient and remainder by UV
//   (and the quotient's remainder by T) come from the host, so that vec, k and t advance by additions and the only divisions are the 32-bit
//   ones of a thread's first unit and of k by the units per head.
//   VEC = false: a unit is one output element (UV = h * dh): any geometry.
//   VEC = true : 16-byte loads and stores; needs off, ld and dh multiples of 4, rd / 2 (half) or rd (interleaved) a multiple of 4 and
//     16-byte aligned pointers; the launcher chooses per launch, uniformly.  Interleaved: a unit is one quad of 4 columns (dh / 4 per head),
//     whose partners are inside it.  Half: a unit of the rotated part is the quad at column c < rd / 2 TOGETHER with its partner quad at
//     c + rd / 2 -- two loads, two stores, nothing read twice -- (rd / 8 per head); the (dh - rd) / 4 pass-through quads follow.
// A row's bits depend on the model and that row only.  Element offsets are 64-bit: rows * T * h * dh passes 2^32 in a device-resident call.
#include "device_common.hpp"

#include <algorithm>

#include "../host/attention.hpp"

#pragma clang fp contract(off)

namespace infera_hip::kern {

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;  // 8 work groups per CU of 256: the rest of a long call is walked by the stride

struct RotaryArgs {
  const float *x, *A, *B;
  float *y;
  int64_t nvec, ld, off;       // vectors (rows * T); floats between two vectors of x; first column of head 0
  int T, dh, rd, E;            // E = h * dh
  unsigned UV, U;              // units per vector and per head
  unsigned dvec, dk, dt;       // the grid's stride G = gridDim.x * kBlock as G / UV, G % UV and (G / UV) % T
};

template <bool VEC, bool INTER>
__global__ __launch_bounds__(kBlock) void rotary_kernel(const RotaryArgs a) {
  const unsigned i0 = blockIdx.x * unsigned(kBlock) + threadIdx.x;  // (< kMaxBlocks * kBlock)
  const unsigned v0 = i0 / a.UV;
  int64_t vec = v0;
  unsigned k = i0 - v0 * a.UV;
  unsigned t = v0 % unsigned(a.T);
  const int half = a.rd >> 1;
  while (vec < a.nvec) {
    const unsigned g = k / a.U, u = k - g * a.U;
    const float *xh = a.x + vec * a.ld + a.off + int64_t(g) * a.dh;
    float *yh = a.y + vec * a.E + int64_t(g) * a.dh;
    const float *At = a.A + int64_t(t) * a.rd, *Bt = a.B + int64_t(t) * a.rd;
    if constexpr (!VEC) {
      const int j = int(u);
      float v = xh[j];
      if (j < a.rd) {
        const int pj = INTER ? (j ^ 1) : (j < half ? j + half : j - half);
        const float p = xh[pj];
        const float m0 = v * At[j], m1 = p * Bt[j];
        v = m0 + m1;
      }
      yh[j] = v;
    } else if constexpr (INTER) {
      const int c = 4 * int(u);
      f32x4 v = *reinterpret_cast<const f32x4 *>(xh + c);
      if (c < a.rd) {
        const f32x4 p = {v[1], v[0], v[3], v[2]};
        const f32x4 m0 = v * *reinterpret_cast<const f32x4 *>(At + c), m1 = p * *reinterpret_cast<const f32x4 *>(Bt + c);
        v = m0 + m1;
      }
      *reinterpret_cast<f32x4 *>(yh + c) = v;
    } else {
      const int pairs = a.rd >> 3;
      if (int(u) < pairs) {
        const int c = 4 * int(u), d = c + half;
        const f32x4 lo = *reinterpret_cast<const f32x4 *>(xh + c), hi = *reinterpret_cast<const f32x4 *>(xh + d);
        const f32x4 l0 = lo * *reinterpret_cast<const f32x4 *>(At + c), l1 = hi * *reinterpret_cast<const f32x4 *>(Bt + c);
        const f32x4 h0 = hi * *reinterpret_cast<const f32x4 *>(At + d), h1 = lo * *reinterpret_cast<const f32x4 *>(Bt + d);
        *reinterpret_cast<f32x4 *>(yh + c) = l0 + l1;
        *reinterpret_cast<f32x4 *>(yh + d) = h0 + h1;
      } else {
        const int c = a.rd + 4 * (int(u) - pairs);
        *reinterpret_cast<f32x4 *>(yh + c) = *reinterpret_cast<const f32x4 *>(xh + c);
      }
    }
    vec += a.dvec;
    k += a.dk;
    t += a.dt;
    if (k >= a.UV) k -= a.UV, vec++, t++;
    if (t >= unsigned(a.T)) t -= unsigned(a.T);
  }
}

}  // namespace

bool rotary(hipStream_t s, const float *x, int64_t ld, int64_t off, const float *A, const float *B, float *y, int64_t rows, int T, int heads, int dh, int rd,
            bool interleaved) {
  if (T < 1 || T > kAttnMaxT || dh < 2 || dh > kAttnMaxDh || heads < 1 || heads > kAttnMaxHeads || rd < 2 || rd > dh || (rd & 1) != 0 || off < 0 ||
      off + int64_t(heads) * dh > ld || !A || !B)
    return false;
  if (rows <= 0) return true;
  auto aligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = rotary_vec4(ld, off, dh, rd, interleaved) && aligned(x) && aligned(y) && aligned(A) && aligned(B);
  RotaryArgs a;
  a.x = x, a.A = A, a.B = B, a.y = y;
  a.nvec = rows * T, a.ld = ld, a.off = off;
  a.T = T, a.dh = dh, a.rd = rd, a.E = heads * dh;
  a.U = unsigned(!vec ? dh : interleaved ? dh / 4 : rd / 8 + (dh - rd) / 4);
  a.UV = unsigned(heads) * a.U;  // (<= 1024 * 128)
  const int64_t units = a.nvec * int64_t(a.UV);
  const unsigned grid = unsigned(std::min<int64_t>((units + kBlock - 1) / kBlock, kMaxBlocks));
  const unsigned G = grid * unsigned(kBlock);
  a.dvec = G / a.UV, a.dk = G % a.UV, a.dt = a.dvec % unsigned(T);
  if (vec && interleaved) hipLaunchKernelGGL((rotary_kernel<true, true>), dim3(grid), dim3(kBlock), 0, s, a);
  else if (vec) hipLaunchKernelGGL((rotary_kernel<true, false>), dim3(grid), dim3(kBlock), 0, s, a);
  else if (interleaved) hipLaunchKernelGGL((rotary_kernel<false, true>), dim3(grid), dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL((rotary_kernel<false, false>), dim3(grid), dim3(kBlock), 0, s, a);
  return true;
}

}  // namespace infera_hip::kern
