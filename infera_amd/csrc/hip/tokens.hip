// tokens.hip -- the Tokens step (host/tokens.hpp): the [rows, C, S] tensor of a convolutional step
// becomes the flat window [rows, T = P + S, E = C] a Transformer encoder reads, with P constant rows (class tokens) in front and the
// position table added in the store epilogue.  Pure data movement plus at most one rounded f32 addition per element: HBM-bound.
//
// tokens_nchw_kernel<VIN, VOUT>: from NCHW this is a transposition of each image's [C][S] matrix.  A work group of 256 threads moves one tile
//   of kTC = 32 channels x kTS = 64 positions through LDS.  Load: 16 lanes read one channel's 64 positions (256 contiguous bytes, 16 bytes per
//   lane when S % 4 == 0 and the pointer allows -- VIN --, else 64 lanes one word each) and write them as words into tile[c][s].  Store: 8 lanes
//   write 32 channels of one position (128 contiguous bytes, 16 bytes per lane when C % 4 == 0 and the pointers allow -- VOUT --, else 32 lanes
//   one word each) from tile[4 c4 + j][s].  A tile row is 65 words, so that the store phase's reads -- word 65 (4 c4 + j) + s for the 8 quads
//   and 4 positions of a half wave, banks 4 c4 + s + j -- and the scalar form's -- banks c + s -- meet 32 distinct banks.  (The load phase's
//   word writes are two-way conflicted: 16 quads x 2 channels of a half wave fall on 16 banks.  LDS time stays far below the HBM time.)
// tokens_cq_kernel<VEC>: in channel-quad planes [C/4][S][4] a position's four channels are adjacent, so the element moved is a quad and no LDS
//   is needed: lane (q, s) of an 8 quads x 64 positions tile reads quad q of position s -- 8 lanes with one q read 128 contiguous bytes --
//   and writes it at column 4 q of window row P + s -- 8 lanes with one s write 128 contiguous bytes.
// Both: the work groups of position tile 0 also write their channels of the P constant rows.  Rows are walked by blockIdx.y with a stride;
// nothing is shared between rows, there are no atomics, and a row's bits depend on the model and that row only.  Offsets are 64-bit.
#include "device_common.hpp"

#include <algorithm>

#include "../host/tokens.hpp"

#pragma clang fp contract(off)

namespace infera_hip::kern {

namespace {

constexpr int kBlock = 256;
constexpr int kTC = 32, kTS = 64;    // the NCHW tile: channels x positions
constexpr int kQT = 8, kQS = 64;     // the channel-quad tile: quads x positions
constexpr int kMaxRowBlocks = 32768; // blockIdx.y

// the P constant rows of the window at yr, columns c0 .. c0 + n - 1
__device__ __forceinline__ void store_prefix(const float *__restrict__ prefix, const float *__restrict__ pos, float *__restrict__ yr, int P, int C, int c0, int n) {
  for (int i = int(threadIdx.x); i < P * n; i += kBlock) {
    const int p = i / n, c = c0 + i % n;
    if (c >= C) continue;
    float v = prefix[int64_t(p) * C + c];
    if (pos) v = v + pos[int64_t(p) * C + c];
    yr[int64_t(p) * C + c] = v;
  }
}

template <bool VIN, bool VOUT>
__global__ __launch_bounds__(kBlock) void tokens_nchw_kernel(const float *__restrict__ x, const float *__restrict__ prefix, const float *__restrict__ pos,
                                                            float *__restrict__ y, int64_t rows, int C, int S, int P, int tiles_s) {
  __shared__ float tile[kTC][kTS + 1];
  const int tid = int(threadIdx.x);
  const int s0 = int(blockIdx.x % unsigned(tiles_s)) * kTS, c0 = int(blockIdx.x / unsigned(tiles_s)) * kTC;
  const int64_t T = int64_t(P) + S;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const float *xr = x + r * C * S;
    float *yr = y + r * T * C;
    if constexpr (VIN) {  // (S % 4 == 0: a quad that starts inside the tensor lies inside it)
      const int s = 4 * (tid & 15);
#pragma unroll
      for (int k = 0; k < kTC / 16; k++) {
        const int c = (tid >> 4) + 16 * k;
        if (c0 + c < C && s0 + s < S) {
          const f32x4 v = *reinterpret_cast<const f32x4 *>(xr + int64_t(c0 + c) * S + s0 + s);
          tile[c][s] = v[0], tile[c][s + 1] = v[1], tile[c][s + 2] = v[2], tile[c][s + 3] = v[3];
        }
      }
    } else {
      const int s = tid & 63;
#pragma unroll
      for (int k = 0; k < kTC / 4; k++) {
        const int c = (tid >> 6) + 4 * k;
        if (c0 + c < C && s0 + s < S) tile[c][s] = xr[int64_t(c0 + c) * S + s0 + s];
      }
    }
    __syncthreads();
    if constexpr (VOUT) {  // (C % 4 == 0)
      const int c = 4 * (tid & 7);
#pragma unroll
      for (int k = 0; k < kTS / 32; k++) {
        const int s = (tid >> 3) + 32 * k;
        if (c0 + c < C && s0 + s < S) {
          const int64_t o = (int64_t(P) + s0 + s) * C + c0 + c;
          f32x4 v = {tile[c][s], tile[c + 1][s], tile[c + 2][s], tile[c + 3][s]};
          if (pos) v = v + *reinterpret_cast<const f32x4 *>(pos + o);
          *reinterpret_cast<f32x4 *>(yr + o) = v;
        }
      }
    } else {
      const int c = tid & 31;
#pragma unroll
      for (int k = 0; k < kTS / 8; k++) {
        const int s = (tid >> 5) + 8 * k;
        if (c0 + c < C && s0 + s < S) {
          const int64_t o = (int64_t(P) + s0 + s) * C + c0 + c;
          float v = tile[c][s];
          if (pos) v = v + pos[o];
          yr[o] = v;
        }
      }
    }
    if (s0 == 0 && P > 0) store_prefix(prefix, pos, yr, P, C, c0, kTC);
    __syncthreads();  // (the next row's load overwrites the tile)
  }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void tokens_cq_kernel(const float *__restrict__ x, const float *__restrict__ prefix, const float *__restrict__ pos,
                                                          float *__restrict__ y, int64_t rows, int Q, int S, int P, int tiles_s) {
  const int tid = int(threadIdx.x);
  const int s0 = int(blockIdx.x % unsigned(tiles_s)) * kQS, q = int(blockIdx.x / unsigned(tiles_s)) * kQT + (tid & 7);
  const int C = 4 * Q;
  const int64_t T = int64_t(P) + S;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const float *xr = x + r * C * S;
    float *yr = y + r * T * C;
#pragma unroll
    for (int k = 0; k < kQS / 32; k++) {
      const int s = s0 + (tid >> 3) + 32 * k;
      if (q >= Q || s >= S) continue;
      const int64_t i = (int64_t(q) * S + s) * 4, o = (int64_t(P) + s) * C + 4 * q;
      if constexpr (VEC) {
        f32x4 v = *reinterpret_cast<const f32x4 *>(xr + i);
        if (pos) v = v + *reinterpret_cast<const f32x4 *>(pos + o);
        *reinterpret_cast<f32x4 *>(yr + o) = v;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          float v = xr[i + j];
          if (pos) v = v + pos[o + j];
          yr[o + j] = v;
        }
      }
    }
    if (s0 == 0 && P > 0) store_prefix(prefix, pos, yr, P, C, 4 * (q - (tid & 7)), 4 * kQT);
  }
}

}  // namespace

bool tokens(hipStream_t s, const float *X, const float *prefix, const float *pos, float *Y, int64_t rows, int C, int S, int P, bool cq) {
  if (C < 1 || S < 1 || P < 0 || C > kTokensMaxC || S > kTokensMaxS || P > kTokensMaxPrefix || (P > 0 && !prefix) || (cq && C % 4 != 0)) return false;
  if (rows <= 0) return true;
  const unsigned gy = unsigned(std::min<int64_t>(rows, kMaxRowBlocks));
  const bool pos_ok = !pos || (reinterpret_cast<uintptr_t>(pos) & 15) == 0;
  const bool y_ok = (reinterpret_cast<uintptr_t>(Y) & 15) == 0 && pos_ok, x_ok = (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  if (cq) {
    const int Q = C / 4, tiles_s = (S + kQS - 1) / kQS;
    const dim3 grid(unsigned(tiles_s) * unsigned((Q + kQT - 1) / kQT), gy);
    if (x_ok && y_ok) hipLaunchKernelGGL((tokens_cq_kernel<true>), grid, dim3(kBlock), 0, s, X, prefix, pos, Y, rows, Q, S, P, tiles_s);
    else hipLaunchKernelGGL((tokens_cq_kernel<false>), grid, dim3(kBlock), 0, s, X, prefix, pos, Y, rows, Q, S, P, tiles_s);
    return true;
  }
  const int tiles_s = (S + kTS - 1) / kTS;
  const dim3 grid(unsigned(tiles_s) * unsigned((C + kTC - 1) / kTC), gy);
  const bool vin = x_ok && S % 4 == 0, vout = y_ok && C % 4 == 0;
  if (vin && vout) hipLaunchKernelGGL((tokens_nchw_kernel<true, true>), grid, dim3(kBlock), 0, s, X, prefix, pos, Y, rows, C, S, P, tiles_s);
  else if (vin) hipLaunchKernelGGL((tokens_nchw_kernel<true, false>), grid, dim3(kBlock), 0, s, X, prefix, pos, Y, rows, C, S, P, tiles_s);
  else if (vout) hipLaunchKernelGGL((tokens_nchw_kernel<false, true>), grid, dim3(kBlock), 0, s, X, prefix, pos, Y, rows, C, S, P, tiles_s);
  else hipLaunchKernelGGL((tokens_nchw_kernel<false, false>), grid, dim3(kBlock), 0, s, X, prefix, pos, Y, rows, C, S, P, tiles_s);
  return true;
}

}  // namespace infera_hip::kern
