// spatialnorm.hip -- InstanceNormalization / GroupNormalization with the activation behind them, on NCHW tensors and on channel-quad planes
// [C/4][S][4] (host/spatialnorm.hpp).  Bandwidth-bound helpers in the manner of layernorm.hip,
// with its arithmetic: centre, take the mean of the centred values out again, then the variance -- all f32.
//
// spatialnorm_fused_kernel<L, NV, MODE>: a work unit of U floats is loaded ONCE (16-byte loads when U % 4 == 0 and the pointers allow,
// else element by element) into the registers of the L lanes that own it -- L = 8 .. 64 lanes of a wave by U, or the whole 256-thread
// workgroup (then the four wave partials are joined through LDS) --, up to NV quads per lane, and written once: 8 bytes per element.
//   MODE 0: the unit is one group, a contiguous run of E floats (NCHW; channel quads with whole quad planes per group): one set of sums.
//   MODE 1: the unit is one quad plane [S][4] holding four groups (C/G = 1) or two groups of two channels: a lane keeps one set of sums
//           per component, and with two channels per group components (0, 1) and (2, 3) are added after the lanes are joined.
// The general plan, for units beyond the registers and groups that straddle quads:
// spatialnorm_stats_kernel: one workgroup per (row, group), one index function for every layout.  Pass A sums x; pass B reads x again
//   and sums d = x - mean and d^2; resid = sum(d) / E, var = sum(d^2) / E - resid^2 (resid is of the order of one rounding of the mean:
//   nothing cancels); writes (mean, resid, 1 / sqrtf(var + eps)).
// spatialnorm_apply_kernel: y = act(((x - mean) - resid) * inv * gamma[c] + beta[c]), grid-stride, one quad per lane.
// Sums are per-lane partials (lane l takes quads / elements l, l + L, ...) joined by an xor butterfly and, across waves, in the fixed
// order (w0 + w1) + (w2 + w3): deterministic, a function of the model's shapes alone (not of the row count or the call path), no atomics --
// but not the left-to-right order of a numpy restatement.  The epilogue's division, multiplication and addition are each rounded.
#include "device_common.hpp"

#include <algorithm>

#include "../host/spatialnorm.hpp"

#pragma clang fp contract(off)

namespace infera_hip::kern {

namespace {

// sum over the L lanes that own a unit; L == 256: over the workgroup (every thread of it calls this)
template <int L>
__device__ __forceinline__ float join_lanes(float v, float *lds) {
  constexpr int W = L < 64 ? L : 64;
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if constexpr (L == 256) {
    const int wave = int(threadIdx.x) >> 6;
    __syncthreads();  // (the previous join's readers are done with lds)
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    v = (lds[0] + lds[1]) + (lds[2] + lds[3]);
  }
  return v;
}

// channel of element e of a unit whose first channel is c0: NCHW c0 + e / S; channel quads c0 + 4 * (e / 4S) + e % 4
__device__ __forceinline__ int channel_of(int c0, int e, int S, bool cq) { return cq ? c0 + 4 * (e / (4 * S)) + (e & 3) : c0 + e / S; }

template <int L, int NV, int MODE, bool VEC>
__global__ __launch_bounds__(256) void spatialnorm_fused_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                float *__restrict__ y, int64_t nunits, int U, int S, int units_per_row, int chans_per_unit,
                                                                int cg, bool cq, float eps, ActParam act) {
  __shared__ float lds[4];
  constexpr int NS = MODE == 1 ? 4 : 1;  // sets of sums
  const int tid = int(threadIdx.x), lg = tid & (L - 1);
  const int64_t unit = int64_t(blockIdx.x) * (256 / L) + tid / L;
  const bool active = unit < nunits;
  const float *xp = x + unit * U;
  float r[NV * 4];
#pragma unroll
  for (int q = 0; q < NV; q++) {
    const int e0 = 4 * (lg + L * q);
#pragma unroll
    for (int j = 0; j < 4; j++) r[4 * q + j] = 0.f;
    if (!active) continue;
    if (VEC) {
      if (e0 < U) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(xp + e0);
#pragma unroll
        for (int j = 0; j < 4; j++) r[4 * q + j] = t[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (e0 + j < U) r[4 * q + j] = xp[e0 + j];
    }
  }
  // elements per group: the whole unit, or the plane's positions times the channels of a group
  const float n = MODE == 1 ? float(S * cg) : float(U);
  float sum[NS], mean[NS];
  auto join = [&](float *v) {  // lanes, then (two channels per group) the two components of a group
#pragma unroll
    for (int k = 0; k < NS; k++) v[k] = join_lanes<L>(v[k], lds);
    if constexpr (NS == 4) {
      if (cg == 2) {
        const float a = v[0] + v[1], b = v[2] + v[3];
        v[0] = v[1] = a;
        v[2] = v[3] = b;
      }
    }
  };
#pragma unroll
  for (int k = 0; k < NS; k++) sum[k] = 0.f;
#pragma unroll
  for (int i = 0; i < NV * 4; i++) sum[i & (NS - 1)] += r[i];
  join(sum);
#pragma unroll
  for (int k = 0; k < NS; k++) mean[k] = sum[k] / n;
  // centre once, then take the mean of the centred values out as well (layernorm.hip: the first mean carries a rounding error that is
  // small against a common offset of the values but not against their spread)
#pragma unroll
  for (int k = 0; k < NS; k++) sum[k] = 0.f;
#pragma unroll
  for (int q = 0; q < NV; q++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float d = 4 * (lg + L * q) + j < U ? r[4 * q + j] - mean[j & (NS - 1)] : 0.f;
      r[4 * q + j] = d;
      sum[j & (NS - 1)] += d;
    }
  join(sum);
#pragma unroll
  for (int k = 0; k < NS; k++) mean[k] = sum[k] / n;  // (resid)
#pragma unroll
  for (int k = 0; k < NS; k++) sum[k] = 0.f;
#pragma unroll
  for (int q = 0; q < NV; q++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float d = 4 * (lg + L * q) + j < U ? r[4 * q + j] - mean[j & (NS - 1)] : 0.f;
      r[4 * q + j] = d;
      sum[j & (NS - 1)] += d * d;
    }
  join(sum);
  float den[NS];
#pragma unroll
  for (int k = 0; k < NS; k++) den[k] = sqrtf(sum[k] / n + eps);
  if (!active) return;
  float *yp = y + unit * U;
  const int c0 = int(unit % units_per_row) * chans_per_unit;
  // the activation is resolved once (dispatch_act: the kinds the convolution epilogues take), so the unit stays in registers
  dispatch_act(act.kind, [&](auto kind_tag) {
    constexpr int KIND = decltype(kind_tag)::value;
#pragma unroll
    for (int q = 0; q < NV; q++) {
      const int e0 = 4 * (lg + L * q);
      if (e0 < U) {
        f32x4 t;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int e = e0 + j < U ? e0 + j : U - 1;  // (a tail quad's missing elements: computed on a valid channel, not stored)
          const int c = channel_of(c0, e, S, cq);
          t[j] = apply_act_c<KIND>(r[4 * q + j] / den[j & (NS - 1)] * gamma[c] + beta[c], act.a, act.b);
        }
        if (VEC) {
          *reinterpret_cast<f32x4 *>(yp + e0) = t;
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (e0 + j < U) yp[e0 + j] = t[j];
        }
      }
    }
  });
}

template <int L, int NV, int MODE>
void launch_fused(hipStream_t s, const float *x, const float *gamma, const float *beta, float *y, int64_t nunits, int U, int S, int units_per_row,
                  int chans_per_unit, int cg, bool cq, float eps, ActParam act) {
  const bool vec = U % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  const int per_block = 256 / L;
  const dim3 grid(unsigned((nunits + per_block - 1) / per_block));
  if (vec)
    hipLaunchKernelGGL((spatialnorm_fused_kernel<L, NV, MODE, true>), grid, dim3(256), 0, s, x, gamma, beta, y, nunits, U, S, units_per_row, chans_per_unit, cg, cq, eps, act);
  else
    hipLaunchKernelGGL((spatialnorm_fused_kernel<L, NV, MODE, false>), grid, dim3(256), 0, s, x, gamma, beta, y, nunits, U, S, units_per_row, chans_per_unit, cg, cq, eps, act);
}

template <int MODE>
void launch_fused_by_size(hipStream_t s, const float *x, const float *gamma, const float *beta, float *y, int64_t nunits, int U, int S, int units_per_row,
                          int chans_per_unit, int cg, bool cq, float eps, ActParam act) {
#define INFERA_SN_LAUNCH(L, NV) launch_fused<L, NV, MODE>(s, x, gamma, beta, y, nunits, U, S, units_per_row, chans_per_unit, cg, cq, eps, act)
  if (U <= 32) INFERA_SN_LAUNCH(8, 1);
  else if (U <= 64) INFERA_SN_LAUNCH(16, 1);
  else if (U <= 128) INFERA_SN_LAUNCH(32, 1);
  else if (U <= 256) INFERA_SN_LAUNCH(64, 1);
  else if (U <= 1024) INFERA_SN_LAUNCH(64, 4);
  else if (U <= 4096) INFERA_SN_LAUNCH(64, 16);
  else INFERA_SN_LAUNCH(256, 16);
#undef INFERA_SN_LAUNCH
}

// offset inside its row of element i of group k: contiguous groups k * E + i; groups that straddle quads by (channel, position)
__device__ __forceinline__ int64_t group_offset(int k, int i, int E, int S, int cg, bool contiguous) {
  if (contiguous) return int64_t(k) * E + i;
  const int cl = i / S, p = i - cl * S, c = k * cg + cl;
  return (int64_t(c >> 2) * S + p) * 4 + (c & 3);
}

__global__ __launch_bounds__(256) void spatialnorm_stats_kernel(const float *__restrict__ x, float *__restrict__ stats, int64_t per_row, int G, int E, int S,
                                                                int cg, bool contiguous, bool vec, float eps) {
  __shared__ float lds[4];
  const int tid = int(threadIdx.x);
  const int64_t unit = blockIdx.x;  // row * G + k
  const int k = int(unit % G);
  const float *xr = x + (unit / G) * per_row;
  const float n = float(E);
  float sum = 0.f;
  if (vec) {  // (contiguous, E % 4 == 0, 16-byte aligned rows)
    const f32x4 *x4 = reinterpret_cast<const f32x4 *>(xr + int64_t(k) * E);
    for (int q = tid; q < E / 4; q += 256) {
      const f32x4 t = x4[q];
      sum += (t[0] + t[1]) + (t[2] + t[3]);
    }
  } else {
    for (int i = tid; i < E; i += 256) sum += xr[group_offset(k, i, E, S, cg, contiguous)];
  }
  const float mean = join_lanes<256>(sum, lds) / n;
  float sd = 0.f, ss = 0.f;
  if (vec) {
    const f32x4 *x4 = reinterpret_cast<const f32x4 *>(xr + int64_t(k) * E);
    for (int q = tid; q < E / 4; q += 256) {
      const f32x4 t = x4[q];
      const float d0 = t[0] - mean, d1 = t[1] - mean, d2 = t[2] - mean, d3 = t[3] - mean;
      sd += (d0 + d1) + (d2 + d3);
      ss += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  } else {
    for (int i = tid; i < E; i += 256) {
      const float d = xr[group_offset(k, i, E, S, cg, contiguous)] - mean;
      sd += d;
      ss += d * d;
    }
  }
  const float resid = join_lanes<256>(sd, lds) / n;
  const float var = join_lanes<256>(ss, lds) / n - resid * resid;
  if (tid == 0) {
    float *o = stats + unit * 3;
    o[0] = mean;
    o[1] = resid;
    o[2] = 1.0f / sqrtf(var + eps);
  }
}

constexpr int kBlock = 256;

// VEC: one quad per lane (per_row % 4 == 0, aligned pointers); else one element per lane
template <bool VEC>
__global__ __launch_bounds__(kBlock) void spatialnorm_apply_kernel(const float *__restrict__ x, const float *__restrict__ stats, const float *__restrict__ gamma,
                                                                   const float *__restrict__ beta, float *__restrict__ y, int64_t total, int64_t per_row, int G,
                                                                   int S, int cg, bool cq, ActParam act) {
  constexpr int V = VEC ? 4 : 1;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < total; i += stride) {
    const int64_t o = i * V, row = o / per_row;
    const int e0 = int(o - row * per_row);
    const float *st = stats + row * G * 3;
    float v[V];
    if constexpr (VEC) {
      const f32x4 t = *reinterpret_cast<const f32x4 *>(x + o);
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = t[j];
    } else {
      v[0] = x[o];
    }
#pragma unroll
    for (int j = 0; j < V; j++) {
      const int c = channel_of(0, e0 + j, S, cq);
      const float *g = st + (c / cg) * 3;
      v[j] = apply_act(((v[j] - g[0]) - g[1]) * g[2] * gamma[c] + beta[c], act);
    }
    if constexpr (VEC) {
      f32x4 t;
#pragma unroll
      for (int j = 0; j < 4; j++) t[j] = v[j];
      *reinterpret_cast<f32x4 *>(y + o) = t;
    } else {
      y[o] = v[0];
    }
  }
}

bool shape_ok(int64_t rows, int C, int S, int G) {
  return C >= 1 && S >= 1 && G >= 1 && C % G == 0 && int64_t(C / G) * S <= kSpatialNormMaxE && int64_t(C) * S < (int64_t(1) << 31) && rows * G < (int64_t(1) << 31);
}

}  // namespace

bool spatialnorm_fused(hipStream_t s, const float *x, const float *gamma, const float *beta, float *y, int64_t rows, int C, int S, int G, bool cq, float eps,
                       ActParam act) {
  if (rows <= 0) return true;
  if (!shape_ok(rows, C, S, G)) return false;
  const int cg = C / G;
  switch (spatialnorm_fused_unit(C, S, G, cq)) {
    case kSpatialUnitGroup: launch_fused_by_size<0>(s, x, gamma, beta, y, rows * G, cg * S, S, G, cg, cg, cq && S > 1, eps, act); return true;
    case kSpatialUnitPlane: launch_fused_by_size<1>(s, x, gamma, beta, y, rows * (C / 4), 4 * S, S, C / 4, 4, cg, true, eps, act); return true;
    default: return false;
  }
}

bool spatialnorm_stats(hipStream_t s, const float *x, float *stats, int64_t rows, int C, int S, int G, bool cq, float eps) {
  if (rows <= 0) return true;
  if (!shape_ok(rows, C, S, G)) return false;
  const int cg = C / G, E = cg * S;
  const bool contiguous = !cq || S == 1 || cg % 4 == 0;
  const int64_t per_row = int64_t(C) * S;
  const bool vec = contiguous && E % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;  // (then per_row = G * E is whole quads too)
  hipLaunchKernelGGL(spatialnorm_stats_kernel, dim3(unsigned(rows * G)), dim3(256), 0, s, x, stats, per_row, G, E, S, cg, contiguous, vec, eps);
  return true;
}

bool spatialnorm_apply(hipStream_t s, const float *x, const float *stats, const float *gamma, const float *beta, float *y, int64_t rows, int C, int S, int G,
                       bool cq, ActParam act) {
  if (rows <= 0) return true;
  if (!shape_ok(rows, C, S, G)) return false;
  const int64_t per_row = int64_t(C) * S;
  const bool vec = per_row % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  const int64_t total = vec ? rows * per_row / 4 : rows * per_row;
  const unsigned grid = unsigned(std::min<int64_t>((total + kBlock - 1) / kBlock, 8192));
  if (vec) hipLaunchKernelGGL(spatialnorm_apply_kernel<true>, dim3(grid), dim3(kBlock), 0, s, x, stats, gamma, beta, y, total, per_row, G, S, C / G, cq && S > 1, act);
  else hipLaunchKernelGGL(spatialnorm_apply_kernel<false>, dim3(grid), dim3(kBlock), 0, s, x, stats, gamma, beta, y, total, per_row, G, S, C / G, cq && S > 1, act);
  return true;
}

}  // namespace infera_hip::kern
