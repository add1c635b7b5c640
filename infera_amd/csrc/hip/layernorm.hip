// layernorm.hip -- LayerNorm over the last axis and the mean over the time axis, for Transformer encoders.
//
// layernorm_kernel: y = (x - mean) / sqrt(var + eps) * gamma + beta over each vector of E elements.  Bandwidth-bound, so ONE pass over
// HBM: a vector is loaded once (16-byte loads when E % 4 == 0 and the pointers allow) into the registers of the G lanes that own it.
// G = 8 / 16 / 32 / 64 by E, so a wave serves 8 vectors of E <= 32 at a time; up to 16 quads per lane: E <= 4096 (host/attention.hpp).
// The arithmetic runs on those registers, all f32:
//   mean = sum / E;  d = x - mean;  d -= sum(d) / E;  var = sum(d^2) / E;  y = d / sqrtf(var + eps) * gamma + beta.
// The third step takes the rounding error of the first mean out again.  It matters when the values share a large offset, and it runs
// for every vector (a test for "needs no correction" would cost the same reduction): registers only, no memory traffic.
// Sums are per-lane partial sums (lane l of the group takes quads l, l + G, ...) joined by an xor butterfly: fixed order,
// deterministic, but not the left-to-right order of a numpy restatement.
// rmsnorm_kernel (RMSNormalization, opset 23): y = x / sqrtf(sum(x^2) / E + eps) * gamma, as the specification's function body writes
// it: a true division, then one multiply, each rounded.  The same lane layout, loads and butterfly with ONE reduction (the squares are
// accumulated per lane, fused multiply-adds where the compiler forms them): deterministic, not bit-reproducible by numpy.
// mean_time_kernel: out[r, e] = (sum over t in order of x[r, t, e]) / T, one thread per (row, e): coalesced over e.
// mean_time_masked_kernel: the same under a row's own mask (INTEGRATION.md 2.6 "Padded sequences"): the sum over the kept steps / max(count, clip).
#include "device_common.hpp"

#include "../host/attention.hpp"

namespace infera_hip::kern {

namespace {

template <int G, int NV, bool VEC>
__global__ __launch_bounds__(256) void layernorm_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                        float *__restrict__ y, int64_t nvec, int E, float eps) {
  const int tid = int(threadIdx.x), lg = tid & (G - 1);
  const int64_t vec = int64_t(blockIdx.x) * (256 / G) + tid / G;
  const bool active = vec < nvec;
  const float *xp = x + vec * E;
  float r[NV * 4];
#pragma unroll
  for (int q = 0; q < NV; q++) {
    const int e0 = 4 * (lg + G * q);
#pragma unroll
    for (int j = 0; j < 4; j++) r[4 * q + j] = 0.f;
    if (!active) continue;
    if (VEC) {
      if (e0 < E) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(xp + e0);
#pragma unroll
        for (int j = 0; j < 4; j++) r[4 * q + j] = t[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (e0 + j < E) r[4 * q + j] = xp[e0 + j];
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NV * 4; i++) sum += r[i];
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  const float mean = sum / float(E);
  // the f32 sum of values with a large common offset carries a rounding error that is small against the offset but not against the
  // spread (1000 +- 1 over 768 elements: ~6e-5, where the bar allows 1e-6 near a zero crossing): centre once, then take the mean of the
  // centred values out as well -- x - mean is exact for values near the mean, and their sum is small, hence accurate
  float rs = 0.f;
#pragma unroll
  for (int q = 0; q < NV; q++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float d = 4 * (lg + G * q) + j < E ? r[4 * q + j] - mean : 0.f;
      r[4 * q + j] = d;
      rs += d;
    }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) rs += __shfl_xor(rs, o);
  const float resid = rs / float(E);
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < NV; q++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float d = 4 * (lg + G * q) + j < E ? r[4 * q + j] - resid : 0.f;
      r[4 * q + j] = d;
      ss += d * d;
    }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  const float den = sqrtf(ss / float(E) + eps);
  if (!active) return;
  float *yp = y + vec * E;
#pragma unroll
  for (int q = 0; q < NV; q++) {
    const int e0 = 4 * (lg + G * q);
    if (VEC) {
      if (e0 < E) {
        const f32x4 g = *reinterpret_cast<const f32x4 *>(gamma + e0);
        f32x4 t;
#pragma unroll
        for (int j = 0; j < 4; j++) t[j] = r[4 * q + j] / den * g[j] + (beta ? beta[e0 + j] : 0.f);
        *reinterpret_cast<f32x4 *>(yp + e0) = t;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (e0 + j < E) yp[e0 + j] = r[4 * q + j] / den * gamma[e0 + j] + (beta ? beta[e0 + j] : 0.f);
    }
  }
}

template <int G, int NV>
void launch_ln(hipStream_t s, const float *x, const float *gamma, const float *beta, float *y, int64_t nvec, int E, float eps) {
  const bool vec = E % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(gamma)) & 15) == 0;
  const int per_block = 256 / G;
  const dim3 grid(unsigned((nvec + per_block - 1) / per_block));
  if (vec) hipLaunchKernelGGL((layernorm_kernel<G, NV, true>), grid, dim3(256), 0, s, x, gamma, beta, y, nvec, E, eps);
  else hipLaunchKernelGGL((layernorm_kernel<G, NV, false>), grid, dim3(256), 0, s, x, gamma, beta, y, nvec, E, eps);
}

// RMSNormalization: the lane layout and the butterfly of layernorm_kernel with one reduction.  No centring: the sum of squares has no
// cancellation to repair
template <int G, int NV, bool VEC>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float *__restrict__ x, const float *__restrict__ gamma, float *__restrict__ y, int64_t nvec, int E,
                                                      float eps) {
  const int tid = int(threadIdx.x), lg = tid & (G - 1);
  const int64_t vec = int64_t(blockIdx.x) * (256 / G) + tid / G;
  const bool active = vec < nvec;
  const float *xp = x + vec * E;
  float r[NV * 4];
#pragma unroll
  for (int q = 0; q < NV; q++) {
    const int e0 = 4 * (lg + G * q);
#pragma unroll
    for (int j = 0; j < 4; j++) r[4 * q + j] = 0.f;
    if (!active) continue;
    if (VEC) {
      if (e0 < E) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(xp + e0);
#pragma unroll
        for (int j = 0; j < 4; j++) r[4 * q + j] = t[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (e0 + j < E) r[4 * q + j] = xp[e0 + j];
    }
  }
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV * 4; i++) ss += r[i] * r[i];  // (elements beyond E are zero)
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  const float den = sqrtf(ss / float(E) + eps);
  if (!active) return;
  float *yp = y + vec * E;
#pragma unroll
  for (int q = 0; q < NV; q++) {
    const int e0 = 4 * (lg + G * q);
    if (VEC) {
      if (e0 < E) {
        const f32x4 g = *reinterpret_cast<const f32x4 *>(gamma + e0);
        f32x4 t;
#pragma unroll
        for (int j = 0; j < 4; j++) t[j] = r[4 * q + j] / den * g[j];
        *reinterpret_cast<f32x4 *>(yp + e0) = t;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (e0 + j < E) yp[e0 + j] = r[4 * q + j] / den * gamma[e0 + j];
    }
  }
}

template <int G, int NV>
void launch_rms(hipStream_t s, const float *x, const float *gamma, float *y, int64_t nvec, int E, float eps) {
  const bool vec = E % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(gamma)) & 15) == 0;
  const int per_block = 256 / G;
  const dim3 grid(unsigned((nvec + per_block - 1) / per_block));
  if (vec) hipLaunchKernelGGL((rmsnorm_kernel<G, NV, true>), grid, dim3(256), 0, s, x, gamma, y, nvec, E, eps);
  else hipLaunchKernelGGL((rmsnorm_kernel<G, NV, false>), grid, dim3(256), 0, s, x, gamma, y, nvec, E, eps);
}

__global__ __launch_bounds__(256) void mean_time_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t n, int T, int E) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t row = i / E;
  const float *xp = x + row * T * E + (i - row * E);
  float sum = 0.f;
  for (int t = 0; t < T; t++) sum += xp[int64_t(t) * E];
  y[i] = sum / float(T);
}

// one thread per (row, e) as above; the mask value of step t is the same address in all lanes of a row, and the branch is per row
__global__ __launch_bounds__(256) void mean_time_masked_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t n, int T, int E,
                                                               const float *__restrict__ rm, int64_t rm_ld, int rm_off, float rm_cmp, bool rm_int, float clip) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t row = i / E;
  const float *xp = x + row * T * E + (i - row * E);
  const float *mp = rm + row * rm_ld + rm_off;
  float sum = 0.f;
  int count = 0;
  auto keeps = [&](int t) {
    const float mv = mp[t];
    return (rm_int ? truncf(mv) : mv) != rm_cmp;
  };
  int t = 0;
  for (; t + 4 <= T; t += 4) {  // four steps' loads in flight; a masked step's load is not issued, and the sum keeps its order
    bool k[4];
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) k[j] = keeps(t + j);
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = k[j] ? xp[int64_t(t + j) * E] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (k[j]) {
        sum += v[j];
        count++;
      }
  }
  for (; t < T; t++)
    if (keeps(t)) {
      sum += xp[int64_t(t) * E];
      count++;
    }
  y[i] = sum / fmaxf(float(count), clip);
}

}  // namespace

bool layernorm(hipStream_t s, const float *x, const float *gamma, const float *beta, float *y, int64_t nvec, int E, float eps) {
  if (nvec <= 0) return true;
  if (E < 1 || E > kLnMaxE || nvec > (int64_t(1) << 33)) return false;
  if (E <= 32) launch_ln<8, 1>(s, x, gamma, beta, y, nvec, E, eps);
  else if (E <= 64) launch_ln<16, 1>(s, x, gamma, beta, y, nvec, E, eps);
  else if (E <= 128) launch_ln<32, 1>(s, x, gamma, beta, y, nvec, E, eps);
  else if (E <= 256) launch_ln<64, 1>(s, x, gamma, beta, y, nvec, E, eps);
  else if (E <= 1024) launch_ln<64, 4>(s, x, gamma, beta, y, nvec, E, eps);
  else launch_ln<64, 16>(s, x, gamma, beta, y, nvec, E, eps);
  return true;
}

bool rmsnorm(hipStream_t s, const float *x, const float *gamma, float *y, int64_t nvec, int E, float eps) {
  if (nvec <= 0) return true;
  if (E < 1 || E > kLnMaxE || nvec > (int64_t(1) << 33)) return false;
  if (E <= 32) launch_rms<8, 1>(s, x, gamma, y, nvec, E, eps);
  else if (E <= 64) launch_rms<16, 1>(s, x, gamma, y, nvec, E, eps);
  else if (E <= 128) launch_rms<32, 1>(s, x, gamma, y, nvec, E, eps);
  else if (E <= 256) launch_rms<64, 1>(s, x, gamma, y, nvec, E, eps);
  else if (E <= 1024) launch_rms<64, 4>(s, x, gamma, y, nvec, E, eps);
  else launch_rms<64, 16>(s, x, gamma, y, nvec, E, eps);
  return true;
}

void mean_time(hipStream_t s, const float *x, float *y, int64_t rows, int T, int E) {
  const int64_t n = rows * E;
  if (n <= 0) return;
  hipLaunchKernelGGL(mean_time_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, x, y, n, T, E);
}

void mean_time_masked(hipStream_t s, const float *x, float *y, int64_t rows, int T, int E, const float *rm, int64_t rm_ld, int rm_off, float rm_cmp,
                      bool rm_int, float clip) {
  const int64_t n = rows * E;
  if (n <= 0) return;
  hipLaunchKernelGGL(mean_time_masked_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, x, y, n, T, E, rm, rm_ld, rm_off, rm_cmp, rm_int, clip);
}

}  // namespace infera_hip::kern
