// channelnorm.hip -- LayerNorm over the channel axis at each pixel of an [N,C,H,W] tensor, with the activation behind it, on NCHW tensors and
// on channel-quad planes [C/4][S][4] (host/channelnorm.hpp).  A bandwidth-bound helper with the
// arithmetic of layernorm.hip and spatialnorm.hip: centre, take the mean of the centred values out again, then the variance -- all f32.
//
// Lanes run along the pixels, the flattened (row, s) index, so a wave's loads at one channel (NCHW: 256 B) or one quad (channel quads:
// 1 KiB of 16-byte loads when the pointers allow, else element by element) are contiguous wherever the 64 pixels lie in one image.  The
// reduction over C is the lane's own loop, in channel order.  With C > 32 the four waves of a workgroup share one tile of 64 pixels and
// split the channels (a unit = a channel or a quad; host/channelnorm.hpp channelnorm_split); their partial sums are joined
// through LDS in the fixed order (w0 + w1) + (w2 + w3).  With C <= 32 every wave takes 64 pixels of its own and all the channels.
//   channelnorm_regs_small_kernel<R, CQ, VEC> (C <= 32) / channelnorm_regs_kernel<R, CQ, VEC>: a lane keeps its units in registers: x is
//     read once and written once, 8 bytes per element (but for a remainder of C % (R units) channels, which one wave reads again).
//   channelnorm_reread_kernel<WS, CQ, VEC>: the same arithmetic, x read again for each centring and for the write.
// The order of the sums is a function of C, the layout and the form alone (not of the row count, the pixel's place in its tile or the call
// path); no atomics.  A lane writes only what it read, so the step may run in place.  The epilogue's division, multiplication and addition
// are each rounded.
#include "device_common.hpp"

#include <algorithm>

#include "../host/channelnorm.hpp"

#pragma clang fp contract(off)

namespace infera_hip::kern {

namespace {

constexpr int kTile = 64;  // pixels of a tile: one per lane of a wave

// sum of the partials of the WS waves that share a pixel (every thread of the workgroup calls this; each join has an LDS array of its own)
template <int WS>
__device__ __forceinline__ float join_waves(float v, float (*lds)[kTile]) {
  if constexpr (WS == 1) {
    return v;
  } else {
    const int lane = int(threadIdx.x) & 63, wave = int(threadIdx.x) >> 6;
    lds[wave][lane] = v;
    __syncthreads();
    return (lds[0][lane] + lds[1][lane]) + (lds[2][lane] + lds[3][lane]);
  }
}

// one unit of a pixel: a channel (NCHW) or a quad of channels (channel quads; VEC: one 16-byte access)
template <bool CQ, bool VEC>
__device__ __forceinline__ void load_unit(const float *p, float *r) {
  if constexpr (!CQ) {
    r[0] = p[0];
  } else if constexpr (VEC) {
    const f32x4 t = *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = t[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = p[j];
  }
}
template <bool CQ, bool VEC>
__device__ __forceinline__ void store_unit(float *p, const float *r) {
  if constexpr (!CQ) {
    p[0] = r[0];
  } else if constexpr (VEC) {
    f32x4 t;
#pragma unroll
    for (int j = 0; j < 4; j++) t[j] = r[j];
    *reinterpret_cast<f32x4 *>(p) = t;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) p[j] = r[j];
  }
}

// the lane's pixel and its slice of it: the offset of its first unit and how many units it has.  The slice is the wave's (u0 and nu are
// wave-uniform, so `i < nu` is a scalar comparison, not a lane mask per unit).  A tail tile's lanes beyond the last pixel take the last
// pixel again -- every access stays inside the tensor -- and store nothing (active)
template <int WS, bool CQ>
struct Slice {
  int64_t off, ustride;
  int u0, nu;
  bool active;
  __device__ __forceinline__ Slice(int64_t P, int C, int S, int units, int per_wave) {
    const int tid = int(threadIdx.x);
    const int64_t p = WS == 1 ? int64_t(blockIdx.x) * 256 + tid : int64_t(blockIdx.x) * kTile + (tid & 63);
    active = p < P;
    const int64_t pc = active ? p : P - 1;
    u0 = WS == 1 ? 0 : __builtin_amdgcn_readfirstlane(tid >> 6) * per_wave;
    nu = min(per_wave, units - u0);
    nu = nu < 0 ? 0 : nu;
    ustride = int64_t(CQ ? 4 : 1) * S;
    const int64_t n = pc / S, s = pc - n * S;
    off = n * int64_t(C) * S + (CQ ? 4 : 1) * s + u0 * ustride;
  }
};

// C <= 32: every wave takes 64 pixels of its own and all `units` (<= R) of them
template <int R, bool CQ, bool VEC>
__global__ __launch_bounds__(256) void channelnorm_regs_small_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                     float *__restrict__ y, int64_t P, int C, int S, int units, float eps, ActParam act) {
  constexpr int V = CQ ? 4 : 1;
  const Slice<1, CQ> sl(P, C, S, units, units);
  const float *xp = x + sl.off;
  float r[R * V];
#pragma unroll
  for (int i = 0; i < R; i++) {
#pragma unroll
    for (int j = 0; j < V; j++) r[i * V + j] = 0.f;
    if (i < sl.nu) load_unit<CQ, VEC>(xp + i * sl.ustride, r + i * V);
  }
  const float n = float(C);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < R * V; i++) sum += r[i];
  const float mean = sum / n;
  // centre once, then take the mean of the centred values out as well (layernorm.hip: the first mean carries a rounding error that is
  // small against a common offset of the values but not against their spread)
  sum = 0.f;
#pragma unroll
  for (int i = 0; i < R; i++)
#pragma unroll
    for (int j = 0; j < V; j++) {
      const float d = i < sl.nu ? r[i * V + j] - mean : 0.f;
      r[i * V + j] = d;
      sum += d;
    }
  const float resid = sum / n;
  sum = 0.f;
#pragma unroll
  for (int i = 0; i < R; i++)
#pragma unroll
    for (int j = 0; j < V; j++) {
      const float d = i < sl.nu ? r[i * V + j] - resid : 0.f;
      r[i * V + j] = d;
      sum += d * d;
    }
  const float den = sqrtf(sum / n + eps);
  float *yp = y + sl.off;
  // the activation is resolved once (dispatch_act: the kinds the convolution epilogues take), so the slice stays in registers
  dispatch_act(act.kind, [&](auto kind_tag) {
    constexpr int KIND = decltype(kind_tag)::value;
#pragma unroll
    for (int i = 0; i < R; i++) {
      if (i < sl.nu) {
        float t[V];
#pragma unroll
        for (int j = 0; j < V; j++) {
          const int c = i * V + j;
          float v = r[i * V + j] / den * gamma[c];
          if (beta) v = v + beta[c];
          t[j] = apply_act_c<KIND>(v, act.a, act.b);
        }
        if (sl.active) store_unit<CQ, VEC>(yp + i * sl.ustride, t);
      }
    }
  });
}

// C > 32: the four waves share a tile.  Wave w < units / R holds units [w R, (w + 1) R) in registers -- whole slices, so no unit of the
// unrolled loops needs a predicate --; the wave behind them takes the remainder (units % R, possibly none) in a run-time loop that reads
// x again, as the re-read form does.  gamma and beta go through LDS (written first, read behind the joins' barriers): read straight from
// memory with their wave-uniform indices they would be hundreds of scalar loads in flight at once, more than there are scalar registers.
template <int R, bool CQ, bool VEC>
__global__ __launch_bounds__(256) void channelnorm_regs_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                               float *__restrict__ y, int64_t P, int C, int S, int units, float eps, ActParam act) {
  constexpr int V = CQ ? 4 : 1;
  __shared__ float lds[3][4][kTile];
  __shared__ float gb[2][4 * R * V];
  for (int c = int(threadIdx.x); c < C; c += 256) {
    gb[0][c] = gamma[c];
    gb[1][c] = beta ? beta[c] : 0.f;
  }
  const Slice<4, CQ> sl(P, C, S, units, R);  // (nu = R for the whole slices, the remainder behind them, 0 behind that)
  const bool whole = sl.nu == R;
  const float *xp = x + sl.off;
  const float n = float(C);
  float r[R * V], t[V];
  float sum = 0.f;
  if (whole) {
#pragma unroll
    for (int i = 0; i < R; i++) load_unit<CQ, VEC>(xp + i * sl.ustride, r + i * V);
#pragma unroll
    for (int i = 0; i < R * V; i++) sum += r[i];
  } else {
    for (int i = 0; i < sl.nu; i++) {
      load_unit<CQ, VEC>(xp + i * sl.ustride, t);
#pragma unroll
      for (int j = 0; j < V; j++) sum += t[j];
    }
  }
  const float mean = join_waves<4>(sum, lds[0]) / n;
  // centre once, then take the mean of the centred values out as well (see above)
  sum = 0.f;
  if (whole) {
#pragma unroll
    for (int i = 0; i < R * V; i++) {
      r[i] = r[i] - mean;
      sum += r[i];
    }
  } else {
    for (int i = 0; i < sl.nu; i++) {
      load_unit<CQ, VEC>(xp + i * sl.ustride, t);
#pragma unroll
      for (int j = 0; j < V; j++) sum += t[j] - mean;
    }
  }
  const float resid = join_waves<4>(sum, lds[1]) / n;
  sum = 0.f;
  if (whole) {
#pragma unroll
    for (int i = 0; i < R * V; i++) {
      r[i] = r[i] - resid;
      sum += r[i] * r[i];
    }
  } else {
    for (int i = 0; i < sl.nu; i++) {
      load_unit<CQ, VEC>(xp + i * sl.ustride, t);
#pragma unroll
      for (int j = 0; j < V; j++) {
        const float d = (t[j] - mean) - resid;
        sum += d * d;
      }
    }
  }
  const float den = sqrtf(join_waves<4>(sum, lds[2]) / n + eps);
  float *yp = y + sl.off;
  // the activation is resolved once (dispatch_act: the kinds the convolution epilogues take), so the slice stays in registers
  dispatch_act(act.kind, [&](auto kind_tag) {
    constexpr int KIND = decltype(kind_tag)::value;
    if (whole) {
#pragma unroll
      for (int i = 0; i < R; i++) {
        float o[V];
#pragma unroll
        for (int j = 0; j < V; j++) {
          const int c = (sl.u0 + i) * V + j;
          float v = r[i * V + j] / den * gb[0][c];
          if (beta) v = v + gb[1][c];
          o[j] = apply_act_c<KIND>(v, act.a, act.b);
        }
        if (sl.active) store_unit<CQ, VEC>(yp + i * sl.ustride, o);
      }
    } else {
      for (int i = 0; i < sl.nu; i++) {
        float o[V];
        load_unit<CQ, VEC>(xp + i * sl.ustride, o);
#pragma unroll
        for (int j = 0; j < V; j++) {
          const int c = (sl.u0 + i) * V + j;
          float v = ((o[j] - mean) - resid) / den * gb[0][c];
          if (beta) v = v + gb[1][c];
          o[j] = apply_act_c<KIND>(v, act.a, act.b);
        }
        if (sl.active) store_unit<CQ, VEC>(yp + i * sl.ustride, o);
      }
    }
  });
}

template <int WS, bool CQ, bool VEC>
__global__ __launch_bounds__(256) void channelnorm_reread_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                 float *__restrict__ y, int64_t P, int C, int S, int units, int per_wave, float eps,
                                                                 ActParam act) {
  constexpr int V = CQ ? 4 : 1;
  __shared__ float lds[WS == 1 ? 1 : 3][4][kTile];
  const Slice<WS, CQ> sl(P, C, S, units, per_wave);
  const float *xp = x + sl.off;
  const float n = float(C);
  float t[V];
  float sum = 0.f;
  for (int i = 0; i < sl.nu; i++) {
    load_unit<CQ, VEC>(xp + i * sl.ustride, t);
#pragma unroll
    for (int j = 0; j < V; j++) sum += t[j];
  }
  const float mean = join_waves<WS>(sum, lds[0]) / n;
  sum = 0.f;
  for (int i = 0; i < sl.nu; i++) {
    load_unit<CQ, VEC>(xp + i * sl.ustride, t);
#pragma unroll
    for (int j = 0; j < V; j++) sum += t[j] - mean;
  }
  const float resid = join_waves<WS>(sum, lds[WS == 1 ? 0 : 1]) / n;
  sum = 0.f;
  for (int i = 0; i < sl.nu; i++) {
    load_unit<CQ, VEC>(xp + i * sl.ustride, t);
#pragma unroll
    for (int j = 0; j < V; j++) {
      const float d = (t[j] - mean) - resid;
      sum += d * d;
    }
  }
  const float den = sqrtf(join_waves<WS>(sum, lds[WS == 1 ? 0 : 2]) / n + eps);
  float *yp = y + sl.off;
  dispatch_act(act.kind, [&](auto kind_tag) {
    constexpr int KIND = decltype(kind_tag)::value;
    for (int i = 0; i < sl.nu; i++) {
      float v[V];
      load_unit<CQ, VEC>(xp + i * sl.ustride, v);
#pragma unroll
      for (int j = 0; j < V; j++) {
        const int c = (sl.u0 + i) * V + j;
        float o = ((v[j] - mean) - resid) / den * gamma[c];
        if (beta) o = o + beta[c];
        v[j] = apply_act_c<KIND>(o, act.a, act.b);
      }
      if (sl.active) store_unit<CQ, VEC>(yp + i * sl.ustride, v);
    }
  });
}

struct Args {
  hipStream_t s;
  const float *x, *gamma, *beta;
  float *y;
  int64_t P;
  int C, S;
  ChannelNormSplit sp;
  float eps;
  ActParam act;
  bool vec;
};

template <int WS>
dim3 grid_of(const Args &a) {
  const int64_t per_block = WS == 1 ? 256 : kTile;
  return dim3(unsigned((a.P + per_block - 1) / per_block));
}

template <int R, int WS, bool CQ>
void launch_regs(const Args &a) {
  if constexpr (WS == 1) {
    if (CQ && a.vec)
      hipLaunchKernelGGL((channelnorm_regs_small_kernel<R, CQ, CQ>), grid_of<1>(a), dim3(256), 0, a.s, a.x, a.gamma, a.beta, a.y, a.P, a.C, a.S, a.sp.units, a.eps, a.act);
    else
      hipLaunchKernelGGL((channelnorm_regs_small_kernel<R, CQ, false>), grid_of<1>(a), dim3(256), 0, a.s, a.x, a.gamma, a.beta, a.y, a.P, a.C, a.S, a.sp.units, a.eps, a.act);
  } else {
    if (CQ && a.vec)
      hipLaunchKernelGGL((channelnorm_regs_kernel<R, CQ, CQ>), grid_of<4>(a), dim3(256), 0, a.s, a.x, a.gamma, a.beta, a.y, a.P, a.C, a.S, a.sp.units, a.eps, a.act);
    else
      hipLaunchKernelGGL((channelnorm_regs_kernel<R, CQ, false>), grid_of<4>(a), dim3(256), 0, a.s, a.x, a.gamma, a.beta, a.y, a.P, a.C, a.S, a.sp.units, a.eps, a.act);
  }
}

template <int WS, bool CQ>
void launch_reread(const Args &a) {
  if (CQ && a.vec)
    hipLaunchKernelGGL((channelnorm_reread_kernel<WS, CQ, CQ>), grid_of<WS>(a), dim3(256), 0, a.s, a.x, a.gamma, a.beta, a.y, a.P, a.C, a.S, a.sp.units, a.sp.per_wave, a.eps, a.act);
  else
    hipLaunchKernelGGL((channelnorm_reread_kernel<WS, CQ, false>), grid_of<WS>(a), dim3(256), 0, a.s, a.x, a.gamma, a.beta, a.y, a.P, a.C, a.S, a.sp.units, a.sp.per_wave, a.eps, a.act);
}

// the instantiated register sizes: host/channelnorm.cpp channelnorm_split names one of them
template <bool CQ>
bool launch_regs_by_size(const Args &a) {
#define INFERA_CN_CASE(WS, R) \
  if (a.sp.waves == WS && a.sp.regs == R) return launch_regs<R, WS, CQ>(a), true;
  if constexpr (CQ) {
    INFERA_CN_CASE(1, 1) INFERA_CN_CASE(1, 2) INFERA_CN_CASE(1, 4) INFERA_CN_CASE(1, 8)
    INFERA_CN_CASE(4, 4) INFERA_CN_CASE(4, 8) INFERA_CN_CASE(4, 16) INFERA_CN_CASE(4, 32)
  } else {
    INFERA_CN_CASE(1, 1) INFERA_CN_CASE(1, 2) INFERA_CN_CASE(1, 4) INFERA_CN_CASE(1, 8) INFERA_CN_CASE(1, 16) INFERA_CN_CASE(1, 32)
    INFERA_CN_CASE(4, 16) INFERA_CN_CASE(4, 32) INFERA_CN_CASE(4, 64) INFERA_CN_CASE(4, 128)
  }
#undef INFERA_CN_CASE
  return false;
}

}  // namespace

bool channelnorm(hipStream_t s, const float *x, const float *gamma, const float *beta, float *y, int64_t rows, int C, int S, bool cq, bool regs, float eps,
                 ActParam act) {
  if (rows <= 0) return true;
  if (C < 1 || C > kChannelNormMaxC || S < 1 || S > kChannelNormMaxS) return false;
  const int64_t P = rows * S;
  if (P > (int64_t(1) << 36)) return false;  // (the grid: P / 64 workgroups)
  // (an [N,C,1,1] tensor is the same floats in either layout: whole quads are then read as quads)
  const bool quads = C % 4 == 0 && (cq || S == 1);
  Args a{s, x, gamma, beta, y, P, C, S, channelnorm_split(C, quads), eps, act,
         ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0};
  if (regs) {
    if (a.sp.regs <= 0) return false;
    return quads ? launch_regs_by_size<true>(a) : launch_regs_by_size<false>(a);
  }
  if (a.sp.waves == 1) quads ? launch_reread<1, true>(a) : launch_reread<1, false>(a);
  else quads ? launch_reread<4, true>(a) : launch_reread<4, false>(a);
  return true;
}

}  // namespace infera_hip::kern
