// reduce.hip -- HBM-bound reductions along the feature axis: the ONNX Reduce* family over the last axis (RowReduce), ArgMin, TopK and
// the elementwise operators with a per-vector scalar operand ([N, K] (op) [N, 1]).
//
// row_reduce_kernel: a group of W lanes (W = the power of two >= min(E, 64)) owns one vector of E elements, so short vectors share a wave
// and consecutive lanes read consecutive floats.  Each lane folds its elements k = sub, sub + W, ... in ascending order in f32, then a
// butterfly over the W lanes (xor W/2, ..., 1; the lower lane's value is the left operand) joins the partial results.  The order is fixed
// by E alone -- deterministic, but not numpy's pairwise order.  Max / Min propagate NaN (a NaN poisons its own vector only);
// LogSumExp shifts by the vector's maximum.
#include "select.hpp"

#include "../host/plan.hpp"

#include <cmath>

namespace infera_hip::kern {

namespace {

constexpr int kBlock = 256;
inline int grid_for(int64_t work_items) {
  int64_t g = (work_items + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;
  return int(g);
}

__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : b != b ? b : (a > b ? a : b); }
__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : b != b ? b : (a < b ? a : b); }

// how two partial results of reduction OP combine, and what one element contributes
template <int OP>
__device__ __forceinline__ float red_join(float a, float b) {
  if constexpr (OP == kReduceMax) return nan_max(a, b);
  else if constexpr (OP == kReduceMin) return nan_min(a, b);
  else if constexpr (OP == kReduceProd) return a * b;
  else return a + b;
}
template <int OP>
__device__ __forceinline__ float red_elem(float v, float shift) {
  if constexpr (OP == kReduceL1) return fabsf(v);
  else if constexpr (OP == kReduceL2 || OP == kReduceSumSquare) return v * v;
  else if constexpr (OP == kReduceLogSumExp) return expf(v - shift);
  else return v;
}
template <int OP>
__device__ __forceinline__ float red_identity() {
  if constexpr (OP == kReduceMax) return -INFINITY;
  else if constexpr (OP == kReduceMin) return INFINITY;
  else if constexpr (OP == kReduceProd) return 1.f;
  else return 0.f;
}

template <int OP>
__device__ __forceinline__ float group_reduce(const float *src, int E, int W, int sub, float shift) {
  float a = red_identity<OP>();
  for (int k = sub; k < E; k += W) a = red_join<OP>(a, red_elem<OP>(src[k], shift));
  for (int o = W >> 1; o > 0; o >>= 1) {
    const float b = __shfl_xor(a, o);
    a = (sub & o) ? red_join<OP>(b, a) : red_join<OP>(a, b);
  }
  return a;
}

template <int OP>
__global__ __launch_bounds__(kBlock) void row_reduce_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t nvec, int E, int W) {
  const int lane = threadIdx.x & 63, sub = lane & (W - 1), slot = lane / W, vpw = 64 / W;
  const int64_t wave = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6, nwaves = (int64_t(gridDim.x) * kBlock) >> 6;
  for (int64_t v0 = wave * vpw; v0 < nvec; v0 += nwaves * vpw) {
    const int64_t v = v0 + slot;
    const float *src = x + (v < nvec ? v : nvec - 1) * E;
    float shift = 0.f;
    if constexpr (OP == kReduceLogSumExp) {
      const float mx = group_reduce<kReduceMax>(src, E, W, sub, 0.f);
      shift = (mx - mx == 0.f) ? mx : 0.f;  // (an infinite maximum is not subtracted: exp(inf - inf))
    }
    float a = group_reduce<OP>(src, E, W, sub, shift);
    if constexpr (OP == kReduceMean) a = a / float(E);
    if constexpr (OP == kReduceL2) a = sqrtf(a);
    if constexpr (OP == kReduceLogSum) a = logf(a);
    if constexpr (OP == kReduceLogSumExp) a = logf(a) + shift;
    if (v < nvec && sub == 0) y[v] = a;
  }
}

// Index of the first minimum of each row, as an f32 value (the twin of eltwise.hip's ArgMax: element 0 starts the scan, NaN never wins)
__global__ __launch_bounds__(kBlock) void argmin_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t rows, int64_t len) {
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < rows; r += stride) {
    const float *src = x + r * len;
    float best = src[0];
    int64_t bi = 0;
    for (int64_t j = 1; j < len; j++)
      if (src[j] < best) {
        best = src[j];
        bi = j;
      }
    y[r] = float(bi);
  }
}

// The k best of each row of x [rows, M], one lane per row, through the running list of select.hpp.  largest: the values are negated on
// the way in and out (exact), so NaN ranks last and equal values resolve to the lower index in both directions.
template <int K>
__global__ __launch_bounds__(64) void topk_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t rows, int M, int k, bool largest,
                                                  bool indices) {
  const int64_t stride = int64_t(gridDim.x) * 64;
  for (int64_t r = int64_t(blockIdx.x) * 64 + threadIdx.x; r < rows; r += stride) {
    const float *src = x + r * M;
    BestList<K> best;
    best.clear();
    for (int j = 0; j < M; j++) best.insert(largest ? -src[j] : src[j], j);
#pragma unroll
    for (int j = 0; j < K; j++)
      if (j < k) y[r * k + j] = indices ? float(best.i[j]) : largest ? -best.v[j] : best.v[j];
  }
}

// y[v, i] = act(a[v, i] (op) b[v])   (scalar_left: b[v] (op) a[v, i]) over nvec vectors of E elements
__global__ __launch_bounds__(kBlock) void binary_rowscalar_kernel(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ y, int64_t n,
                                                                 int64_t E, char op, bool scalar_left, ActParam act) {
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) y[i] = apply_act(apply_bop(a[i], b[i / E], op, scalar_left), act);
}

}  // namespace

void row_reduce(hipStream_t s, const float *x, float *y, int64_t nvec, int E, int op) {
  if (nvec <= 0 || E <= 0) return;
  int W = 1;
  while (W < E && W < 64) W <<= 1;
  const dim3 grid(grid_for((nvec + 64 / W - 1) / (64 / W) * 64));
#define INFERA_REDUCE_OP(OP) \
  case OP: hipLaunchKernelGGL(row_reduce_kernel<OP>, grid, dim3(kBlock), 0, s, x, y, nvec, E, W); break;
  switch (op) {
    INFERA_REDUCE_OP(kReduceSum) INFERA_REDUCE_OP(kReduceMean) INFERA_REDUCE_OP(kReduceMax) INFERA_REDUCE_OP(kReduceMin) INFERA_REDUCE_OP(kReduceProd)
    INFERA_REDUCE_OP(kReduceL1) INFERA_REDUCE_OP(kReduceL2) INFERA_REDUCE_OP(kReduceSumSquare) INFERA_REDUCE_OP(kReduceLogSum)
    INFERA_REDUCE_OP(kReduceLogSumExp)
  }
#undef INFERA_REDUCE_OP
}

void argmin_rows(hipStream_t s, const float *x, float *y, int64_t rows, int64_t len) {
  if (rows <= 0 || len <= 0) return;
  hipLaunchKernelGGL(argmin_kernel, dim3(grid_for(rows)), dim3(kBlock), 0, s, x, y, rows, len);
}

void topk_rows(hipStream_t s, const float *x, float *y, int64_t rows, int M, int k, bool largest, bool indices) {
  if (rows <= 0 || M <= 0) return;
  const unsigned g = unsigned(std::min<int64_t>(4096, (rows + 63) / 64));
  if (k <= 1) hipLaunchKernelGGL(topk_kernel<1>, dim3(g), dim3(64), 0, s, x, y, rows, M, k, largest, indices);
  else hipLaunchKernelGGL(topk_kernel<16>, dim3(g), dim3(64), 0, s, x, y, rows, M, k, largest, indices);
}

void binary_rowscalar(hipStream_t s, const float *a, const float *b, float *y, int64_t nvec, int64_t E, char op, bool scalar_left, ActParam act) {
  if (nvec <= 0 || E <= 0) return;
  hipLaunchKernelGGL(binary_rowscalar_kernel, dim3(grid_for(nvec * E)), dim3(kBlock), 0, s, a, b, y, nvec * E, E, op, scalar_left, act);
}

}  // namespace infera_hip::kern
