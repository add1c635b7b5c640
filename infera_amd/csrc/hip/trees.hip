// trees.hip -- ai.onnx.ml tree ensembles (TreeEnsembleRegressor / TreeEnsembleClassifier) on gfx950.
//
// tree_walk_kernel: one lane per table row, one wave (64 rows) per block.  The row tile is read with coalesced loads (16 B per
// lane when aligned) and staged in LDS with a row stride of F + 1 floats, so the per-node feature reads are conflict-free LDS
// reads; tables wider than kStageMaxF read the features from global memory (L1 / L2) instead.  Node records (8 B, host/trees.hpp)
// come from global memory: a few MB of ensemble stays in L2 / MALL.  Each level of a walk is a dependent load, so every lane walks
// kInFlight trees at once.  The trees are cut into `S` slices fixed at load time from the ensemble alone; block b works on row
// tile b / S and slice b % S (the slices of one tile run side by side and share its input lines in L2) and writes its slice's
// partial sums.  tree_reduce_kernel adds the slices in slice order -- no float atomics, so a row's bits depend only on the model
// and the row.  Sums are kept in f64 (a 1000-tree sum that cancels to near zero keeps the project's 1e-4 relative bar; the f32 leaf
// values are exact in it) and a partial is stored as an f32 pair (hi, lo = the rest), so the scratch needs no 8-byte alignment.
// Accumulators: per-lane registers for walk widths up to 16 (compile-time buckets), the lane's own partial row in global memory
// beyond that.
#include "device_common.hpp"

#include "../host/plan.hpp"
#include "../host/trees.hpp"

namespace infera_hip::kern {

namespace {

constexpr int kRows = 64;        // rows per block: one wave, one lane per row
constexpr int kInFlight = 4;     // trees each lane walks at once
constexpr int kStageMaxF = 128;  // widest row tile staged in LDS (64 x 129 floats = 33 KB)
constexpr uint32_t kFeatureMask = uint32_t(kTreeMaxFeature - 1);

__device__ __forceinline__ void store_pair(float *p, double v) {
  const float hi = float(v);
  p[0] = hi;
  p[1] = float(v - double(hi));
}
__device__ __forceinline__ double load_pair(const float *p) { return double(p[0]) + double(p[1]); }

// EB: accumulators per lane (0: accumulate in the partial buffer); W: walk width (1: leaf values inline in the records)
template <int EB, bool STAGED>
__global__ __launch_bounds__(kRows) void tree_walk_kernel(const float *__restrict__ x, const uint2 *__restrict__ nodes,
                                                          const uint32_t *__restrict__ roots, const uint32_t *__restrict__ slice_first,
                                                          const float *__restrict__ leaves, float *__restrict__ part, int64_t nr, int F,
                                                          int W, int S, bool aligned) {
  extern __shared__ float tile[];
  const int s = int(blockIdx.x % unsigned(S));
  const int64_t r0 = int64_t(blockIdx.x / unsigned(S)) * kRows;
  const int lane = int(threadIdx.x);
  const int nrow = int(min(int64_t(kRows), nr - r0));
  const bool live = lane < nrow;
  const int lr = live ? lane : nrow - 1;  // lanes past the last row walk that row and store nothing
  const float *xr;
  if constexpr (STAGED) {
    const float *src = x + r0 * F;
    const int total = nrow * F, stride = F + 1;
    int done = 0;
    if (aligned) {
      const f32x4 *src4 = reinterpret_cast<const f32x4 *>(src);
      for (int v = lane; v < (total >> 2); v += kRows) {
        const f32x4 q = src4[v];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int e = 4 * v + k, r = e / F;
          tile[r * stride + (e - r * F)] = q[k];
        }
      }
      done = total & ~3;
    }
    for (int e = done + lane; e < total; e += kRows) {
      const int r = e / F;
      tile[r * stride + (e - r * F)] = src[e];
    }
    __syncthreads();
    xr = tile + lr * stride;
  } else {
    xr = x + (r0 + lr) * int64_t(F);
  }
  double acc[EB > 0 ? EB : 1];
#pragma unroll
  for (int j = 0; j < (EB > 0 ? EB : 1); j++) acc[j] = 0.0;
  float *prow = part + (int64_t(s) * nr + r0 + lr) * W * 2;  // W (hi, lo) pairs
  if constexpr (EB == 0) {
    if (live)
      for (int j = 0; j < 2 * W; j++) prow[j] = 0.f;
  }
  const uint32_t t_begin = slice_first[s], t_end = slice_first[s + 1];
  for (uint32_t t0 = t_begin; t0 < t_end; t0 += kInFlight) {
    uint32_t cur[kInFlight];
    uint2 nd[kInFlight];
#pragma unroll
    for (int k = 0; k < kInFlight; k++) cur[k] = roots[min(t0 + uint32_t(k), t_end - 1)];
    for (;;) {
#pragma unroll
      for (int k = 0; k < kInFlight; k++) nd[k] = nodes[cur[k]];
      bool more = false;
#pragma unroll
      for (int k = 0; k < kInFlight; k++) {
        const uint32_t m = nd[k].y, kind = m >> 30;
        if (kind == kTreeLeaf) continue;
        more = true;
        const float v = xr[(m >> kTreeFeatureShift) & kFeatureMask], t = __uint_as_float(nd[k].x);
        const bool holds = kind == 0 ? v <= t : kind == 1 ? v < t : v == t;
        const bool right = v != v ? (m & kTreeNanRight) != 0 : !holds;
        cur[k] += (m & kTreeDeltaMask) + (right ? 1u : 0u);
      }
      if (!more) break;
    }
#pragma unroll
    for (int k = 0; k < kInFlight; k++) {
      if (t0 + uint32_t(k) >= t_end) break;
      if constexpr (EB == 1) {
        acc[0] += double(__uint_as_float(nd[k].x));
      } else {
        const float *l = leaves + int64_t(nd[k].y & kTreeLeafRowMask) * W;
        if constexpr (EB == 0) {
          if (live)
            for (int j = 0; j < W; j++) store_pair(prow + 2 * j, load_pair(prow + 2 * j) + double(l[j]));
        } else {
#pragma unroll
          for (int j = 0; j < EB; j++)
            if (j < W) acc[j] += double(l[j]);
        }
      }
    }
  }
  if constexpr (EB > 0) {
    if (live)
#pragma unroll
      for (int j = 0; j < EB; j++)
        if (j < W) store_pair(prow + 2 * j, acc[j]);
  }
}

constexpr int kReduceBlock = 256;

// part: [S][nr][W] (hi, lo) pairs.  mode: host/plan.hpp TreeOut.  Sums in f64, rounded to f32 once.
__global__ __launch_bounds__(kReduceBlock) void tree_reduce_kernel(const float *__restrict__ part, const float *__restrict__ base,
                                                                   const float *__restrict__ labels, float *__restrict__ y, int64_t nr, int W,
                                                                   int S, double ntrees, bool average, int mode, bool is_signed) {
  const int64_t stride = int64_t(gridDim.x) * kReduceBlock, plane = nr * W;
  const int64_t n = mode == kTreeScores ? plane : nr;
  auto total = [&](int64_t e, int j) {  // element e = row * W + j of the [nr][W] plane
    double v = 0.0;
    for (int s = 0; s < S; s++) v += load_pair(part + 2 * (s * plane + e));
    if (average) v = v / ntrees;
    if (base) v += double(base[j]);
    return v;
  };
  for (int64_t i = int64_t(blockIdx.x) * kReduceBlock + threadIdx.x; i < n; i += stride) {
    if (mode == kTreeScores) {
      y[i] = float(total(i, int(i % W)));
      continue;
    }
    if (mode == kTreeLabel) {
      int best = 0;
      double bv = 0.0;
      for (int j = 0; j < W; j++) {
        const double v = total(i * W + j, j);
        if (j == 0 || v > bv) best = j, bv = v;  // the first maximum
      }
      y[i] = labels[best];
      continue;
    }
    const double v = total(i, 0);  // binary single-column form: W == 1
    if (mode == kTreeBinaryScores) {
      y[2 * i] = float(is_signed ? -v : 1.0 - v);
      y[2 * i + 1] = float(v);
    } else {
      y[i] = labels[(is_signed ? v > 0.0 : v > 0.5) ? 1 : 0];
    }
  }
}

template <int EB>
void walk_launch(hipStream_t s, const float *x, int F, const uint32_t *tab, int64_t n_nodes, int64_t n_trees, const float *leaves, int W, int S,
                 float *part, int64_t rows) {
  const uint2 *nodes = reinterpret_cast<const uint2 *>(tab);
  const uint32_t *roots = tab + 2 * n_nodes, *slices = roots + n_trees;
  const dim3 grid(unsigned((rows + kRows - 1) / kRows * S));
  const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  if (F <= kStageMaxF)
    hipLaunchKernelGGL((tree_walk_kernel<EB, true>), grid, dim3(kRows), size_t(kRows) * size_t(F + 1) * 4, s, x, nodes, roots, slices, leaves,
                       part, rows, F, W, S, aligned);
  else
    hipLaunchKernelGGL((tree_walk_kernel<EB, false>), grid, dim3(kRows), 0, s, x, nodes, roots, slices, leaves, part, rows, F, W, S, aligned);
}

}  // namespace

void tree_walk(hipStream_t s, const float *x, int F, const uint32_t *tab, int64_t n_nodes, int64_t n_trees, const float *leaves, int W, int S,
               float *part, int64_t rows) {
  if (rows <= 0) return;
  if (W == 1) walk_launch<1>(s, x, F, tab, n_nodes, n_trees, leaves, W, S, part, rows);
  else if (W <= 4) walk_launch<4>(s, x, F, tab, n_nodes, n_trees, leaves, W, S, part, rows);
  else if (W <= 8) walk_launch<8>(s, x, F, tab, n_nodes, n_trees, leaves, W, S, part, rows);
  else if (W <= 16) walk_launch<16>(s, x, F, tab, n_nodes, n_trees, leaves, W, S, part, rows);
  else walk_launch<0>(s, x, F, tab, n_nodes, n_trees, leaves, W, S, part, rows);
}

void tree_reduce(hipStream_t s, const float *part, const float *base, const float *labels, float *y, int64_t rows, int W, int S, int64_t n_trees,
                 bool average, int mode, bool is_signed) {
  if (rows <= 0) return;
  const int64_t n = mode == kTreeScores ? rows * W : rows;
  const int64_t g = std::min<int64_t>(2048, (n + kReduceBlock - 1) / kReduceBlock);
  hipLaunchKernelGGL(tree_reduce_kernel, dim3(unsigned(g)), dim3(kReduceBlock), 0, s, part, base, labels, y, rows, W, S, double(n_trees), average,
                     mode, is_signed);
}

}  // namespace infera_hip::kern
