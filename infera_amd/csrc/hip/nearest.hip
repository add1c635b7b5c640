// nearest.hip -- squared Euclidean distances of each row to a constant reference set, with the selection fused (KMeans / nearest
// centroid labels, k-NN search) on gfx950 (semantics: INTEGRATION.md section 2.6; tables: host/nearest.hpp).
//
// nearest_kernel: the structure of svm.hip stage 1.  A wave owns 32 rows, a workgroup 1, 2 or 4 waves (as many as keep the row tiles
// within 64 KB of LDS; one wave and up to 129 KB for F > 504).  The rows are staged in LDS once (row stride F_pad + 4 floats:
// conflict-free ds_read_b128), centred on the load-time mean of the reference set, and their squared norms summed in a fixed order.
// Block b works on row tile b / S and reference slice b % S; a slice is a run of 32-vector tiles fixed at load from the model alone.
// Per tile:
//   dot[c, row] = (C - mu) . (X - mu)^T on v_mfma_f32_32x32x2_f32 (exact f32: a k-ordered fma chain), A = the reference tile straight
//            from L2 in fragment order (one 16-B load per lane feeds four k-steps), B = X from LDS; k order inside each group of 8
//            features is 0,4,1,5,2,6,3,7 (the dense.hip permutation): the set is packed in the same order.
//   epilogue on the VALU, in registers, while the other waves of the SIMD issue MFMAs: lane (r, h) holds row r and vectors
//            32 t + 8 (i >> 2) + 4 h + (i & 3), i = 0..15, ascending in i.  d2 = max(|x|^2 + |c|^2 - 2 dot, 0) (a NaN row stays NaN) is
//            stored with plain vector stores (the [rows, M] outputs; the distances of a selection are never written), or inserted into
//            the lane's running best-K list: K (value, index) pairs in VGPRs (K = 1 or 16: 32 registers at K = 16, beside the 16
//            accumulators), one comparison per candidate once the list has filled with near vectors.
// At the end of the slice the list of the other lane half is merged in (fixed order) and half 0 writes part[row][slice][K].
// nearest_reduce_kernel (one lane per row) merges the slices in slice order and writes the label, the indices or the values.  The order
// is total -- smaller distance, NaN after every number, equal distances by lower index -- so the result does not depend on the tiling or
// the slicing.  No float atomics: a row's bits depend only on the model and the row, never on the row count, the chunking or the call path.
//
// Bound designed for: 2 F_pad M MFMA flop per row at 157.3 TFLOP/s, plus the [rows, M] write at the HBM rate when it is served; the
// epilogue (about 5 VALU instructions per candidate, 16 per lane per tile) hides behind the 64-cycle MFMAs only while F_pad >= ~32.
// What binds first is the cache, not the matrix cores: every wave streams its slice of the set itself (the waves of a workgroup do not
// share A through LDS), a 1 KB fragment load feeds four MFMAs of 4096 flop -- 16 flop per byte, so the MFMA peak would need ~10 TB/s from
// L2.  The measured fractions of the MFMA bound are in DESIGN.md section 3.13.
#include "select.hpp"

#include "../host/nearest.hpp"

#include <cmath>

namespace infera_hip::kern {

namespace {

constexpr int kMaxWaves = 4;
constexpr int kLdsBudget = 64 * 1024;

// K > 0: the selection (part); K == 0: the matrix (out [rows, M], rooted: sqrt(d2))
template <int K>
__global__ __launch_bounds__(kMaxWaves * 64) void nearest_kernel(const float *__restrict__ x, int F, int F_pad, const float *__restrict__ center,
                                                                const f32x4 *__restrict__ ref, const float *__restrict__ ref_norm,
                                                                const uint32_t *__restrict__ slice_tile, float *__restrict__ out, int64_t nr, int S,
                                                                int M, bool rooted) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int nw = int(blockDim.x >> 6), wave = int(threadIdx.x >> 6), lane = int(threadIdx.x & 63), r = lane & 31, h = lane >> 5;
  const int s = int(blockIdx.x % unsigned(S));
  const int64_t row0 = int64_t(blockIdx.x / unsigned(S)) * (32 * nw) + 32 * wave;
  const int stride = F_pad + 4;
  float *tile = lds + wave * 32 * stride;
  for (int e = lane; e < 32 * F_pad; e += 64) {
    const int rr = e / F_pad, k = e - rr * F_pad;
    const int64_t g = row0 + rr;
    float v = 0.f;
    if (k < F && g < nr) v = x[g * F + k] - center[k];
    tile[rr * stride + k] = v;
  }
  __syncthreads();
  float xn;
  {  // |x - center|^2: each lane half sums half of the features, halves added in order
    const int half = F_pad / 2;
    float a = 0.f;
    for (int k = h * half; k < (h + 1) * half; k++) a = fmaf(tile[r * stride + k], tile[r * stride + k], a);
    const float o = __shfl_xor(a, 32);
    xn = h ? o + a : a + o;
  }
  const int64_t row = row0 + r;
  BestList<K ? K : 1> best;
  best.clear();

  const int G = F_pad / 8;
  const float *xr = tile + r * stride + 4 * h;
  const uint32_t t_end = slice_tile[s + 1];
  for (uint32_t t = slice_tile[s]; t < t_end; t++) {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.f;
    const f32x4 *rt = ref + int64_t(t) * G * 64 + lane;
    for (int g = 0; g < G; g++) {
      const f32x4 a4 = rt[g * 64];
      const f32x4 b4 = *reinterpret_cast<const f32x4 *>(xr + 8 * g);
#pragma unroll
      for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j], b4[j], acc, 0, 0, 0);
    }
    // acc[i] = (x_r - mu) . (c - mu) for vector 32 t + 8 (i >> 2) + 4 h + (i & 3)
    f32x4 cn[4];
#pragma unroll
    for (int q = 0; q < 4; q++) cn[q] = *reinterpret_cast<const f32x4 *>(ref_norm + int64_t(t) * 32 + 8 * q + 4 * h);
#pragma unroll
    for (int i = 0; i < 16; i++) {
      float d2 = xn + cn[i >> 2][i & 3] - 2.f * acc[i];
      d2 = d2 < 0.f ? 0.f : d2;  // (cancellation; NaN stays NaN)
      const int idx = int(t) * 32 + 8 * (i >> 2) + 4 * h + (i & 3);
      if constexpr (K > 0) {
        if (idx < M) best.insert(d2, idx);
      } else {
        if (idx < M && row < nr) out[row * M + idx] = rooted ? sqrtf(d2) : d2;
      }
    }
  }
  if constexpr (K > 0) {
    // the other half's list (copied first: inserting shifts entries), merged entry by entry; half 0 stores the result
    float ov[K];
    int oi[K];
#pragma unroll
    for (int j = 0; j < K; j++) ov[j] = __shfl_xor(best.v[j], 32), oi[j] = __shfl_xor(best.i[j], 32);
#pragma unroll
    for (int j = 0; j < K; j++) best.insert(ov[j], oi[j]);
    if (h == 0 && row < nr) {
      float *p = out + (row * S + s) * (2 * K);
#pragma unroll
      for (int j = 0; j < K; j++) p[j] = best.v[j], p[K + j] = __int_as_float(best.i[j]);
    }
  }
}

// part: [rows][S][2 K] (K values, K index patterns); mode: host/nearest.hpp NearestOut; k <= K results per row
template <int K>
__global__ __launch_bounds__(64) void nearest_reduce_kernel(const float *__restrict__ part, float *__restrict__ y, int64_t nr, int S, int k, int mode) {
  const int64_t stride = int64_t(gridDim.x) * 64;
  for (int64_t row = int64_t(blockIdx.x) * 64 + threadIdx.x; row < nr; row += stride) {
    BestList<K> best;
    best.clear();
    for (int s = 0; s < S; s++) {
      const float *p = part + (row * S + s) * (2 * K);
#pragma unroll
      for (int j = 0; j < K; j++) best.insert(p[j], __float_as_int(p[K + j]));
    }
    if (mode == kNearestLabel) {
      y[row] = float(best.i[0]);
      continue;
    }
#pragma unroll
    for (int j = 0; j < K; j++)
      if (j < k) y[row * k + j] = mode == kNearestIndices ? float(best.i[j]) : mode == kNearestValuesSqrt ? sqrtf(best.v[j]) : best.v[j];
  }
}

// The k-NN vote (INTEGRATION.md section 2.6 "The k-NN vote"): the merge of nearest_reduce_kernel, then the neighbours' classes / targets
// from the constant tables (plain 4-byte gathers, the tables stay in L2), the weights and the tally.  One lane per row; a block is ONE
// wave, which walks 64-row tiles with a stride.  Every sum runs over ascending neighbour j from 0.f and nothing is contracted into an
// FMA, so an f32 restatement reproduces the bits.  The tally keeps no per-class array: tot[j] = the total of neighbour j's class is k
// compare-adds over the list in VGPRs (K^2 after unrolling), the class-0 total starts the first-maximum scan (as the ArgMax step's scan
// starts at element 0: a NaN there stays) and a later class wins where its total compares greater, ties to the lower class.
// Probabilities: the wave zeroes a [64, C] tile in LDS (64 C 4 B <= 64 KB: C <= 256, host/nearest.hpp), every lane drops its <= k
// totals into its row, and the tile -- which is one contiguous run of the [rows, C] output -- leaves linearly, a 16-byte piece per lane
// (scalar where the run is not 16-byte aligned or ends), each element divided by its row's weight sum fetched from the owning lane.
// Bound designed for: the bytes of the lists read (8 K S per row) plus the output written (4, or 4 C), at the HBM rate.  Known cost
// outside that bound: a lane reads its own row's lists (row-strided 4-byte loads, as nearest_reduce_kernel), and the <= k scattered
// LDS writes of a row conflict when C is even (row stride C floats).  Measured: DESIGN.md section 3.13.
constexpr unsigned kVoteGridCap = 4096;

template <int K>
__global__ __launch_bounds__(64) void nearest_vote_kernel(const float *__restrict__ part, const int *__restrict__ cls, const float *__restrict__ target,
                                                         const float *__restrict__ class_value, float *__restrict__ y, int64_t nr, int S, int M, int k, int C,
                                                         int mode, bool weighted, bool rooted, float eps) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = int(threadIdx.x);
  for (int64_t base = int64_t(blockIdx.x) * 64; base < nr; base += int64_t(gridDim.x) * 64) {
    const int64_t row = base + lane;
    const bool live = row < nr;
    BestList<K> best;
    best.clear();
    if (live)
      for (int s = 0; s < S; s++) {
        const float *p = part + (row * S + s) * (2 * K);
#pragma unroll
        for (int j = 0; j < K; j++) best.insert(p[j], __float_as_int(p[K + j]));
      }
    // k <= M of the entries are reference vectors; the guard keeps a gather inside its table whatever the lists hold
    int at[K];
    float w[K], sum = 0.f;
#pragma unroll
    for (int j = 0; j < K; j++) {
      at[j] = unsigned(best.i[j]) < unsigned(M) ? best.i[j] : 0;
      const float d = rooted ? sqrtf(best.v[j]) : best.v[j];
      w[j] = !weighted ? 1.f : d != d ? d : 1.f / fmaxf(d, eps);  // (a NaN distance is a NaN weight: ONNX Max keeps the NaN, fmaxf would drop it)
      if (j < k) sum += w[j];
    }
    if (mode == kVoteValue) {
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < K; j++)
        if (j < k) {
          const float t = live ? target[at[j]] : 0.f;
          a += weighted ? w[j] * t : t;
        }
      if (live) y[row] = a / (weighted ? sum : float(k));
      continue;
    }
    int c[K];
#pragma unroll
    for (int j = 0; j < K; j++) c[j] = live && j < k ? cls[at[j]] : -1;
    float tot[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < K; i++)
        if (i < k && c[i] == c[j]) a += w[i];
      tot[j] = a;
    }
    if (mode == kVoteLabel) {
      float bv = 0.f;  // the total of class 0 (0.f when no neighbour carries it)
#pragma unroll
      for (int j = 0; j < K; j++)
        if (j < k && c[j] == 0) bv = tot[j];
      int bc = 0;
#pragma unroll
      for (int j = 0; j < K; j++)
        if (j < k && (tot[j] > bv || (tot[j] == bv && c[j] < bc))) bv = tot[j], bc = c[j];
      if (live) y[row] = class_value[bc];
      continue;
    }
    // kVoteProba: rows base .. base + n - 1 are one run of n C floats of the output
    const int n = int(nr - base < 64 ? nr - base : 64), total = n * C;
    for (int e = 4 * lane; e < total; e += 256) *reinterpret_cast<f32x4 *>(lds + e) = f32x4{0.f, 0.f, 0.f, 0.f};  // (64 C is a multiple of 4: e + 3 stays inside)
    __syncthreads();
    if (live) {
#pragma unroll
      for (int j = 0; j < K; j++)
        if (j < k) lds[lane * C + c[j]] = tot[j];  // (neighbours of one class write the same total)
    }
    __syncthreads();
    float *out = y + base * C;
    const bool wide = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int e0 = 0; e0 < total; e0 += 256) {  // (the same trip count in every lane: each takes part in the shuffles)
      const int e = e0 + 4 * lane;
      f32x4 v = e < total ? *reinterpret_cast<const f32x4 *>(lds + e) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int r = (e + q) / C;
        v[q] = v[q] / __shfl(sum, r < 63 ? r : 63);
      }
      if (wide && e + 3 < total) {
        *reinterpret_cast<f32x4 *>(out + e) = v;
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++)
          if (e + q < total) out[e + q] = v[q];
      }
    }
    __syncthreads();  // (the next tile zeroes what this one still reads)
  }
}

template <int K>
bool launch(hipStream_t s, const float *x, int F, int F_pad, const float *center, const float *ref, const float *ref_norm, const uint32_t *slice_tile,
            float *out, int64_t rows, int S, int M, bool rooted) {
  int nw = kMaxWaves;
  while (nw > 1 && size_t(nw) * 32 * size_t(F_pad + 4) * 4 > size_t(kLdsBudget)) nw /= 2;
  const size_t lds = size_t(nw) * 32 * size_t(F_pad + 4) * 4;
  auto kernel = nearest_kernel<K>;
  if (lds > size_t(kLdsBudget) &&  // F > 504: one wave, dynamic LDS beyond 64 KB is opt-in
      hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
    return false;
  const int64_t tiles = (rows + 32 * nw - 1) / (32 * nw);
  hipLaunchKernelGGL(kernel, dim3(unsigned(tiles * S)), dim3(unsigned(64 * nw)), lds, s, x, F, F_pad, center, reinterpret_cast<const f32x4 *>(ref), ref_norm,
                     slice_tile, out, rows, S, M, rooted);
  return true;
}

}  // namespace

bool nearest(hipStream_t s, const float *x, int F, int F_pad, const float *center, const float *ref, const float *ref_norm, const uint32_t *slice_tile,
             float *out, int64_t rows, int S, int M, int k, int mode) {
  if (rows <= 0) return true;
  if (mode != kNearestSelect) return launch<0>(s, x, F, F_pad, center, ref, ref_norm, slice_tile, out, rows, S, M, mode == kNearestMatrixSqrt);
  switch (nearest_list_width(k)) {
    case 1: return launch<1>(s, x, F, F_pad, center, ref, ref_norm, slice_tile, out, rows, S, M, false);
    default: return launch<16>(s, x, F, F_pad, center, ref, ref_norm, slice_tile, out, rows, S, M, false);
  }
}

void nearest_reduce(hipStream_t s, const float *part, float *y, int64_t rows, int S, int k, int mode) {
  if (rows <= 0) return;
  const unsigned g = unsigned(std::min<int64_t>(4096, (rows + 63) / 64));
  switch (nearest_list_width(k)) {
    case 1: hipLaunchKernelGGL(nearest_reduce_kernel<1>, dim3(g), dim3(64), 0, s, part, y, rows, S, k, mode); break;
    default: hipLaunchKernelGGL(nearest_reduce_kernel<16>, dim3(g), dim3(64), 0, s, part, y, rows, S, k, mode); break;
  }
}

bool nearest_vote(hipStream_t s, const float *part, const int *cls, const float *target, const float *class_value, float *y, int64_t rows, int S, int M, int k,
                  int C, int mode, bool weighted, bool rooted, float eps) {
  if (rows <= 0) return true;
  const size_t lds = mode == kVoteProba ? size_t(64) * size_t(C) * 4 : 0;
  if (lds > size_t(kLdsBudget) || k < 1 || k > M || k > int(kNearestMaxK)) return false;
  const unsigned g = unsigned(std::min<int64_t>(kVoteGridCap, (rows + 63) / 64));
  switch (nearest_list_width(k)) {
    case 1: hipLaunchKernelGGL(nearest_vote_kernel<1>, dim3(g), dim3(64), lds, s, part, cls, target, class_value, y, rows, S, M, k, C, mode, weighted, rooted, eps); break;
    default: hipLaunchKernelGGL(nearest_vote_kernel<16>, dim3(g), dim3(64), lds, s, part, cls, target, class_value, y, rows, S, M, k, C, mode, weighted, rooted, eps); break;
  }
  return true;
}

}  // namespace infera_hip::kern
