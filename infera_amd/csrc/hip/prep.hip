// prep.hip -- ai.onnx.ml preprocessing regions (Imputer, Scaler, Binarizer, OneHotEncoder, LabelEncoder, FeatureVectorizer,
// ArrayFeatureExtractor, integer inputs) as one column program per output column (host/prep.hpp).
//
// prep_kernel is memory-bound: a row tile of the input is one contiguous range of R * F_in floats and the output tile one of R * F
// floats.  A block stages its input tile in LDS with 16-byte loads (R is chosen at load time so the tile is about 32 KiB), then each
// thread produces 4 consecutive output elements per step and stores them as one 16-byte store.  (row, column) of a thread's first
// element is derived once and stepped with wrap-around.  Tiles whose ends are not 16-byte aligned (F_in or F not a multiple of 4, an
// unaligned caller pointer) take per-element loads / stores for the partial quads at their ends.  Column descriptors (16 B), the
// impute / affine constants and the sorted key tables are copied into LDS behind the row tile when they fit 16 KB together (F' up to a
// few hundred columns with short key tables), else read from global memory (L1 / L2): read from global memory, every element waited on
// an L1/L2 load and every LabelEncoder column on a chain of them (profiles/r09_prep.txt).  LabelEncoder columns (and the strict check
// of a zeros = 0 OneHotEncoder) binary-search their table.
//
// Every step is one rounded f32 operation and nothing is contracted into an FMA, so a numpy f32 restatement reproduces the output bit
// for bit.  The zeros = 0 failure word is written with ordinary stores: every writer of one OneHotEncoder writes the same value.
#include "device_common.hpp"

#include "../host/prep.hpp"

#pragma clang fp contract(off)

namespace infera_hip::kern {

namespace {

constexpr int kBlock = 256;
constexpr size_t kStageTabBytes = 16384;  // descriptors + constants (32 B per column) + key pairs staged in LDS up to this size

// lower bound of k among cnt ascending keys; *val: the value of an equal key
__device__ __forceinline__ bool prep_find(const float2 *__restrict__ tab, uint32_t off, uint32_t cnt, float k, float *val) {
  uint32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tab[off + mid].x < k) lo = mid + 1;
    else hi = mid;
  }
  if (lo < cnt && tab[off + lo].x == k) {
    *val = tab[off + lo].y;
    return true;
  }
  return false;
}

// column program j (descriptor d) on the gathered value x
__device__ __forceinline__ float prep_eval(float x, const uint4 d, const float4 *__restrict__ cst, const float2 *__restrict__ tab, int j,
                                           int *err) {
  const uint32_t w = d.x;
  if (w & kPrepTrunc) x = truncf(x);
  if (w & (kPrepImpute | kPrepAffine)) {
    const float4 k = cst[j];  // replaced, imputed, offset, scale
    if (w & kPrepImpute) {
      const bool hit = (w & kPrepImputeNan) ? isnan(x) : x == k.x;
      x = hit ? k.y : x;
    }
    if (w & kPrepAffine) {
      x = x - k.z;
      x = x * k.w;
    }
  }
  const uint32_t kind = (w >> kPrepKindShift) & 3u;
  const float c = __uint_as_float(d.z);
  if (kind == kPrepBin) return x > c ? 1.f : 0.f;
  if (kind == kPrepOneHot) {
    const float t = truncf(x);
    if (w & kPrepStrict) {
      float v;
      if (isnan(t) || !prep_find(tab, d.y, d.w, t, &v)) *err = int(w >> kPrepStrictShift);
    }
    return t == c ? 1.f : 0.f;
  }
  if (kind == kPrepLookup) {
    const float k = (w & kPrepIntKey) ? truncf(x) : x;
    if (isnan(k)) return (w & kPrepNanKey) ? tab[d.y + d.w].y : c;
    float v;
    return prep_find(tab, d.y, d.w, k, &v) ? v : c;
  }
  return x;
}

// STAGED: the descriptors, constants and key tables are copied into LDS behind the row tile (plans whose tables fit kStageTabBytes)
template <bool STAGED>
__global__ __launch_bounds__(kBlock) void prep_kernel(const float *__restrict__ x, int F_in, const uint4 *__restrict__ g_desc,
                                                      const float4 *__restrict__ g_cst, const float2 *__restrict__ g_tab, int ntab,
                                                      float *__restrict__ y, int F, int64_t nr, int R, int tile_floats, int *err) {
  extern __shared__ float tile[];
  const int tid = int(threadIdx.x);
  const uint4 *desc = g_desc;
  const float4 *cst = g_cst;
  const float2 *tab = g_tab;
  if constexpr (STAGED) {
    uint4 *s_desc = reinterpret_cast<uint4 *>(tile + tile_floats);
    float4 *s_cst = reinterpret_cast<float4 *>(s_desc + F);
    float2 *s_tab = reinterpret_cast<float2 *>(s_cst + F);
    for (int i = tid; i < F; i += kBlock) {
      s_desc[i] = g_desc[i];
      s_cst[i] = g_cst[i];
    }
    for (int i = tid; i < ntab; i += kBlock) s_tab[i] = g_tab[i];
    desc = s_desc;
    cst = s_cst;
    tab = s_tab;
  }
  const int64_t r0 = int64_t(blockIdx.x) * R;
  const int nrow = int(min(int64_t(R), nr - r0));
  // ---- stage the input tile: quads aligned in memory, element e of the tile at tile[lead + e]
  const float *src = x + r0 * F_in;
  const int n = nrow * F_in;
  const int lead = int((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
  const int nchunk = (lead + n + 3) >> 2;
  for (int q = tid; q < nchunk; q += kBlock) {
    const int e0 = 4 * q - lead;
    f32x4 v;
    if (e0 >= 0 && e0 + 4 <= n) {
      v = *reinterpret_cast<const f32x4 *>(src + e0);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = (e0 + k >= 0 && e0 + k < n) ? src[e0 + k] : 0.f;
    }
    *reinterpret_cast<f32x4 *>(tile + 4 * q) = v;
  }
  __syncthreads();
  // ---- the output tile, 4 consecutive elements per thread and step (quads aligned in memory: element e at dst + e)
  float *dst = y + r0 * F;
  const int m = nrow * F;
  const int olead = int((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);
  const int ochunk = (olead + m + 3) >> 2;
  constexpr int kStep = 4 * kBlock;
  const int drow = kStep / F, dcol = kStep - drow * F;
  int e0 = 4 * tid - olead;
  int row = e0 >= 0 ? e0 / F : -((-e0 + F - 1) / F);  // (floor: the first quad may start before the tile)
  int col = e0 - row * F;
  for (int q = tid; q < ochunk; q += kBlock) {
    f32x4 o;
    int r = row, c = col;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int e = e0 + k;
      o[k] = 0.f;
      if (e >= 0 && e < m) {
        const uint4 d = desc[c];
        o[k] = prep_eval(tile[lead + r * F_in + int(d.x & 0xFFFFu)], d, cst, tab, c, err);
      }
      if (++c == F) c = 0, r++;
    }
    if (e0 >= 0 && e0 + 4 <= m) {
      *reinterpret_cast<f32x4 *>(dst + e0) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (e0 + k >= 0 && e0 + k < m) dst[e0 + k] = o[k];
    }
    e0 += kStep;
    col += dcol;
    row += drow;
    if (col >= F) col -= F, row++;
  }
}

}  // namespace

void prep(hipStream_t s, const float *x, int F_in, const uint32_t *desc, const float *cst, const float *tab, int ntab, float *y, int F, int64_t rows,
          int R, int *err) {
  if (rows <= 0 || F <= 0) return;
  const int64_t blocks = (rows + R - 1) / R;
  const int tile_floats = (R * F_in + 8 + 3) / 4 * 4;  // (16-byte aligned end: the staged tables follow)
  const size_t tab_bytes = size_t(F) * 32 + size_t(ntab) * 8;
  const bool staged = tab_bytes <= kStageTabBytes;
  const size_t lds = size_t(tile_floats) * 4 + (staged ? tab_bytes : 0);
  const auto *d4 = reinterpret_cast<const uint4 *>(desc);
  const auto *c4 = reinterpret_cast<const float4 *>(cst);
  const auto *t2 = reinterpret_cast<const float2 *>(tab);
  if (staged)
    hipLaunchKernelGGL(prep_kernel<true>, dim3(unsigned(blocks)), dim3(kBlock), lds, s, x, F_in, d4, c4, t2, ntab, y, F, rows, R, tile_floats, err);
  else
    hipLaunchKernelGGL(prep_kernel<false>, dim3(unsigned(blocks)), dim3(kBlock), lds, s, x, F_in, d4, c4, t2, ntab, y, F, rows, R, tile_floats, err);
}

}  // namespace infera_hip::kern
