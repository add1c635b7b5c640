// embed.hip -- embedding lookups (Gather of a constant table by runtime indices), the column picks, casts and offsets in front of them, and
// the Concat with numeric columns behind them, as one pass (host/embed.hpp: pieces).
//
// embed_kernel is memory-bound: per row it reads W source floats once, gathers sum(d_j) table floats and writes F floats once.  A work
// group owns a tile of R rows (R from the model alone, so nothing depends on the grid).  The tile's source columns are one contiguous
// range of R * W floats: they are staged in LDS with 16-byte loads (STAGED; a source row too wide for that is read where it lies).  The
// piece descriptors (32 B each) and, for rows of up to kEmbedMapMaxF columns, a column -> piece map (MAPPED; else a binary search over the
// pieces' first columns) sit in LDS in front of the tile.  Each thread then produces quads of 4 consecutive output floats, aligned in
// memory: where a quad lies in one piece it takes one index (validated once) and one 16-byte table load when the table address allows it,
// four 4-byte loads otherwise; a quad that straddles pieces or rows is put together element by element.  A gap piece (V < 0) is zeros:
// the columns of a Concat input that another step computes and a CopyCols behind this step writes.  Every full quad leaves as one
// 16-byte store, the partial quads at the ends of a tile as element stores.
//
// No value is computed: every output float is a table's or the source's bit pattern.  An index outside [-V, V - 1] (NaN and infinities
// included) never reaches an address: the load goes to row 0 and the call's failure word gets the piece's node id, by an ordinary store
// (every writer of one node writes the same value; which node wins among several bad ones is not defined, one of them is reported).
// No atomics.
#include "device_common.hpp"

#include "../host/embed.hpp"

namespace infera_hip::kern {

namespace {

constexpr int kBlock = 256;

// the table row of source value v, or 0 with the failure word raised
__device__ __forceinline__ int embed_row(float v, int V, int offset, int node, int *err) {
  const float t = truncf(v);
  // (V and |offset| are at most 2^24: an index in range has |t| <= 2^25, and such a t plus the offset stays inside int)
  int i = fabsf(t) <= 33554432.f ? int(t) + offset : V;
  if (i < 0) i += V;
  if (i < 0 || i >= V) {
    if (err) *err = node;
    i = 0;
  }
  return i;
}

// NT: the full quads leave as non-temporal stores (the default; INFERA_EMBED_NT=0 takes plain stores; measured in profiles/r19_embed.txt)
template <bool STAGED, bool MAPPED, bool NT>
__global__ __launch_bounds__(kBlock) void embed_kernel(const float *__restrict__ x, int W, const int4 *__restrict__ g_desc, int P,
                                                       const uint32_t *__restrict__ g_map, int map_words, const float *__restrict__ tab,
                                                       float *__restrict__ y, int F, int64_t nr, int R, int *err) {
  extern __shared__ float lds[];
  const int tid = int(threadIdx.x);
  int4 *s_desc = reinterpret_cast<int4 *>(lds);
  uint32_t *s_map32 = reinterpret_cast<uint32_t *>(s_desc + 2 * P);
  const uint16_t *s_map = reinterpret_cast<const uint16_t *>(s_map32);
  float *tile = reinterpret_cast<float *>(s_map32 + map_words);
  for (int i = tid; i < 2 * P; i += kBlock) s_desc[i] = g_desc[i];
  if constexpr (MAPPED)
    for (int i = tid; i < map_words; i += kBlock) s_map32[i] = g_map[i];
  const int64_t r0 = int64_t(blockIdx.x) * R;
  const int nrow = int(min(int64_t(R), nr - r0));
  const float *src = x + r0 * W;
  int lead = 0;
  if constexpr (STAGED) {  // element e of the tile's source at tile[lead + e]; quads aligned in memory
    const int n = nrow * W;
    lead = int((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
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
  }
  __syncthreads();
  auto source = [&](int r, int c) -> float {
    if constexpr (STAGED) return tile[lead + r * W + c];
    else return src[int64_t(r) * W + c];
  };
  auto piece_of = [&](int c) -> int {
    if constexpr (MAPPED) return int(s_map[c]);
    int lo = 0, hi = P - 1;  // the last piece that starts at or before c
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_desc[2 * mid].x <= c) lo = mid;
      else hi = mid - 1;
    }
    return lo;
  };
  // ---- the output tile: element e at dst + e, quads aligned in memory
  float *dst = y + r0 * int64_t(F);
  const int64_t m = int64_t(nrow) * F;
  const int olead = int((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);
  const int64_t ochunk = (olead + m + 3) >> 2;
  constexpr int kStep = 4 * kBlock;
  const int drow = kStep / F, dcol = kStep - drow * F;
  int64_t e0 = 4 * tid - olead;
  int row = e0 >= 0 ? int(e0 / F) : -int((-e0 + F - 1) / F);  // (floor: the first quad may start up to 3 elements before the tile)
  int col = int(e0 - int64_t(row) * F);
  for (int64_t q = tid; q < ochunk; q += kBlock) {
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    const bool full = e0 >= 0 && e0 + 4 <= m;
    bool done = false;
    if (full && col + 4 <= F) {
      const int p = piece_of(col);
      const int4 d0 = s_desc[2 * p];  // out, len, src, V
      if (col + 4 <= d0.x + d0.y) {
        const int within = col - d0.x;
        if (d0.w == 0) {
#pragma unroll
          for (int k = 0; k < 4; k++) o[k] = source(row, d0.z + within + k);
        } else if (d0.w < 0) {  // a gap: zeros, a later CopyCols writes these columns
        } else {
          const int4 d1 = s_desc[2 * p + 1];  // offset, table base, node id
          const int i = embed_row(source(row, d0.z), d0.w, d1.x, d1.z, err);
          const int at = i * d0.y + within;  // (V * d <= 2^27)
          const float *t = tab + size_t(d1.y) + size_t(at);
          if ((at & 3) == 0) {
            o = *reinterpret_cast<const f32x4 *>(t);
          } else {
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = t[k];
          }
        }
        done = true;
      }
    }
    if (!done) {
      int r = row, c = col;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int64_t e = e0 + k;
        if (e >= 0 && e < m) {
          const int p = piece_of(c);
          const int4 d0 = s_desc[2 * p];
          if (d0.w == 0) {
            o[k] = source(r, d0.z + (c - d0.x));
          } else if (d0.w < 0) {  // a gap
          } else {
            const int4 d1 = s_desc[2 * p + 1];
            const int i = embed_row(source(r, d0.z), d0.w, d1.x, d1.z, err);
            o[k] = tab[size_t(d1.y) + size_t(i * d0.y + (c - d0.x))];
          }
        }
        if (++c == F) c = 0, r++;
      }
    }
    if (full) {
      if constexpr (NT) __builtin_nontemporal_store(o, reinterpret_cast<f32x4 *>(dst + e0));
      else *reinterpret_cast<f32x4 *>(dst + e0) = o;
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

bool embed(hipStream_t s, const float *x, int W, const int32_t *desc, int P, const uint16_t *map, int map_entries, const float *tab, float *y, int64_t F,
           int64_t rows, int R, bool staged, int *err, bool nt) {
  if (rows <= 0 || F <= 0) return true;
  if (P < 1 || P > kEmbedMaxPieces || R < 1 || R > kEmbedMaxRowsPerTile || F >= (int64_t(1) << 31) - 4096 || map_entries % 8 != 0) return false;
  const int64_t blocks = (rows + R - 1) / R;
  const int map_words = map ? map_entries / 2 : 0;
  const int64_t tile_floats = staged ? (int64_t(R) * W + 8 + 3) / 4 * 4 : 0;
  const int64_t lds = int64_t(P) * kEmbedDescInts * 4 + int64_t(map_words) * 4 + tile_floats * 4;
  if (lds > kEmbedLdsBytes || blocks > 0x7fffffff) return false;
  const auto *d4 = reinterpret_cast<const int4 *>(desc);
  const auto *m32 = reinterpret_cast<const uint32_t *>(map);
#define INFERA_EMBED_LAUNCH(ST, MP)                                                                                                                    \
  do {                                                                                                                                                \
    if (nt)                                                                                                                                           \
      hipLaunchKernelGGL((embed_kernel<ST, MP, true>), dim3(unsigned(blocks)), dim3(kBlock), size_t(lds), s, x, W, d4, P, m32, map_words, tab, y, int(F), rows, R, err); \
    else                                                                                                                                              \
      hipLaunchKernelGGL((embed_kernel<ST, MP, false>), dim3(unsigned(blocks)), dim3(kBlock), size_t(lds), s, x, W, d4, P, m32, map_words, tab, y, int(F), rows, R, err); \
  } while (0)
  if (staged && map) INFERA_EMBED_LAUNCH(true, true);
  else if (staged) INFERA_EMBED_LAUNCH(true, false);
  else if (map) INFERA_EMBED_LAUNCH(false, true);
  else INFERA_EMBED_LAUNCH(false, false);
#undef INFERA_EMBED_LAUNCH
  return true;
}

}  // namespace infera_hip::kern
