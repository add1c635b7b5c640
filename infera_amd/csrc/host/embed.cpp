// embed.cpp -- the Embed step's load-time checks and packing (host/embed.hpp).
#include "embed.hpp"

#include <algorithm>

namespace infera_hip {

std::string embed_table_refusal(const std::vector<int64_t> &dims) {
  if (dims.empty() || dims.size() > 2) return "a table of rank " + std::to_string(dims.size()) + "; only [V, d] and [V] tables are looked up";
  const int64_t V = dims[0], d = dims.size() == 2 ? dims[1] : 1;
  if (V <= 0 || d <= 0) return "an empty table (V = " + std::to_string(V) + ", d = " + std::to_string(d) + ")";
  if (V > kEmbedMaxV) return "a table of V = " + std::to_string(V) + " rows, above the cap of " + std::to_string(kEmbedMaxV) + " (2^24: indices arrive as f32 values)";
  if (d > kEmbedMaxD) return "a table of d = " + std::to_string(d) + " columns, above the cap of " + std::to_string(kEmbedMaxD);
  return "";
}

std::string pack_embed(EmbedPack &p) {
  const int64_t P = int64_t(p.pieces.size());
  if (P < 1) return "no pieces";
  if (P > kEmbedMaxPieces) return std::to_string(P) + " pieces, above the cap of " + std::to_string(kEmbedMaxPieces) + " per step";
  int64_t F = 0;
  p.gathered = 0;
  for (const EmbedPiece &q : p.pieces) {
    if (q.d <= 0 || q.out != F || q.src < 0 || (q.table != -2 && q.src + (q.table < 0 ? q.d : 1) > p.W)) return "internal: a piece outside its row";
    if (__builtin_add_overflow(F, q.d, &F) || F >= (int64_t(1) << 31) - 4096) return "an output row beyond 2^31 elements";
    if (q.table >= 0) p.gathered += q.d;
  }
  p.F = F;
  p.table_base.clear();
  int64_t elems = 0;
  for (const auto &t : p.tables) {
    p.table_base.push_back(elems);
    elems += (int64_t(t->size()) + 3) / 4 * 4;  // (the lowering has held the sum to kEmbedMaxTableElems)
  }
  p.tab.assign(size_t(elems), 0.f);
  for (size_t i = 0; i < p.tables.size(); i++) std::copy(p.tables[i]->begin(), p.tables[i]->end(), p.tab.begin() + p.table_base[i]);
  p.n_tables = int64_t(p.tables.size());
  p.tables.clear();  // (the packed copy is the one the step keeps)
  p.desc.assign(size_t(P) * kEmbedDescInts, 0);
  for (int64_t i = 0; i < P; i++) {
    const EmbedPiece &q = p.pieces[size_t(i)];
    int32_t *d = &p.desc[size_t(i) * kEmbedDescInts];
    d[0] = int32_t(q.out), d[1] = int32_t(q.d), d[2] = int32_t(q.src);
    if (q.table >= 0) d[3] = int32_t(q.V), d[4] = int32_t(q.offset), d[5] = int32_t(p.table_base[size_t(q.table)]), d[6] = q.node;
    if (q.table == -2) d[3] = -1;
  }
  p.map.clear();
  if (F <= kEmbedMapMaxF) {
    p.map.assign(size_t((F + 7) / 8 * 8), 0);
    for (int64_t i = 0; i < P; i++)
      for (int64_t c = 0; c < p.pieces[size_t(i)].d; c++) p.map[size_t(p.pieces[size_t(i)].out + c)] = uint16_t(i);
  }
  // rows per tile: about kEmbedTileFloats output floats a work group, as many source rows as the LDS behind the descriptors and the map holds
  const int64_t target = std::clamp<int64_t>(kEmbedTileFloats / F, 1, kEmbedMaxRowsPerTile);
  const int64_t avail = std::min<int64_t>(kEmbedTileBytes, kEmbedLdsBytes - P * kEmbedDescInts * 4 - int64_t(p.map.size()) * 2 - 64);
  const int64_t fit = (avail / 4 - 12) / std::max<int64_t>(p.W, 1);
  p.staged = fit >= 1;
  p.R = int(p.staged ? std::min(target, fit) : target);
  return "";
}

}  // namespace infera_hip
