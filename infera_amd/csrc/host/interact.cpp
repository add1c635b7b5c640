// interact.cpp -- the Interact step's load-time checks and packing (host/interact.hpp).
#include "interact.hpp"

namespace infera_hip {

std::string interact_refusal(int64_t k, int64_t d, int64_t P) {
  if (k < 1 || d < 1) return "an empty window (k = " + std::to_string(k) + ", d = " + std::to_string(d) + ")";
  if (k > kInteractMaxK) return "k = " + std::to_string(k) + " fields, above the cap of " + std::to_string(kInteractMaxK);
  if (d > kInteractMaxD) return "d = " + std::to_string(d) + " values per field, above the cap of " + std::to_string(kInteractMaxD);
  if (P > kInteractMaxP) return "P = " + std::to_string(P) + " selected products, above the cap of " + std::to_string(kInteractMaxP);
  return "";
}

std::string pack_interact(InteractPack &p) {
  p.P = p.mode == kInteractDot ? int64_t(p.sel.size()) : 0;
  if (const std::string why = interact_refusal(p.k, p.d, p.whole ? 0 : p.P); !why.empty()) return why;
  p.tile = p.k <= 16 ? 16 : p.k <= 32 ? 32 : 64;
  p.map.clear();
  if (p.mode == kInteractFm) {
    p.F = p.sum_last ? 1 : p.d;
    return "";
  }
  if (p.P < 1) return "an empty selection";
  int64_t F = p.P;
  for (const InteractPass &q : p.passes)
    if (q.len < 1 || q.src < 0 || q.src + q.len > p.k * p.d || __builtin_add_overflow(F, q.len, &F) || F >= (int64_t(1) << 31) - 4096)
      return q.len < 1 || q.src < 0 || q.src + q.len > p.k * p.d ? "internal: a pass-through range outside its row" : "an output row beyond 2^31 elements";
  p.F = F;
  p.map.assign(size_t(F), INT32_MIN);
  for (const InteractPass &q : p.passes) {
    if (q.out < 0 || q.out + q.len > F) return "internal: a pass-through range outside the output row";
    for (int64_t c = 0; c < q.len; c++) p.map[size_t(q.out + c)] = int32_t(-(q.src + c) - 1);
  }
  if (p.sel_out < 0 || p.sel_out + p.P > F) return "internal: the selection lies outside the output row";
  for (int64_t i = 0; i < p.P; i++) {
    const int64_t s = p.sel[size_t(i)];
    if (s < 0 || s >= p.k * p.k) return "internal: a selected index outside the matrix";
    if (p.map[size_t(p.sel_out + i)] != INT32_MIN) return "internal: the pieces of the output row overlap";
    p.map[size_t(p.sel_out + i)] = int32_t(s / p.k * p.tile + s % p.k);
  }
  for (int32_t v : p.map)
    if (v == INT32_MIN) return "internal: the pieces do not cover the output row";
  return "";
}

}  // namespace infera_hip
