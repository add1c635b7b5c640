// interact.hpp -- feature interactions as one step kind (INTEGRATION.md 2.6 "Feature interactions"): what the lowering packs
// for an Interact step and what its kernels (hip/interact.hip) read.
//   in  [rows, k, d]   T: a rows-first window, k fields of d values, flat in its buffer
//   dot  out [rows, F]: Z = T . T^T ([k, k], every entry an f32 fma chain over the d columns in one fixed order), of which the row keeps
//        the P entries `sel` names (an index i * k + j each, any order, duplicates allowed), or all k * k in order (whole).  In front of and
//        behind the selection stand the pass-through ranges: bit copies of column runs of T's own row.
//   fm   out [rows, d]: h * ((sum_f T[r, f, c])^2 - sum_f T[r, f, c]^2), evaluated as written in f32, f ascending; sum_last: the sum of
//        that over c, out [rows, 1] (h_after: h multiplies the sum, as the model wrote it).
// Caps (refused at load, interact_refusal): k <= kInteractMaxK, d <= kInteractMaxD, P <= kInteractMaxP, F < 2^31 - 4096.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace infera_hip {

constexpr int64_t kInteractMaxK = 64;
constexpr int64_t kInteractMaxD = 256;
constexpr int64_t kInteractMaxP = 4096;

enum InteractMode : int { kInteractDot = 0, kInteractFm = 1 };

struct InteractPass {  // out[r, out : out + len] = T[r, src : src + len] (src counts floats of the flat row)
  int64_t src = 0, len = 0, out = 0;
};

struct InteractPack {
  int mode = kInteractDot;
  int64_t k = 0, d = 0;
  // dot
  bool whole = false;         // the whole Gram matrix in order (sel is 0 .. k * k - 1)
  std::vector<int64_t> sel;   // indices into the flat [k * k] matrix, already in [0, k * k)
  int64_t sel_out = 0;        // the first output column of the selection
  std::vector<InteractPass> passes;
  // fm
  float h = 1.f;
  bool has_h = false, sum_last = false;
  bool h_after = false;  // the multiply by h follows the sum over the columns (else it precedes it)
  // filled by pack_interact
  int64_t P = 0, F = 0;
  int tile = 0;               // the matrix tile: 16 (k <= 16), 32 (k <= 32) or 64: the row stride of Z where a wave stages it
  std::vector<int32_t> map;   // dot: per output column, >= 0: the staged address i * tile + j of a Z entry; < 0: -(column of T's row) - 1
  int64_t bytes_per_row() const { return 4 * (k * d + F); }
};

// why these sizes cannot be served ("" = they can); P = 0 in fm mode
std::string interact_refusal(int64_t k, int64_t d, int64_t P);

// fills P, F, tile and map from the rest.  "" or why the step cannot be served
std::string pack_interact(InteractPack &p);

}  // namespace infera_hip
