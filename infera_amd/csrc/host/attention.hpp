// attention.hpp -- the caps of the Transformer-encoder kernels (hip/attention.hip, hip/layernorm.hip), shared by the lowering (which refuses
// by name what the kernels cannot serve: INTEGRATION.md section 2.6) and the launchers.
#pragma once

#include <cstdint>

namespace infera_hip {

constexpr int64_t kAttnMaxT = 1024;   // window length: the [T, T] mask constant and the 32-bit score indices
constexpr int64_t kAttnMaxDh = 128;   // head width: Q and the output tile of a wave live in registers (8 + 8 fragments of 16 columns)
constexpr int64_t kAttnMaxHeads = 1024;
// how a row mask's fill reaches a masked key's score (Step::rm_mode): added to the scaled score (BERT) or in its place (masked_fill)
enum RowMaskMode : int { kRowMaskAdd = 0, kRowMaskReplace = 1 };
// a fill at or below this (the finfo.min family and -inf) excludes its keys; anything above it is a bias that goes through the softmax
constexpr float kRowMaskExcludingFill = -1e30f;
// The Rotary step (hip/rotary.hip) shares kAttnMaxT, kAttnMaxDh and kAttnMaxHeads.  Whether a view (ld, off) of heads of dh columns, rd of them
// rotated, takes the kernel's 16-byte form (the launcher also wants 16-byte aligned pointers); else the scalar form: the same bits
inline bool rotary_vec4(int64_t ld, int64_t off, int64_t dh, int64_t rd, bool interleaved) {
  return ld % 4 == 0 && off % 4 == 0 && dh % 4 == 0 && (interleaved ? rd % 4 == 0 : rd % 8 == 0);
}
constexpr int64_t kLnMaxE = 4096;     // LayerNorm vector length: one vector is held in the registers of one wave (64 floats per lane)

}  // namespace infera_hip
