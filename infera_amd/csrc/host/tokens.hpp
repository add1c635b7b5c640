// tokens.hpp -- the crossing from the image path to the table path as one step kind: what the lowering
// checks and folds for a Tokens step, and the caps of its kernels (hip/tokens.hip).
//   in  [rows, C, S]        the tensor a convolutional step wrote (S = H * W or L), NCHW order or channel-quad planes [C/4][S][4]
//   out [rows, T, E]        a flat window, T = P + S, E = C:
//     out[r, P + s, c] = in[r, c, s] (+ pos[P + s, c])
//     out[r, p, c]     = prefix[p, c] (+ pos[p, c])      for p < P  (class / distillation tokens: the same constant rows in every image)
//   The add is one rounded f32 addition per element, made on the device: the bits of BinaryConst('+') behind an unfused step.
// Caps (refused at load, tokens_refusal):
//   P <= kTokensMaxPrefix    the constant rows are written by the work groups of the first position tile, element by element
//   C <= kTokensMaxC, S <= kTokensMaxS    so that the tiles of one image, ceil(C / 32) * ceil(S / 64) <= 2^25, fit one grid axis
//   T * E < 2^31             elements per window row (the planner's cap on every activation row); element offsets are 64-bit on the device,
//                            so rows * T * E may exceed 32 bits
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace infera_hip {

constexpr int64_t kTokensMaxPrefix = 16;
constexpr int64_t kTokensMaxC = int64_t(1) << 16;
constexpr int64_t kTokensMaxS = int64_t(1) << 20;

// why a crossing cannot be served ("" = it can): x_shape = the shape [N, C, spatial...] of the convolutional tensor
std::string tokens_refusal(const std::vector<int64_t> &x_shape);

// why `n_rows` constant rows of `width` columns cannot be put in front of a window of S positions and E columns that has `have` already
std::string tokens_prefix_refusal(int64_t have, int64_t n_rows, int64_t width, int64_t E);

// the rows of an f32 constant [1, p, E] / [p, E] / [B, p, E] (B equal slices, as an Expand over a fixed batch leaves them) as p * E floats;
// false: another shape, or slices that differ
bool tokens_prefix_rows(const std::vector<int64_t> &dims, const std::vector<float> &data, int64_t *p, int64_t *width, std::vector<float> *rows);

}  // namespace infera_hip
