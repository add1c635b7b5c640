// tokens.cpp -- checks and table folding of the Tokens step (host/tokens.hpp).
#include "tokens.hpp"

#include <cstring>

namespace infera_hip {

std::string tokens_refusal(const std::vector<int64_t> &x_shape) {
  const size_t rank = x_shape.size();
  if (rank != 3 && rank != 4) return "the tensor behind the view must be [N,C,L] or [N,C,H,W], got rank " + std::to_string(rank);
  if (x_shape[1] <= 0) return "a symbolic channel count";
  int64_t S = 1;
  for (size_t i = 2; i < rank; i++) {
    if (x_shape[i] <= 0) return "symbolic spatial extents (only the row axis may be symbolic)";
    if (x_shape[i] > kTokensMaxS) return "a spatial extent of " + std::to_string(x_shape[i]) + " is above the cap of " + std::to_string(kTokensMaxS) + " positions";
    S *= x_shape[i];
  }
  if (x_shape[1] > kTokensMaxC) return "C = " + std::to_string(x_shape[1]) + " channels, above the cap of " + std::to_string(kTokensMaxC);
  if (S > kTokensMaxS) return "S = " + std::to_string(S) + " positions, above the cap of " + std::to_string(kTokensMaxS);
  return "";
}

std::string tokens_prefix_refusal(int64_t have, int64_t n_rows, int64_t width, int64_t E) {
  if (width != E) return "the constant rows are " + std::to_string(width) + " wide, the tokens E = " + std::to_string(E);
  if (n_rows < 1) return "an empty constant operand";
  if (have + n_rows > kTokensMaxPrefix)
    return std::to_string(have + n_rows) + " constant rows in front of the tokens, above the cap of " + std::to_string(kTokensMaxPrefix);
  return "";
}

bool tokens_prefix_rows(const std::vector<int64_t> &dims, const std::vector<float> &data, int64_t *p, int64_t *width, std::vector<float> *rows) {
  if (dims.size() != 2 && dims.size() != 3) return false;
  const int64_t B = dims.size() == 3 ? dims[0] : 1, P = dims[dims.size() - 2], E = dims.back();
  if (B < 1 || P < 1 || E < 1 || P > (int64_t(1) << 24) || E > (int64_t(1) << 24) || int64_t(data.size()) / B != P * E || int64_t(data.size()) % B != 0) return false;
  const size_t per = size_t(P * E);
  for (int64_t b = 1; b < B; b++)
    if (std::memcmp(data.data(), data.data() + size_t(b) * per, per * sizeof(float)) != 0) return false;
  *p = P;
  *width = E;
  rows->assign(data.begin(), data.begin() + int64_t(per));
  return true;
}

}  // namespace infera_hip
