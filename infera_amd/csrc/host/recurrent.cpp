// recurrent.cpp -- LSTM / GRU / RNN: validation, folded biases, one row of initial state, [W | R] in MFMA fragment order.
#include "recurrent.hpp"

#include <algorithm>
#include <cmath>

namespace infera_hip {

namespace {

[[noreturn]] void fail(const std::string &why) { throw RnnError("unsupported operator form: " + why); }

std::string num(int64_t v) { return std::to_string(v); }

std::string dims_str(const std::vector<int64_t> &s) {
  std::string o = "[";
  for (size_t i = 0; i < s.size(); i++) o += (i ? "," : "") + num(s[i]);
  return o + "]";
}

const std::vector<float> &f32_const(const RnnInput &in, const char *what, const std::vector<int64_t> &want) {
  if (!in.c || in.c->dtype != onnx::kFloat) fail(std::string(what) + " must be a constant f32 tensor");
  if (in.c->dims != want) fail(std::string(what) + " has shape " + dims_str(in.c->dims) + ", expected " + dims_str(want));
  return in.c->f32;
}

// one row [D][H] of an initial state that is the same for every row: [D, b, H] (layout 0) or [b, D, H] (layout 1)
std::vector<float> state_row(const RnnInput &in, const char *what, int64_t D, int64_t H, int64_t Hp, int64_t layout) {
  std::vector<float> out(size_t(D * Hp), 0.f);
  if (!in.present) return out;
  if (!in.c || in.c->dtype != onnx::kFloat) fail(std::string(what) + " is computed from the rows (only a value that is the same for every row is supported)");
  const auto &d = in.c->dims;
  const size_t bi = layout ? 0 : 1, di = layout ? 1 : 0;
  if (d.size() != 3 || d[di] != D || d[2] != H || d[bi] < 1)
    fail(std::string(what) + " has shape " + dims_str(d) + ", expected " + (layout ? "[rows," + num(D) + "," + num(H) + "]" : "[" + num(D) + ",rows," + num(H) + "]"));
  const int64_t b = d[bi];
  auto at = [&](int64_t dd, int64_t r, int64_t j) { return in.c->f32[size_t(layout ? (r * D + dd) * H + j : (dd * b + r) * H + j)]; };
  for (int64_t dd = 0; dd < D; dd++)
    for (int64_t j = 0; j < H; j++) {
      for (int64_t r = 1; r < b; r++)
        if (!(at(dd, r, j) == at(dd, 0, j))) fail(std::string(what) + " differs per row");
      out[size_t(dd * Hp + j)] = at(dd, 0, j);
    }
  return out;
}

}  // namespace

RnnPack pack_recurrent(const onnx::NodeDef &n, int64_t T, int64_t F, const RnnInput &W, const RnnInput &R, const RnnInput &B, const RnnInput &seq_lens,
                       const RnnInput &h0, const RnnInput &c0, const RnnInput &P) {
  RnnPack p;
  p.op = n.op == "LSTM" ? kRnnLstm : n.op == "GRU" ? kRnnGru : kRnnPlain;
  p.G = p.op == kRnnLstm ? 4 : p.op == kRnnGru ? 3 : 1;
  const int64_t G = p.G;
  p.T = T;
  p.F = F;
  if (!n.attr("hidden_size")) fail("missing hidden_size");
  const int64_t H = p.H = n.attr_i("hidden_size", 0);
  if (H < 1) fail("hidden_size " + num(H));
  if (H > kRnnMaxH) fail("hidden_size " + num(H) + " is above the cap of " + num(kRnnMaxH));
  if (F > kRnnMaxF) fail("input width " + num(F) + " is above the cap of " + num(kRnnMaxF));
  if (T > kRnnMaxT) fail("sequence length " + num(T) + " is above the cap of " + num(kRnnMaxT));
  const std::string dir = n.attr_s("direction", "forward");
  if (dir != "forward" && dir != "reverse" && dir != "bidirectional") fail("direction '" + dir + "'");
  const int64_t D = p.D = dir == "bidirectional" ? 2 : 1;
  p.reverse = dir == "reverse";
  p.layout = n.attr_i("layout", 0);
  if (p.layout != 0 && p.layout != 1) fail("layout " + num(p.layout));
  p.lbr = p.op == kRnnGru && n.attr_i("linear_before_reset", 0) != 0;
  if (n.attr("clip")) fail("clip");
  if (p.op == kRnnLstm && n.attr_i("input_forget", 0) != 0) fail("input_forget = 1");
  if (const onnx::Attribute *a = n.attr("activation_alpha"); a && !a->floats.empty()) fail("activation_alpha");
  if (const onnx::Attribute *a = n.attr("activation_beta"); a && !a->floats.empty()) fail("activation_beta");
  if (const onnx::Attribute *a = n.attr("activations"); a && !a->strings.empty()) {
    std::vector<std::string> dflt = p.op == kRnnLstm ? std::vector<std::string>{"Sigmoid", "Tanh", "Tanh"}
                                    : p.op == kRnnGru ? std::vector<std::string>{"Sigmoid", "Tanh"}
                                                      : std::vector<std::string>{"Tanh"};
    const size_t per = dflt.size();
    if (p.op == kRnnPlain && a->strings[0] == "Relu") dflt = {"Relu"}, p.relu = true;
    std::string got;
    for (const auto &s : a->strings) got += (got.empty() ? "" : ", ") + s;
    bool ok = a->strings.size() == per * size_t(D);
    for (size_t i = 0; ok && i < a->strings.size(); i++) ok = a->strings[i] == dflt[i % per];
    if (!ok) fail("activations (" + got + ") other than the defaults" + (p.op == kRnnPlain ? " (Tanh or Relu, the same for both directions)" : ""));
  }
  // (lengths that are a column of a graph input never come here: the lowering traces them, find_seq_lens; what is left is a constant, which
  // cannot match a symbolic row count)
  if (seq_lens.present && !(seq_lens.c && seq_lens.c->count() == 0)) fail("sequence_lens (per-row sequence lengths)");

  const std::vector<float> &w = f32_const(W, "W", {D, G * H, F});
  const std::vector<float> &r = f32_const(R, "R", {D, G * H, H});
  const std::vector<float> *b = B.present ? &f32_const(B, "B", {D, 2 * G * H}) : nullptr;
  if (P.present) {
    if (!P.c || P.c->dtype != onnx::kFloat) fail("peepholes P must be a constant");
    for (float v : P.c->f32)
      if (v != 0.f) fail("peepholes P that are not all zero");
  }

  const int64_t Fp = p.Fp = (F + 15) / 16 * 16, Hp = p.Hp = (H + 15) / 16 * 16, K = Fp + Hp;
  p.h0 = state_row(h0, "initial_h", D, H, Hp, p.layout);
  p.c0 = state_row(c0, "initial_c", D, H, Hp, p.layout);
  p.bias.assign(size_t(D * G * Hp), 0.f);
  p.bias2.assign(size_t(D * Hp), 0.f);
  if (b)
    for (int64_t d = 0; d < D; d++)
      for (int64_t g = 0; g < G; g++)
        for (int64_t j = 0; j < H; j++) {
          const float wb = (*b)[size_t(d * 2 * G * H + g * H + j)], rb = (*b)[size_t(d * 2 * G * H + (G + g) * H + j)];
          if (p.lbr && g == 2) {  // Rb_h stays inside r (.) (...)
            p.bias[size_t((d * G + g) * Hp + j)] = wb;
            p.bias2[size_t(d * Hp + j)] = rb;
          } else {
            p.bias[size_t((d * G + g) * Hp + j)] = float(double(wb) + double(rb));
          }
        }
  auto wr = [&](int64_t d, int64_t g, int64_t j, int64_t k) -> float {  // [W | R] of direction d, gate g, unit j, padded column k
    if (j >= H) return 0.f;
    if (k < Fp) return k < F ? w[size_t((d * G * H + g * H + j) * F + k)] : 0.f;
    const int64_t kh = k - Fp;
    return kh < H ? r[size_t((d * G * H + g * H + j) * H + kh)] : 0.f;
  };
  const int64_t HT = Hp / 16, KQ = K / 16;
  p.wr.assign(size_t(D * HT * KQ * G * 256), 0.f);
  size_t o = 0;
  for (int64_t d = 0; d < D; d++)
    for (int64_t t = 0; t < HT; t++)
      for (int64_t q = 0; q < KQ; q++)
        for (int64_t g = 0; g < G; g++)
          for (int lane = 0; lane < 64; lane++)
            for (int j = 0; j < 4; j++) p.wr[o++] = wr(d, g, 16 * t + (lane & 15), 16 * q + 4 * j + (lane >> 4));
  return p;
}

}  // namespace infera_hip
