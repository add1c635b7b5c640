// lowering.cpp -- ONNX graph -> Plan (shape inference with a symbolic row axis + peephole fusion).
//
// Fusions performed while walking the (topologically sorted) node list:
//   MatMul + Add(const [M])            -> Dense with bias
//   per-feature (x-mean)/std, x*s+t ... + MatMul/Gemm -> folded into the Dense weights and bias
//   Gemm(transB, alpha, beta)          -> Dense (constants folded into W / bias)
//   Dense|Conv|Binary|Affine + act     -> trailing activation fused into the producing step
//   Conv + BatchNormalization          -> BN folded into conv weights/bias
//   Identity/Dropout/Flatten/Reshape/Squeeze/Unsqueeze/Cast(f32) -> buffer alias (no kernel)
//   Shape/Gather/Concat/Unsqueeze/Squeeze/Slice/Cast on constants -> folded (the usual exporter pattern
//     Shape -> Gather -> Unsqueeze -> Concat -> Reshape; the symbolic row count is carried as 0 = "copy")
//   ReduceMean over the spatial axes -> GlobalAvgPool;  Concat(axis=1) -> one CopyCols step per input
// Dense chains are kept as consecutive Dense steps; the device executor decides whether a chain
// runs as one whole-chain fused kernel or layer by layer.
//
// struct Lowerer is declared in lowerer.hpp, which lists every member function under the file that defines it.  This file defines the
// core (constructor, buffer and value helpers, lower_node, run) and the dense, shape, conv, norm, attention, quantised and interaction
// families, indented one level as members of Lowerer; the recurrent, ai.onnx.ml, preprocessing, distance and embedding families are in
// lower_<family>.cpp.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "attention.hpp"
#include "channelnorm.hpp"
#include "deconv.hpp"
#include "interact.hpp"
#include "lowerer.hpp"
#include "nearest.hpp"
#include "recurrent.hpp"
#include "spatialnorm.hpp"
#include "tokens.hpp"

namespace infera_hip {

namespace lowering {

  Lowerer::Lowerer(const onnx::Model &model, const std::string &output_select_in) : m(model) {
    // Which graph output is served.  Default: the first (engine.rs:146-149).  A selector names another one, by output
    // name or by decimal index (infera_load_model(name, "model.onnx#probabilities"), SURVEY.md 8f-3 "named / multi outputs").
    if (m.outputs.empty()) throw InferaError::onnx("model has no outputs");
    // (a leading '?' makes the selector optional -- a URL fragment that names no output leaves the default, capi.cpp)
    const bool optional = !output_select_in.empty() && output_select_in[0] == '?';
    const std::string output_select = optional ? output_select_in.substr(1) : output_select_in;
    if (!output_select.empty()) {
      bool found = false;
      for (size_t i = 0; i < m.outputs.size() && !found; i++)
        if (m.outputs[i].name == output_select) out_index = i, found = true;
      if (!found && output_select.find_first_not_of("0123456789") == std::string::npos && output_select.size() < 6 &&
          size_t(std::atoi(output_select.c_str())) < m.outputs.size())
        out_index = size_t(std::atoi(output_select.c_str())), found = true;
      if (!found && !optional) {
        std::string names;
        for (const auto &o : m.outputs) names += (names.empty() ? "" : ", ") + o.name;
        throw InferaError::onnx("model has no output '" + output_select + "' (outputs: " + names + ")");
      }
    }
  }

  int Lowerer::new_buf(const std::vector<int64_t> &shape) {
    // [N,C,L] tensors (1-D convolutional nets) are laid out and scheduled as [N,C,1,L]; values keep their 3-D shape
    plan.buf_shape.push_back(shape.size() == 3 ? std::vector<int64_t>{shape[0], shape[1], 1, shape[2]} : shape);
    const int64_t per_row = prod(shape, 1);
    if (per_row < 0 || per_row > kMaxPerRow) throw InferaError::onnx("activation of " + std::to_string(per_row) + " elements per row is too large");
    plan.buf_per_row.push_back(per_row);
    return int(plan.buf_shape.size()) - 1;
  }

  // input i of n; a preprocessing-region value is materialised first (get_raw: as it is)
  const Val &Lowerer::get(const NodeDef &n, size_t i) {
    const Val &v = get_raw(n, i);
    if (v.pv) materialize(n.inputs[i], &n);
    if (v.nn) materialize_nearest(n.inputs[i]);
    return v;
  }
  const Val &Lowerer::get_raw(const NodeDef &n, size_t i) {
    if (i >= n.inputs.size() || n.inputs[i].empty()) unsupported(n, "missing input " + std::to_string(i));
    auto it = vals.find(n.inputs[i]);
    if (it != vals.end()) {
      // a pending distance value has no buffer: whoever reads it as a value (an alias included) reads the [rows, M] matrix.  (ArgMin, TopK
      // and Sqrt look at it first, nearest_reader.)
      if (it->second.nn) materialize_nearest(n.inputs[i]);
      return it->second;
    }
    auto ci = m.initializers.find(n.inputs[i]);
    if (ci != m.initializers.end()) return vals[n.inputs[i]] = const_val(ci->second);
    unsupported(n, "input '" + n.inputs[i] + "' is not produced by any earlier node");
  }
  bool Lowerer::has_input(const NodeDef &n, size_t i) const { return i < n.inputs.size() && !n.inputs[i].empty(); }

  const std::vector<float> &Lowerer::cf32(const NodeDef &n, const Val &v) {
    if (!v.is_const || v.c->dtype != onnx::kFloat) unsupported(n, "expected a constant f32 tensor");
    return v.c->f32;
  }

  // Binds the node's first output to `buf`.  `folded` = the node itself emitted no step (alias or
  // fused into its producer), i.e. it is an edge inside the buffer rather than a consumer of it.
  void Lowerer::set_act(const NodeDef &n, int buf, const std::vector<int64_t> &shape, bool folded, int ra) {
    Val v;
    v.buf = buf;
    v.shape = shape;
    v.ra = ra;
    vals[n.outputs[0]] = v;
    buf_names[buf].push_back(n.outputs[0]);
    if (folded) alias_edges[buf]++;
  }

  // Number of not-yet-folded consumers (incl. graph outputs) of a buffer across all its names.
  int Lowerer::live_uses(int buf) {
    int total = 0;
    for (const auto &nm : buf_names[buf]) total += uses[nm];
    return total - alias_edges[buf];
  }

  // The step that produced `v` if it can still absorb a trailing op: sole consumer is this node.
  Step *Lowerer::fusable_producer(const NodeDef &n, size_t in_idx) {
    const Val &v = get(n, in_idx);
    if (v.is_const || v.buf <= 0) return nullptr;
    if (live_uses(v.buf) != 1) return nullptr;
    auto it = producer.find(v.buf);
    if (it == producer.end()) return nullptr;
    return &plan.steps[size_t(it->second)];
  }
  // The last step, if it wrote `buf` and nothing but this node reads `buf`: it can be folded into this node and removed (drop_tail)
  const Step *Lowerer::sole_tail(int buf) {
    auto pit = producer.find(buf);
    if (buf <= 0 || pit == producer.end() || pit->second != int(plan.steps.size()) - 1 || live_uses(buf) != 1) return nullptr;
    return &plan.steps.back();
  }
  void Lowerer::drop_tail() {
    producer.erase(plan.steps.back().out);
    plan.steps.pop_back();
  }

  // Appends `s` writing a new buffer of `shape`; returns the buffer.
  int Lowerer::push_step(Step s, const std::vector<int64_t> &shape) {
    s.out = new_buf(shape);
    plan.steps.push_back(std::move(s));
    producer[plan.steps.back().out] = int(plan.steps.size()) - 1;
    return plan.steps.back().out;
  }
  Step &Lowerer::emit(Step s, const NodeDef &n, const std::vector<int64_t> &out_shape) {
    s.origin = node_label(n);
    // a rank-3 value computed elementwise from a window [rows, T, C] that a step wrote into a flat [rows, T * C] buffer (a recurrent,
    // window Dense, LayerNorm or attention step) is a window itself, not an [N, C, L] tensor: its buffer stays flat, so time steps can
    // be cut out of it.  (Values computed from the model input keep the [N, C, 1, L] registration a Conv1d behind them relies on.)
    const bool eltwise = s.kind == StepKind::Unary || s.kind == StepKind::BinaryConst || s.kind == StepKind::BinaryAct || s.kind == StepKind::AffineChannel;
    const bool window = eltwise && out_shape.size() == 3 && s.in0 > 0 && plan.buf_shape[size_t(s.in0)].size() == 2;
    set_act(n, push_step(std::move(s), window ? flat_shape(out_shape) : out_shape), out_shape);
    return plan.steps.back();
  }
  std::vector<int64_t> Lowerer::flat_shape(const std::vector<int64_t> &shape) { return {shape[0], prod(shape, 1)}; }
  // ... the same for a step whose output is a window by construction
  void Lowerer::emit_window(Step s, const NodeDef &n, const std::vector<int64_t> &out_shape) {
    if (s.origin.empty()) s.origin = node_label(n);
    set_act(n, push_step(std::move(s), flat_shape(out_shape)), out_shape);
  }

  // ------------------------------------------------------------------------------------------
  void Lowerer::dense(const NodeDef &n, bool gemm) {
    const Val &a = get(n, 0);
    const Val &b = get(n, 1);
    if (a.is_const) unsupported(n, "constant left operand is not supported");
    if (b.is_const && b.c->q_data && qdense_from_qdq(n, gemm)) return;
    if (b.is_const && hdense(n, gemm)) return;
    if (!b.is_const) {
      auto why = attn_fail.find(&n);
      if (why != attn_fail.end()) unsupported(n, "unsupported operator form: " + why->second);
      unsupported(n, "right operand must be a constant weight matrix");
    }
    if (!gemm && a.shape.size() == 3 && a.ra == 0 && b.shape.size() == 2) return dense_window(n);
    if (a.shape.size() != 2 || b.shape.size() != 2) unsupported(n, "only [rows,K] x [K,M] is supported, got " + shape_str(a.shape) + " x " + shape_str(b.shape));
    bool tA = gemm && n.attr_i("transA", 0) != 0, tB = gemm && n.attr_i("transB", 0) != 0;
    if (tA) unsupported(n, "transA=1 mixes table rows and is not supported");
    float alpha = gemm ? n.attr_f("alpha", 1.f) : 1.f, beta = gemm ? n.attr_f("beta", 1.f) : 1.f;
    const auto &w = cf32(n, b);
    int64_t K = tB ? b.shape[1] : b.shape[0], M = tB ? b.shape[0] : b.shape[1];
    if (a.shape[1] != K) unsupported(n, "inner dimensions differ: " + shape_str(a.shape) + " x " + shape_str(b.shape));
    int in_buf = a.buf;
    const std::vector<int64_t> a_shape = a.shape;
    // Per-feature affine preprocessing in front of the layer -- (x - mean) / std, x * scale + shift: the sklearn
    // StandardScaler / MinMaxScaler + linear model pipeline -- is folded into the weights:
    //   ((x (op) c) . W + b)  ==  x . (s W) + (b + t . W)   with x' = s x + t composed over the chain,
    // so the elementwise passes over the table disappear (exact algebra; rounding differs within the tolerance).
    // Only when the preprocessing value has no other consumer and its steps are the last ones emitted.
    std::vector<double> fs(size_t(K), 1.0), ft(size_t(K), 0.0);
    bool folded = false;
    std::string folded_origin;
    while (const Step *tail = sole_tail(in_buf)) {
      const Step &p = *tail;
      if (p.kind == StepKind::AffineChannel && p.act == Act::None && p.S == 1 && p.C == K) {  // BatchNormalization of the features
        for (int64_t k = 0; k < K; k++) {
          ft[size_t(k)] += fs[size_t(k)] * double(p.shift[size_t(k)]);
          fs[size_t(k)] *= double(p.scale[size_t(k)]);
        }
      } else {
        if (p.kind != StepKind::BinaryConst || p.act != Act::None || int64_t(p.cst.size()) != K) break;
        if (p.bop != '+' && p.bop != '-' && p.bop != '*' && !(p.bop == '/' && !p.const_left)) break;
        for (int64_t k = 0; k < K; k++) {
          const double c = p.cst[size_t(k)], sk = fs[size_t(k)], tk = ft[size_t(k)];
          switch (p.bop) {
            case '+': ft[size_t(k)] = sk * c + tk; break;
            case '-':
              if (p.const_left) { fs[size_t(k)] = -sk; ft[size_t(k)] = sk * c + tk; }  // c - u
              else ft[size_t(k)] = tk - sk * c;
              break;
            case '*': fs[size_t(k)] = sk * c; break;
            default: fs[size_t(k)] = sk / c; break;
          }
        }
      }
      folded = true;
      folded_origin = p.origin + (folded_origin.empty() ? "" : "+" + folded_origin);
      in_buf = p.in0;
      drop_tail();
    }
    // A wide layer over rows whose length is not a multiple of 4 floats (30 features, ...): copy the rows into a
    // zero-padded matrix first so the MFMA kernels can read them in 16-byte quads; the padded k carry zero weights.
    // (Narrow heads stream their input once and take any K.)
    // (up to 64 outputs over more than 128 columns the wide-table kernel reads the rows as they are)
    const int64_t Kp = (M > 32 && K % 4 != 0 && !(K > 128 && M <= 64)) ? (K + 3) / 4 * 4 : K;
    if (Kp != K) {
      Step p;
      p.kind = StepKind::PadCols;
      p.in0 = in_buf;
      p.K = K;
      p.M = Kp;
      p.origin = node_label(n) + "[pad]";
      in_buf = push_step(std::move(p), {a_shape[0], Kp});
    }
    Step s;
    s.kind = StepKind::Dense;
    s.in0 = in_buf;
    s.K = Kp;
    s.M = M;
    s.W.assign(size_t(Kp * M), 0.f);
    for (int64_t k = 0; k < K; k++)
      for (int64_t j = 0; j < M; j++) {
        float v = tB ? w[size_t(j * K + k)] : w[size_t(k * M + j)];
        s.W[size_t(k * M + j)] = alpha == 1.f ? v : alpha * v;
      }
    if (gemm && has_input(n, 2)) {
      const Val &c = get(n, 2);
      const auto &cv = cf32(n, c);
      if (int64_t(cv.size()) != M && cv.size() != 1) unsupported(n, "bias C must have M or 1 elements (row-independent)");
      s.bias.resize(size_t(M));
      for (int64_t j = 0; j < M; j++) {
        float v = cv.size() == 1 ? cv[0] : cv[size_t(j)];
        s.bias[size_t(j)] = beta == 1.f ? v : beta * v;
      }
    }
    if (folded) {
      std::vector<double> extra(size_t(M), 0.0);
      for (int64_t k = 0; k < K; k++)
        for (int64_t j = 0; j < M; j++) {
          const double wkj = s.W[size_t(k * M + j)];
          extra[size_t(j)] += ft[size_t(k)] * wkj;
          s.W[size_t(k * M + j)] = float(fs[size_t(k)] * wkj);
        }
      if (s.bias.empty()) s.bias.assign(size_t(M), 0.f);
      for (int64_t j = 0; j < M; j++) s.bias[size_t(j)] = float(double(s.bias[size_t(j)]) + extra[size_t(j)]);
    }
    Step &e = emit(std::move(s), n, {a_shape[0], M});
    if (folded) e.origin = folded_origin + "+" + e.origin;
  }

  // MatMul of a window [rows, T, K] by a constant [K, M]: the flat buffer IS the [rows * T, K] matrix, so this is a Dense step with a
  // repeat count (Step::rep), served by the Dense kernels over rows * T rows.  The bias Add and the activation behind it fuse as usual.
  void Lowerer::dense_window(const NodeDef &n) {
    const Val a = get(n, 0);
    const Val &b = get(n, 1);
    const auto &w = cf32(n, b);
    const int64_t N = a.shape[0], T = a.shape[1], K = b.shape[0], M = b.shape[1];
    if (T <= 0 || a.shape[2] != K) unsupported(n, "inner dimensions differ: " + shape_str(a.shape) + " x " + shape_str(b.shape));
    if (K <= 0 || M <= 0 || int64_t(w.size()) != K * M) unsupported(n, "weight matrix " + shape_str(b.shape) + " does not match its data");
    prod({T, std::max(K, M) + 3});  // (throws when T * K or T * M leaves int64)
    int in_buf = a.buf;
    const int64_t Kp = (M > 32 && K % 4 != 0 && !(K > 128 && M <= 64)) ? (K + 3) / 4 * 4 : K;  // (the rule of dense())
    if (Kp != K) {
      Step p;
      p.kind = StepKind::PadCols;
      p.in0 = in_buf;
      p.K = K;
      p.M = Kp;
      p.rep = T;
      p.origin = node_label(n) + "[pad]";
      in_buf = push_step(std::move(p), {N, T * Kp});
    }
    Step s;
    s.kind = StepKind::Dense;
    s.in0 = in_buf;
    s.K = Kp;
    s.M = M;
    s.rep = T;
    s.W.assign(size_t(Kp * M), 0.f);
    std::copy(w.begin(), w.end(), s.W.begin());
    emit_window(std::move(s), n, {N, T, M});
  }

  // Broadcast a constant against an activation's per-row shape; returns per_row floats.
  std::vector<float> Lowerer::broadcast_const(const NodeDef &n, const Val &c, const std::vector<int64_t> &act_shape) {
    const auto &cv = cf32(n, c);
    std::vector<int64_t> cs = c.shape;
    if (cs.size() > act_shape.size()) unsupported(n, "constant operand has higher rank than the activation");
    while (cs.size() < act_shape.size()) cs.insert(cs.begin(), 1);
    if (cs[0] != 1) unsupported(n, "constant operand varies along the row axis");
    for (size_t i = 1; i < cs.size(); i++)
      if (cs[i] != 1 && cs[i] != act_shape[i]) unsupported(n, "constant operand " + shape_str(c.shape) + " does not broadcast to " + shape_str(act_shape));
    int64_t per_row = prod(act_shape, 1);
    std::vector<float> out(size_t(per_row), 0.f);
    size_t r = act_shape.size();
    for (int64_t flat = 0; flat < per_row; flat++) {
      int64_t rem = flat, idx = 0, stride = 1;
      for (size_t i = r; i-- > 1;) {
        int64_t coord = rem % act_shape[i];
        rem /= act_shape[i];
        if (cs[i] != 1) idx += coord * stride;
        stride *= cs[i];
      }
      out[size_t(flat)] = cv[size_t(idx)];
    }
    return out;
  }

  float Lowerer::fold_bop(char op, float u, float v) {
    switch (op) {
      case '+': return u + v;
      case '-': return u - v;
      case '*': return u * v;
      case '/': return u / v;
      case 'm': return std::fmin(u, v);
      case 'M': return std::fmax(u, v);
      case '^': return std::pow(u, v);
      default: return u >= 0.f ? u : v * u;  // 'p'
    }
  }

  void Lowerer::binary(const NodeDef &n, char op) {
    if (n.inputs.size() != 2) unsupported(n, "exactly two inputs are supported");
    const Val &a = get(n, 0);
    const Val &b = get(n, 1);
    if (a.is_const && b.is_const && a.c->dtype == onnx::kInt64 && b.c->dtype == onnx::kInt64) return fold_int_binary(n, op, a, b);
    if (a.is_const && b.is_const) {  // fold
      const auto &x = cf32(n, a), &y = cf32(n, b);
      if (a.shape != b.shape && x.size() != 1 && y.size() != 1) unsupported(n, "constant folding needs equal shapes or a scalar");
      std::vector<float> f(std::max(x.size(), y.size()));
      for (size_t i = 0; i < f.size(); i++) f[i] = fold_bop(op, x[x.size() == 1 ? 0 : i], y[y.size() == 1 ? 0 : i]);
      vals[n.outputs[0]] = const_f32(std::move(f), x.size() >= y.size() ? a.shape : b.shape);
      return;
    }
    if (!a.is_const && !b.is_const && op == '*' && a.shape == b.shape) {
      // x * Sigmoid(x) (Swish / SiLU as exporters spell it): the Sigmoid pass and the multiply become ONE activation on x,
      // which then folds into the epilogue of the convolution / layer that produced x when nothing else reads it
      for (int side = 0; side < 2; side++) {
        const Val &x = side ? b : a, &sg = side ? a : b;
        const Step *ps = sole_tail(sg.buf);
        if (!ps || ps->kind != StepKind::Unary || ps->act != Act::Sigmoid || ps->in0 != x.buf) continue;
        drop_tail();
        alias_edges[x.buf]++;  // the Sigmoid node no longer consumes x
        apply_unary(n, side ? 1 : 0, Act::Swish, 0.f, 0.f, "Swish");
        return;
      }
    }
    if (!a.is_const && !b.is_const) {
      // per-channel gate: [N,C,H,W] (op) [N,C,1,1]  (squeeze-and-excitation blocks); either order for + * min max
      auto is_gate = [](const Val &big, const Val &small) {
        if (big.shape.size() < 3 || small.shape.size() != big.shape.size() || small.shape[0] != big.shape[0] || small.shape[1] != big.shape[1]) return false;
        for (size_t i = 2; i < small.shape.size(); i++)
          if (small.shape[i] != 1) return false;
        return prod(big.shape, 2) > 1;
      };
      const bool commutes = op == '+' || op == '*' || op == 'm' || op == 'M';
      if (a.shape != b.shape && (is_gate(a, b) || (commutes && is_gate(b, a)))) {
        const bool swap = !is_gate(a, b);
        const Val &big = swap ? b : a, &small = swap ? a : b;
        Step s;
        s.kind = StepKind::BinaryAct;
        s.in0 = big.buf;
        s.in1 = small.buf;
        s.bop = op;
        s.C = big.shape[1];
        s.S = prod(big.shape, 2);  // > 1 marks the broadcast form
        std::vector<int64_t> shape = big.shape;
        emit(std::move(s), n, shape);
        return;
      }
      // one scalar per vector: [N, K] (op) [N, 1], [N, T, E] (op) [N, T, 1]; either order (a commuting operator keeps the vectors on the left)
      auto is_row_scalar = [](const Val &big, const Val &small) {
        const size_t r = big.shape.size();
        if ((r != 2 && r != 3) || small.shape.size() != r || big.ra != 0 || small.ra != 0 || small.shape.back() != 1 || big.shape.back() < 1) return false;
        for (size_t i = 0; i + 1 < r; i++)
          if (small.shape[i] != big.shape[i]) return false;
        return true;
      };
      const bool arith = commutes || op == '-' || op == '/';
      if (a.shape != b.shape && arith && (is_row_scalar(a, b) || is_row_scalar(b, a))) {
        const bool left = !is_row_scalar(a, b);  // the scalar is the left operand
        const Val big = left ? b : a, small = left ? a : b;
        Step s;
        s.kind = StepKind::BinaryAct;
        s.in0 = big.buf;
        s.in1 = small.buf;
        s.bop = op;
        s.K = big.shape.back();
        s.rep = prod(big.shape, 1) / s.K;
        s.const_left = left && !commutes;
        if (big.shape.size() == 3) emit_window(std::move(s), n, big.shape);
        else emit(std::move(s), n, big.shape);
        return;
      }
      if (a.shape != b.shape) unsupported(n, "activation operands must have equal shapes (or [N,C,H,W] with [N,C,1,1]), got " + shape_str(a.shape) + " and " + shape_str(b.shape));
      Step s;
      s.kind = StepKind::BinaryAct;
      s.in0 = a.buf;
      s.in1 = b.buf;
      s.bop = op;
      emit(std::move(s), n, a.shape);
      return;
    }
    const bool const_left = a.is_const;
    const Val &act = const_left ? b : a;
    const Val &cst = const_left ? a : b;
    std::vector<int64_t> act_shape = act.shape;
    if (op == 'p' && const_left) unsupported(n, "PRelu needs a constant slope");
    if ((op == 'm' || op == 'M') && const_left) {  // commutative: keep the activation on the left
      Step s;
      s.kind = StepKind::BinaryConst;
      s.in0 = act.buf;
      s.bop = op;
      s.cst = broadcast_const(n, cst, act_shape);
      emit(std::move(s), n, act_shape);
      return;
    }
    // MatMul + Add(const over M) -> Dense bias
    if (op == '+') {
      Step *p = fusable_producer(n, const_left ? 1 : 0);
      const auto &cv = cf32(n, cst);
      // the position table [1, T, E] / [T, E] behind a Tokens step that nothing else reads: added in its store (one rounded addition, the
      // bits of the BinaryConst this would be).  Not in a float16 graph, where the sum is rounded to half by its own step
      if (p && p->kind == StepKind::Tokens && p->cst.empty() && !cur_half && tokens_producer(act) == p && cst.c->elem != onnx::kFloat16 &&
          ((cst.shape.size() == 3 && cst.shape[0] == 1) || cst.shape.size() == 2) && cst.shape[cst.shape.size() - 2] == p->rep && cst.shape.back() == p->K &&
          int64_t(cv.size()) == p->rep * p->K) {
        p->cst = cv;
        p->origin += "+" + node_label(n);
        set_act(n, act.buf, act_shape, true);
        return;
      }
      bool over_m = p && p->kind == StepKind::Dense && p->bias.empty() && p->act == Act::None && int64_t(cv.size()) == p->M &&
                    (cst.shape.size() == 1 || (cst.shape.size() == 2 && cst.shape[0] == 1));
      if (p && p->kind == StepKind::QDense && !p->qy.on && p->act == Act::None && p->bias.empty() && p->q_bias.empty() && int64_t(cv.size()) == p->M &&
          (cst.shape.size() == 1 || (cst.shape.size() == 2 && cst.shape[0] == 1))) {
        qdense_take_bias(n, *p, cst);
        p->origin += "+Add";
        set_act(n, act.buf, act_shape, true);
        return;
      }
      if (p && p->kind == StepKind::HDense && p->h_bias_mode == kHalfBiasNone && p->act == Act::None && cst.c->elem == onnx::kFloat16 && int64_t(cv.size()) == p->M &&
          (cst.shape.size() == 1 || (cst.shape.size() == 2 && cst.shape[0] == 1))) {
        p->h_bias = half_bits(cv);
        p->h_bias_mode = kHalfBiasMatmulAdd;
        p->origin += "+Add";
        set_act(n, act.buf, act_shape, true);
        return;
      }
      // (a float16 MatMul -> Add rounds the product before the sum: two steps, each rounded, not one Dense with a bias)
      if (over_m && !cur_half) {
        p->bias = cv;
        p->origin += "+Add";
        set_act(n, act.buf, act_shape, true);
        return;
      }
    }
    // Per-feature affine arithmetic on a [rows, K] table (x - mean, / std, * scale, + shift ...) or per-channel on an
    // [N,C,H,W] tensor (a bias Add / scale Mul an exporter left behind a convolution, in-graph pixel normalisation) is
    // one multiply-add per element however many nodes spell it: consecutive ones compose into a single AffineChannel
    // pass, fold into the convolution that produced the tensor, and the Dense fold above still finds them.
    // (a divisor whose reciprocal is no normal f32 -- zero, a subnormal, anything above 2^126 -- stays a division: x * (1 / c) would be
    // x * inf, or x times a reciprocal that has lost bits)
    const bool reciprocal_ok = op != '/' || const_left || std::all_of(cf32(n, cst).begin(), cf32(n, cst).end(), [](float c) { return std::isnormal(c) && std::isnormal(1.0f / c); });
    if (act_shape.size() >= 2 && (op == '+' || op == '-' || op == '*' || (op == '/' && !const_left && reciprocal_ok))) {
      const std::vector<float> cv = broadcast_const(n, cst, act_shape);
      const size_t C = size_t(act_shape[1]), S = size_t(prod(act_shape, 2));
      bool per_channel = cv.size() == C * S;
      for (size_t c = 0; per_channel && c < C; c++)
        for (size_t q = 1; q < S; q++)
          if (cv[c * S + q] != cv[c * S]) { per_channel = false; break; }
      if (per_channel) {
        std::vector<double> sc(C, 1.0), sh(C, 0.0);
        for (size_t k = 0; k < C; k++) {
          const double c = cv[k * S];
          if (op == '+') sh[k] = c;
          else if (op == '-') { sc[k] = const_left ? -1.0 : 1.0; sh[k] = const_left ? c : -c; }
          else if (op == '*') sc[k] = c;
          else sc[k] = 1.0 / c;
        }
        const std::string label = node_label(n);
        Step *p = fusable_producer(n, const_left ? 1 : 0);
        if (p && p->kind == StepKind::AffineChannel && p->act == Act::None && size_t(p->S) == S && size_t(p->C) == C) {
          for (size_t k = 0; k < C; k++) {
            p->shift[k] = float(sc[k] * double(p->shift[k]) + sh[k]);
            p->scale[k] = float(sc[k] * double(p->scale[k]));
          }
          p->origin += "+" + label;
          set_act(n, act.buf, act_shape, true);
          return;
        }
        if (p && p->kind == StepKind::SpatialNorm && p->act == Act::None && size_t(p->C) == C && size_t(p->S) == S) {  // into gamma and beta
          for (size_t k = 0; k < C; k++) {
            p->shift[k] = float(sc[k] * double(p->shift[k]) + sh[k]);
            p->scale[k] = float(sc[k] * double(p->scale[k]));
          }
          p->origin += "+" + label;
          set_act(n, act.buf, act_shape, true);
          return;
        }
        if (p && p->kind == StepKind::ChannelNorm && p->act == Act::None && size_t(p->C) == C && size_t(p->S) == S) {  // into gamma and beta (beta may be absent)
          const bool shifts = !p->shift.empty() || std::any_of(sh.begin(), sh.end(), [](double v) { return v != 0.0; });
          if (shifts && p->shift.empty()) p->shift.assign(C, 0.f);
          for (size_t k = 0; k < C; k++) {
            if (shifts) p->shift[k] = float(sc[k] * double(p->shift[k]) + sh[k]);
            p->scale[k] = float(sc[k] * double(p->scale[k]));
          }
          p->origin += "+" + label;
          set_act(n, act.buf, act_shape, true);
          return;
        }
        if (p && p->kind == StepKind::ConvTranspose2d && p->act == Act::None && size_t(p->Mo) == C) {
          convt_fold_affine(*p, sc, sh, label);
          set_act(n, act.buf, act_shape, true);
          return;
        }
        if (p && p->kind == StepKind::Conv2d && p->act == Act::None && size_t(p->Mo) == C) {  // into the conv's weights and bias
          const size_t per_m = size_t(p->K);
          for (size_t mo = 0; mo < C; mo++)
            for (size_t k = 0; k < per_m; k++) p->W[mo * per_m + k] = float(sc[mo] * double(p->W[mo * per_m + k]));
          if (p->bias.empty()) p->bias.assign(C, 0.f);
          for (size_t mo = 0; mo < C; mo++) p->bias[mo] = float(sc[mo] * double(p->bias[mo]) + sh[mo]);
          p->origin += "+" + label;
          set_act(n, act.buf, act_shape, true);
          return;
        }
        Step a;
        a.kind = StepKind::AffineChannel;
        a.in0 = act.buf;
        a.C = int64_t(C);
        a.S = int64_t(S);
        a.scale.resize(C);
        a.shift.resize(C);
        for (size_t k = 0; k < C; k++) {
          a.scale[k] = float(sc[k]);
          a.shift[k] = float(sh[k]);
        }
        emit(std::move(a), n, act_shape);
        return;
      }
    }
    Step s;
    s.kind = StepKind::BinaryConst;
    s.in0 = act.buf;
    s.bop = op;
    s.const_left = const_left;
    s.cst = broadcast_const(n, cst, act_shape);
    const int src = act.buf;
    const Step &e = emit(std::move(s), n, act_shape);
    if (int_bufs.count(src) && (op == '+' || op == '-' || op == '*') &&
        std::all_of(e.cst.begin(), e.cst.end(), [](float c) { return c == std::nearbyint(c); }))
      int_bufs.insert(e.out);
  }

  // ---- constant folding of the integer (shape) sub-graphs exporters emit around Reshape ----
  void Lowerer::set_const_i64(const NodeDef &n, std::vector<int64_t> v, std::vector<int64_t> dims) {
    vals[n.outputs[0]] = const_i64(std::move(v), std::move(dims));
  }
  void Lowerer::fold_int_binary(const NodeDef &n, char op, const Val &a, const Val &b) {
    const auto &x = a.c->i64, &y = b.c->i64;
    if (x.size() != y.size() && x.size() != 1 && y.size() != 1) unsupported(n, "integer folding needs equal sizes or a scalar");
    std::vector<int64_t> o(std::max(x.size(), y.size()));
    for (size_t i = 0; i < o.size(); i++) {
      const int64_t u = x[x.size() == 1 ? 0 : i], v = y[y.size() == 1 ? 0 : i];
      if (op == '/' && v == 0) unsupported(n, "integer division by zero");
      o[i] = op == '+' ? u + v : op == '-' ? u - v : op == '*' ? u * v : op == '/' ? u / v : op == 'm' ? std::min(u, v) : std::max(u, v);
    }
    set_const_i64(n, o, x.size() >= y.size() ? a.shape : b.shape);
  }
  void Lowerer::shape_op(const NodeDef &n) {
    const Val &a = get(n, 0);
    std::vector<int64_t> d = a.shape;
    // the symbolic row count is carried as 0, which Reshape reads as "copy this dim from the input"
    if (!a.is_const && !d.empty() && d[size_t(a.ra)] < 0) d[size_t(a.ra)] = 0;
    int64_t r = int64_t(d.size()), st = n.attr_i("start", 0), en = n.attr_i("end", r);
    if (st < 0) st += r;
    if (en < 0) en += r;
    st = std::clamp<int64_t>(st, 0, r);
    en = std::clamp<int64_t>(en, st, r);
    std::vector<int64_t> o(d.begin() + st, d.begin() + en);
    const int64_t cnt = int64_t(o.size());
    set_const_i64(n, std::move(o), {cnt});
  }
  std::vector<int64_t> Lowerer::const_ints(const NodeDef &n, size_t i, const char *what) {
    const Val &v = get(n, i);
    if (!v.is_const || v.c->dtype != onnx::kInt64) unsupported(n, std::string(what) + " must be a constant integer tensor");
    return v.c->i64;
  }
  void Lowerer::gather(const NodeDef &n) {
    const Val &d = get(n, 0);
    const Val &ix = get(n, 1);
    // column pick out of a [rows, K] activation (the probability of one class, a feature subset): a contiguous range
    if (!d.is_const && d.shape.size() == 2 && ix.is_const && ix.c->dtype == onnx::kInt64 && !ix.c->i64.empty() && ix.shape.size() <= 1) {
      int64_t axis = n.attr_i("axis", 0);
      if (axis < 0) axis += 2;
      if (axis != 1) unsupported(n, "only axis 1 keeps rows independent");
      std::vector<int64_t> v = ix.c->i64;
      for (auto &i : v)
        if (i < 0) i += d.shape[1];
      for (size_t i = 1; i < v.size(); i++)
        if (v[i] != v[0] + int64_t(i)) unsupported(n, "only a contiguous column range");
      if (v[0] < 0 || v[0] + int64_t(v.size()) > d.shape[1]) unsupported(n, "column index out of range");
      const Val src = d;
      emit_slice_cols(node_label(n), src, v[0], v[0] + int64_t(v.size()), n.outputs[0]);
      if (ix.shape.empty()) {  // scalar index: the axis disappears ([rows] instead of [rows, 1])
        Val &o = vals[n.outputs[0]];
        o.shape = {src.shape[0]};
      }
      return;
    }
    // one time step of a [rows, T, C] (or time-major [T, rows, C]) activation: a contiguous range of every row
    if (!d.is_const && time_steppable(d) && ix.is_const && ix.c->dtype == onnx::kInt64 && ix.c->i64.size() == 1 && ix.shape.size() <= 1) {
      int64_t axis = n.attr_i("axis", 0);
      if (axis < 0) axis += 3;
      if (axis != 1 - d.ra) unsupported(n, "only one step of the time axis (axis " + std::to_string(1 - d.ra) + ") keeps rows independent");
      const Val src = d;
      return time_step(n, src, ix.c->i64[0], ix.shape.empty());
    }
    if (!d.is_const && d.ra != 0) unsupported(n, "only one step of the time axis of a [T, rows, C] activation");
    if (!d.is_const || !ix.is_const || ix.c->dtype != onnx::kInt64) unsupported(n, "only constant data with constant indices is folded");
    if (d.shape.size() > 1 || n.attr_i("axis", 0) != 0) unsupported(n, "only 1-D data / axis 0");
    const int64_t len = d.c->dtype == onnx::kInt64 ? int64_t(d.c->i64.size()) : int64_t(d.c->f32.size());
    auto at = [&](int64_t i) {
      if (i < 0) i += len;
      if (i < 0 || i >= len) unsupported(n, "index out of range");
      return size_t(i);
    };
    if (d.c->dtype == onnx::kInt64) {
      std::vector<int64_t> o;
      for (auto i : ix.c->i64) o.push_back(d.c->i64[at(i)]);
      set_const_i64(n, std::move(o), ix.shape);
    } else {
      std::vector<float> o;
      for (auto i : ix.c->i64) o.push_back(d.c->f32[at(i)]);
      vals[n.outputs[0]] = const_f32(std::move(o), ix.shape);
    }
  }
  // May one time step be cut out of `a` as a contiguous column range?  Only a rank-3 value [rows, T, C] / [T, rows, C] whose buffer is
  // registered as a flat [rows, per_row] matrix: what a recurrent step writes, or a Reshape of a flat table.  Every other rank-3 activation
  // (Conv1d tensors, which may live in the channel-quad layout) keeps the channel-slice path and its layout rules.
  bool Lowerer::time_steppable(const Val &a) const {
    return !a.is_const && a.buf >= 0 && a.shape.size() == 3 && a.ra <= 1 && plan.buf_shape[size_t(a.buf)].size() == 2;
  }
  // Step `t` of the time axis of a rank-3 activation `a` (rows first or time-major) as output 0 of n: a SliceCols of C columns, or -- the
  // schedule fold -- nothing at all when `a` is the whole forward Y of a unidirectional recurrent step that nothing else reads and t is
  // the last step: that step then stores Y_h (H values per row, not T * H).  drop_axis: the time axis disappears (a scalar Gather index)
  void Lowerer::time_step(const NodeDef &n, const Val &a, int64_t t, bool drop_axis) {
    const int64_t T = a.shape[size_t(1 - a.ra)], C = a.shape[2], N = a.shape[size_t(a.ra)];
    if (t < 0) t += T;
    if (t < 0 || t >= T) unsupported(n, "time step out of range");
    Val v;
    v.ra = drop_axis ? 0 : a.ra;
    v.shape = drop_axis ? std::vector<int64_t>{N, C} : a.ra ? std::vector<int64_t>{1, N, C} : std::vector<int64_t>{N, 1, C};
    auto pit = producer.find(a.buf);
    Step *p = pit == producer.end() ? nullptr : &plan.steps[size_t(pit->second)];
    if (p && p->kind == StepKind::Recurrent && p->out == a.buf && p->out_mode == kRnnY && p->rnn->D == 1 && !p->rnn->reverse && t == T - 1 &&
        C == p->rnn->H && live_uses(a.buf) == 1 && p->in3 < 0) {  // (with sequence_lens Y[T - 1] is 0 for a short row, not its Y_h)
      p->out_mode = kRnnYh;
      p->origin += "+" + node_label(n);
      plan.buf_per_row[size_t(a.buf)] = C;
      plan.buf_shape[size_t(a.buf)] = {N, C};
      v.buf = a.buf;
      alias_edges[v.buf]++;
    } else {
      Step s;
      s.kind = StepKind::SliceCols;
      s.in0 = a.buf;
      s.col_off = t * C;
      s.K = C;
      s.origin = node_label(n);
      v.buf = push_step(std::move(s), {N, C});
    }
    vals[n.outputs[0]] = v;
    buf_names[v.buf].push_back(n.outputs[0]);
  }
  // feature-axis slice of a [rows, K] activation: out = in[:, b:e]
  // ... or a channel range of an [N,C,H,W] activation: channels [b, e) are one contiguous block of every sample, in
  // NCHW and (whole quads) in the channel-quad layout alike
  void Lowerer::emit_slice_cols(const std::string &origin, const Val &a, int64_t b, int64_t e, const std::string &out_name) {
    const int64_t inner = prod(a.shape, 2);
    std::vector<int64_t> oshape = a.shape;
    oshape[1] = e - b;
    Step s;
    s.kind = StepKind::SliceCols;
    s.in0 = a.buf;
    s.col_off = b * inner;
    s.K = (e - b) * inner;
    s.origin = origin;
    Val v;
    v.buf = push_step(std::move(s), oshape);
    v.shape = oshape;
    vals[out_name] = v;
    buf_names[v.buf].push_back(out_name);
  }
  void Lowerer::split(const NodeDef &n) {
    const Val &a = get(n, 0);
    if (a.is_const || a.shape.size() < 2) unsupported(n, "only [rows, K] or [N,C,...] activations");
    int64_t axis = n.attr_i("axis", 0);
    if (axis < 0) axis += int64_t(a.shape.size());
    if (axis != 1) unsupported(n, "only axis 1 keeps rows independent");
    std::vector<int64_t> sizes;
    if (has_input(n, 1)) sizes = const_ints(n, 1, "split");
    else if (auto *p = n.attr_ints("split")) sizes = *p;
    const int64_t K = a.shape[1], nout = int64_t(n.outputs.size());
    if (sizes.empty()) {
      const int64_t parts = n.attr_i("num_outputs", nout), each = (K + parts - 1) / parts;
      for (int64_t i = 0; i < parts; i++) sizes.push_back(std::min(each, K - i * each));
    }
    if (int64_t(sizes.size()) != nout || std::accumulate(sizes.begin(), sizes.end(), int64_t(0)) != K) unsupported(n, "split sizes do not cover the axis");
    const Val src = a;  // `a` may dangle once vals grows
    int64_t off = 0;
    for (int64_t i = 0; i < nout; i++) {
      if (sizes[size_t(i)] <= 0) unsupported(n, "empty split piece");
      if (!n.outputs[size_t(i)].empty() && uses.count(n.outputs[size_t(i)])) emit_slice_cols(node_label(n), src, off, off + sizes[size_t(i)], n.outputs[size_t(i)]);
      off += sizes[size_t(i)];
    }
  }
  void Lowerer::slice(const NodeDef &n) {
    const Val &d = get(n, 0);
    if (!d.is_const && d.shape.size() >= 2) {  // activation: feature / channel axis slice with step 1
      std::vector<int64_t> st, en, ax, sp;
      if (has_input(n, 1)) {
        st = const_ints(n, 1, "starts");
        en = const_ints(n, 2, "ends");
        if (has_input(n, 3)) ax = const_ints(n, 3, "axes");
        if (has_input(n, 4)) sp = const_ints(n, 4, "steps");
      } else {
        if (auto *p = n.attr_ints("starts")) st = *p;
        if (auto *p = n.attr_ints("ends")) en = *p;
        if (auto *p = n.attr_ints("axes")) ax = *p;
      }
      if (st.size() != 1 || en.size() != 1 || ax.size() > 1 || (!sp.empty() && sp[0] != 1)) unsupported(n, "one axis, step 1");
      const int64_t axis = ax.empty() ? 0 : (ax[0] < 0 ? ax[0] + int64_t(d.shape.size()) : ax[0]);
      const int64_t time_axis = time_steppable(d) ? 1 - d.ra : -1;
      if (d.ra != 0 && axis != time_axis) unsupported(n, "only one step of the time axis of a [T, rows, C] activation");
      if (axis != 1 && d.ra == 0) unsupported(n, "only axis 1 (features / channels)");
      const int64_t K = d.shape[size_t(axis)];
      int64_t b = st[0] < 0 ? st[0] + K : st[0], e = en[0] < 0 ? en[0] + K : en[0];
      b = std::clamp<int64_t>(b, 0, K);
      e = std::clamp<int64_t>(e, b, K);
      if (e == b) unsupported(n, "empty slice");
      const Val src = d;
      if (axis == time_axis && e - b == 1) return time_step(n, src, b, false);  // (the last step of a recurrent layer's Y: folded)
      if (d.ra != 0) unsupported(n, "only one step of the time axis of a [T, rows, C] activation");
      emit_slice_cols(node_label(n), src, b, e, n.outputs[0]);
      return;
    }
    if (!d.is_const || d.c->dtype != onnx::kInt64 || d.shape.size() != 1) unsupported(n, "only 1-D constant integer data is folded");
    std::vector<int64_t> st, en, ax, sp;
    if (has_input(n, 1)) {
      st = const_ints(n, 1, "starts");
      en = const_ints(n, 2, "ends");
      if (has_input(n, 3)) ax = const_ints(n, 3, "axes");
      if (has_input(n, 4)) sp = const_ints(n, 4, "steps");
    } else {
      if (auto *p = n.attr_ints("starts")) st = *p;
      if (auto *p = n.attr_ints("ends")) en = *p;
    }
    if (st.size() != 1 || en.size() != 1 || (!ax.empty() && ax[0] != 0 && ax[0] != -1)) unsupported(n, "one axis only");
    const int64_t len = int64_t(d.c->i64.size()), step = sp.empty() ? 1 : sp[0];
    if (step != 1) unsupported(n, "step must be 1");
    int64_t b = st[0] < 0 ? st[0] + len : st[0], e = en[0] < 0 ? en[0] + len : en[0];
    b = std::clamp<int64_t>(b, 0, len);
    e = std::clamp<int64_t>(e, b, len);
    std::vector<int64_t> o(d.c->i64.begin() + b, d.c->i64.begin() + e);
    const int64_t cnt = int64_t(o.size());
    set_const_i64(n, std::move(o), {cnt});
  }
  void Lowerer::cast(const NodeDef &n) {
    const Val &a = get(n, 0);
    const int64_t to = n.attr_i("to", onnx::kFloat);
    const bool to_int = to == onnx::kInt64 || to == onnx::kInt32, to_h = to == onnx::kFloat16, to_f = to == onnx::kFloat || to == onnx::kDouble || to_h;
    if (!to_int && !to_f) unsupported(n, "only casts to f32/f64/f16/int32/int64");
    if (a.is_const) {
      if (a.c->dtype == onnx::kFloat && to_f) {  // between float types: the same values, rounded when the target is float16
        auto t = std::make_shared<TensorData>(*a.c);
        t->elem = to_h ? onnx::kFloat16 : onnx::kFloat;
        if (to_h)
          for (float &f : t->f32) f = onnx::round_to_half(f);
        vals[n.outputs[0]] = const_val(std::move(t));
        return;
      }
      if ((a.c->dtype == onnx::kInt64) == to_int) { vals[n.outputs[0]] = a; return; }
      if (to_int) {
        std::vector<int64_t> o;
        for (float f : a.c->f32) o.push_back(int64_t(f));
        set_const_i64(n, std::move(o), a.shape);
      } else {
        std::vector<float> o;
        for (int64_t i : a.c->i64) o.push_back(to_h ? onnx::round_to_half(float(i)) : float(i));
        vals[n.outputs[0]] = const_f32(std::move(o), a.shape);
        if (to_h) vals[n.outputs[0]].c->elem = onnx::kFloat16;
      }
      return;
    }
    if (to_h) {  // an activation becomes float16: one rounding (none when it is half already)
      if (a.half) { alias(n, a.shape); mark_half(n.outputs[0]); return; }
      if (a.ra != 0) bad_form(n, "a cast of a time-major value to float16");
      Step s;
      s.kind = StepKind::RoundHalf;
      s.in0 = a.buf;
      std::vector<int64_t> shape = a.shape;
      emit(std::move(s), n, shape);
      mark_half(n.outputs[0]);
      return;
    }
    if (a.half && to_f) {
      // float16 -> float: the same values under a float name.  Float operators behind it must not fuse into the step that made the half
      // value (its result is rounded first), so the buffer forgets its producer
      const int buf = a.buf;
      alias(n, a.shape);
      producer.erase(buf);
      return;
    }
    // activations are always f32 here: a float cast is an alias, an integer cast truncates toward zero and
    // the values stay in f32 storage (the C ABI returns f32, rust.h:28-49)
    if (to_f || int_bufs.count(a.buf)) { alias(n, a.shape); return; }  // (already whole numbers: ArgMax labels and the like)
    Step s;
    s.kind = StepKind::Unary;
    s.in0 = a.buf;
    s.act = Act::Trunc;
    std::vector<int64_t> shape = a.shape;
    int_bufs.insert(emit(std::move(s), n, shape).out);
  }
  void Lowerer::concat(const NodeDef &n) {
    if (n.inputs.empty()) unsupported(n, "no inputs");
    bool all_const = true;
    for (size_t i = 0; i < n.inputs.size(); i++) all_const = all_const && get(n, i).is_const;
    if (all_const) {
      std::vector<int64_t> o;
      for (size_t i = 0; i < n.inputs.size(); i++) {
        const Val &v = get(n, i);
        if (v.c->dtype != onnx::kInt64 || v.shape.size() > 1) unsupported(n, "only 1-D integer constants are folded");
        o.insert(o.end(), v.c->i64.begin(), v.c->i64.end());
      }
      const int64_t cnt = int64_t(o.size());
      set_const_i64(n, std::move(o), {cnt});
      return;
    }
    if (tokens_concat(n)) return;
    const Val &first = get(n, 0);
    if (first.is_const) unsupported(n, "mixing constants and activations");
    const int64_t rank = int64_t(first.shape.size());
    int64_t axis = n.attr_i("axis", 1);
    if (axis < 0) axis += rank;
    if (axis != 1) unsupported(n, "only axis 1 (features / channels) is supported");
    std::vector<int64_t> out_shape = first.shape;
    out_shape[1] = 0;
    for (size_t i = 0; i < n.inputs.size(); i++) {
      const Val &v = get(n, i);
      if (v.is_const) unsupported(n, "mixing constants and activations");
      if (v.shape.size() != first.shape.size()) unsupported(n, "rank mismatch");
      for (size_t d = 0; d < v.shape.size(); d++)
        if (d != 1 && v.shape[d] != first.shape[d]) unsupported(n, "shape mismatch " + shape_str(v.shape) + " vs " + shape_str(first.shape));
      out_shape[1] += v.shape[1];
    }
    const int out = new_buf(out_shape);
    int64_t off = 0;
    for (size_t i = 0; i < n.inputs.size(); i++) {
      const Val &v = get(n, i);
      Step s;
      s.kind = StepKind::CopyCols;
      s.in0 = v.buf;
      s.out = out;
      s.col_off = off;
      s.origin = n.op + (n.name.empty() ? "" : ":" + n.name) + "[" + std::to_string(i) + "]";
      off += prod(v.shape, 1);
      plan.steps.push_back(std::move(s));
    }
    producer[out] = int(plan.steps.size()) - 1;
    set_act(n, out, out_shape);
  }
  void Lowerer::reduce_mean(const NodeDef &n) {
    const Val &a = get(n, 0);
    if (!a.is_const && a.shape.size() == 2) {
      const Val x = a;
      if (decomposed_layer_norm(n, x)) return;
      return row_reduce(n);
    }
    if (!a.is_const && a.shape.size() == 4) {
      const Val x = a;
      if (channels_first_norm(n, x)) return;
    }
    if (a.is_const || a.shape.size() < 3) unsupported(n, "only spatial means of [N,C,...] activations");
    std::vector<int64_t> axes;
    if (has_input(n, 1)) axes = const_ints(n, 1, "axes");
    else if (auto *p = n.attr_ints("axes")) axes = *p;
    const int64_t rank = int64_t(a.shape.size());
    std::vector<bool> red(size_t(rank), false);
    for (auto ax : axes) {
      const int64_t na = ax < 0 ? ax + rank : ax;
      if (na < 0 || na >= rank) unsupported(n, "axis " + std::to_string(ax) + " is out of range for rank " + std::to_string(rank));
      red[size_t(na)] = true;
    }
    if (rank == 3 && a.ra == 0 && red[1] && !red[0] && !red[2]) {  // the mean over the time axis of a window [rows, T, E] -> [rows, E]
      Step s;
      s.kind = StepKind::MeanTime;
      s.in0 = a.buf;
      s.rep = a.shape[1];
      s.K = a.shape[2];
      const int64_t N = a.shape[0], E = a.shape[2];
      if (n.attr_i("keepdims", 1) != 0) emit_window(std::move(s), n, {N, 1, E});
      else emit(std::move(s), n, {N, E});
      return;
    }
    for (int64_t i = 0; i < rank; i++)
      if (red[size_t(i)] != (i >= 2)) unsupported(n, "axes must be exactly the spatial axes");
    Step s;
    s.kind = StepKind::GlobalAvgPool;
    s.in0 = a.buf;
    s.C = a.shape[1];
    s.S = prod(a.shape, 2);
    std::vector<int64_t> shape = {a.shape[0], a.shape[1]};
    if (n.attr_i("keepdims", 1) != 0)
      for (int64_t i = 2; i < rank; i++) shape.push_back(1);
    emit(std::move(s), n, shape);
  }
  // The Reduce* family over the last axis of [rows, F] or of a window [rows, T, E]: one RowReduce step (hip/reduce.hip)
  void Lowerer::row_reduce(const NodeDef &n) {
    static const std::map<std::string, int> ops = {{"ReduceSum", kReduceSum}, {"ReduceMean", kReduceMean}, {"ReduceMax", kReduceMax}, {"ReduceMin", kReduceMin},
                                                   {"ReduceProd", kReduceProd}, {"ReduceL1", kReduceL1}, {"ReduceL2", kReduceL2},
                                                   {"ReduceSumSquare", kReduceSumSquare}, {"ReduceLogSum", kReduceLogSum}, {"ReduceLogSumExp", kReduceLogSumExp}};
    const Val a = get(n, 0);
    const int64_t rank = int64_t(a.shape.size());
    if (a.is_const || a.ra != 0 || (rank != 2 && rank != 3)) bad_form(n, "the input must be a [rows, F] or [rows, T, E] activation, got " + shape_str(a.shape));
    std::vector<int64_t> axes;
    if (has_input(n, 1)) axes = const_ints(n, 1, "axes");
    else if (auto *p = n.attr_ints("axes")) axes = *p;
    if (n.attr_i("noop_with_empty_axes", 0) != 0) bad_form(n, "noop_with_empty_axes = 1");
    if (axes.empty()) bad_form(n, "empty axes reduce over every axis, the row axis included");
    if (axes.size() != 1 || (axes[0] != -1 && axes[0] != rank - 1))
      bad_form(n, "only the last axis of " + shape_str(a.shape) + " is reduced (the other axes mix rows or need a transpose)");
    const int64_t E = a.shape.back();
    if (E < 1 || E > kReduceMaxE) bad_form(n, "F = " + std::to_string(E) + " elements per reduced vector, above the cap of " + std::to_string(kReduceMaxE));
    Step s;
    s.kind = StepKind::RowReduce;
    s.in0 = a.buf;
    s.K = E;
    s.rep = prod(a.shape, 1) / E;
    s.out_mode = ops.at(n.op);
    std::vector<int64_t> shape(a.shape.begin(), a.shape.end() - 1);
    if (n.attr_i("keepdims", 1) != 0) shape.push_back(1);
    if (shape.size() == 3) emit_window(std::move(s), n, shape);
    else emit(std::move(s), n, shape);
  }
  // ArgMin: the twin of ArgMax
  void Lowerer::argmin(const NodeDef &n) {
    const Val &a = get(n, 0);
    if (a.is_const || a.shape.size() != 2) unsupported(n, "only [rows, K] activations");
    int64_t axis = n.attr_i("axis", 0);
    if (axis < 0) axis += 2;
    if (axis != 1) unsupported(n, "only axis 1 keeps rows independent");
    if (n.attr_i("select_last_index", 0) != 0) unsupported(n, "select_last_index=1");
    Step s;
    s.kind = StepKind::ArgMin;
    s.in0 = a.buf;
    s.K = a.shape[1];
    std::vector<int64_t> shape = {a.shape[0]};
    if (n.attr_i("keepdims", 1) != 0) shape.push_back(1);
    int_bufs.insert(emit(std::move(s), n, shape).out);
  }
  // k of a TopK node (a constant input from opset 10 on, an attribute before); -1: not a constant
  int64_t Lowerer::topk_k(const NodeDef &n) {
    if (has_input(n, 1)) {
      const Val *v = find_value(n.inputs[1]);
      return v && v->is_const && v->c->dtype == onnx::kInt64 && v->c->i64.size() == 1 ? v->c->i64[0] : -1;
    }
    return n.attr_i("k", -1);
  }
  // binds output o of n to a new buffer written by step s
  int Lowerer::bind_output(const NodeDef &n, size_t o, Step s, const std::vector<int64_t> &shape, bool whole) {
    Val v;
    v.buf = push_step(std::move(s), shape);
    v.shape = shape;
    vals[n.outputs[o]] = v;
    buf_names[v.buf].push_back(n.outputs[o]);
    if (whole) int_bufs.insert(v.buf);
    return v.buf;
  }
  // TopK over the last axis of [rows, M]: one step per output that is read (Values, Indices as f32 values)
  void Lowerer::topk(const NodeDef &n) {
    const Val a = get(n, 0);
    if (a.is_const || a.shape.size() != 2 || a.ra != 0) bad_form(n, "the input must be a [rows, M] activation, got " + shape_str(a.shape));
    int64_t axis = n.attr_i("axis", -1);
    if (axis < 0) axis += 2;
    if (axis != 1) bad_form(n, "only the last axis keeps rows independent, got axis " + std::to_string(n.attr_i("axis", -1)));
    const int64_t k = topk_k(n), M = a.shape[1];
    if (k < 0) bad_form(n, "k must be a constant");
    if (k < 1 || k > kNearestMaxK) bad_form(n, "k = " + std::to_string(k) + " is outside 1 .. " + std::to_string(kNearestMaxK));
    if (k > M) bad_form(n, "k = " + std::to_string(k) + " is above the row length M = " + std::to_string(M));
    for (size_t o = 0; o < 2; o++) {
      if (!wanted(n, o)) continue;
      Step s;
      s.kind = StepKind::TopK;
      s.in0 = a.buf;
      s.K = M;
      s.M = k;
      s.is_max = n.attr_i("largest", 1) != 0;
      s.out_mode = int(o);
      s.origin = node_label(n);
      bind_output(n, o, std::move(s), {a.shape[0], k}, o == 1);
    }
  }

  void Lowerer::argmax(const NodeDef &n) {
    const Val &a = get(n, 0);
    if (a.is_const || a.shape.size() != 2) unsupported(n, "only [rows, classes] activations");
    int64_t axis = n.attr_i("axis", 0);
    if (axis < 0) axis += 2;
    if (axis != 1) unsupported(n, "only axis 1 keeps rows independent");
    if (n.attr_i("select_last_index", 0) != 0) unsupported(n, "select_last_index=1");
    Step s;
    s.kind = StepKind::ArgMax;
    s.in0 = a.buf;
    s.K = a.shape[1];
    std::vector<int64_t> shape = {a.shape[0]};
    if (n.attr_i("keepdims", 1) != 0) shape.push_back(1);
    int_bufs.insert(emit(std::move(s), n, shape).out);
  }

  void Lowerer::unary(const NodeDef &n) {
    Act act;
    float pa = 0.f, pb = 0.f;
    static const std::map<std::string, Act> simple = {
        {"Relu", Act::Relu}, {"Sigmoid", Act::Sigmoid}, {"Tanh", Act::Tanh}, {"Exp", Act::Exp}, {"Log", Act::Log},
        {"Sqrt", Act::Sqrt}, {"Neg", Act::Neg}, {"Abs", Act::Abs}, {"Softplus", Act::Softplus}, {"HardSwish", Act::HardSwish},
        {"Erf", Act::Erf}, {"Reciprocal", Act::Reciprocal}, {"Floor", Act::Floor}, {"Ceil", Act::Ceil},
        {"Softsign", Act::Softsign}, {"Round", Act::Round}};
    auto si = simple.find(n.op);
    if (si != simple.end()) act = si->second;
    else if (n.op == "LeakyRelu") { act = Act::LeakyRelu; pa = n.attr_f("alpha", 0.01f); }
    else if (n.op == "Elu") { act = Act::Elu; pa = n.attr_f("alpha", 1.0f); }
    else if (n.op == "Selu") { act = Act::Selu; pa = n.attr_f("alpha", 1.67326319217681884765625f); pb = n.attr_f("gamma", 1.05070102214813232421875f); }
    else if (n.op == "HardSigmoid") { act = Act::HardSigmoid; pa = n.attr_f("alpha", 0.2f); pb = n.attr_f("beta", 0.5f); }
    else if (n.op == "Gelu") {
      if (n.attr_s("approximate", "none") != "none") unsupported(n, "only the exact (erf) form");
      act = Act::Gelu;
    }
    else {  // Clip
      act = Act::Clip;
      pa = -INFINITY;
      pb = INFINITY;
      if (auto *a = n.attr("min")) pa = a->f;
      if (auto *a = n.attr("max")) pb = a->f;
      if (has_input(n, 1)) { const Val &v = get(n, 1); if (cf32(n, v).size() != 1) unsupported(n, "min must be a scalar constant"); pa = v.c->f32[0]; }
      if (has_input(n, 2)) { const Val &v = get(n, 2); if (cf32(n, v).size() != 1) unsupported(n, "max must be a scalar constant"); pb = v.c->f32[0]; }
    }
    apply_unary(n, 0, act, pa, pb, n.op);
  }
  // activation `act` on input `idx` of node n: into the epilogue of the step that produced it when that step takes one
  // and nothing else reads the value, else an elementwise pass
  void Lowerer::apply_unary(const NodeDef &n, size_t idx, Act act, float pa, float pb, const std::string &label) {
    const Val &a = get(n, idx);
    if (a.is_const) unsupported(n, "activation of a constant");
    std::vector<int64_t> shape = a.shape;
    if (Step *p = fusable_producer(n, idx)) {
      const bool mfma_step = p->kind == StepKind::Dense || p->kind == StepKind::Conv2d;
      const bool takes_act = p->kind == StepKind::Dense || p->kind == StepKind::Conv2d || p->kind == StepKind::AffineChannel ||
                             p->kind == StepKind::BinaryConst || p->kind == StepKind::BinaryAct;
      const bool qdense_act = quantised_layer(*p) && !p->qy.on && (act == Act::Relu || act == Act::Clip);  // on `real`, before the requantisation
      const bool hdense_act = p->kind == StepKind::HDense && cur_half && int(act) >= 1 && int(act) <= kMaxMfmaFusedAct;  // r = half(act(float(r)))
      const bool convt_act = p->kind == StepKind::ConvTranspose2d && int(act) >= 1 && int(act) <= kMaxMfmaFusedAct;  // kinds 1..5 in its epilogue
      const bool norm_act = (p->kind == StepKind::SpatialNorm || p->kind == StepKind::ChannelNorm) && mfma_fusable(act);  // the kinds the convolution epilogues take
      if (p->act == Act::None && (takes_act || qdense_act || hdense_act || convt_act || norm_act) && (!mfma_step || mfma_fusable(act))) {
        p->act = act;
        p->act_a = pa;
        p->act_b = pb;
        p->origin += "+" + label;
        set_act(n, a.buf, shape, true);
        return;
      }
    }
    Step s;
    s.kind = StepKind::Unary;
    s.in0 = a.buf;
    s.act = act;
    s.act_a = pa;
    s.act_b = pb;
    emit(std::move(s), n, shape);
  }

  void Lowerer::alias(const NodeDef &n, const std::vector<int64_t> &new_shape) {
    const Val &a = get_raw(n, 0);
    if (prod(new_shape, 1) != prod(a.shape, 1) || new_shape.empty() || new_shape[0] != a.shape[0])
      unsupported(n, "reshape " + shape_str(a.shape) + " -> " + shape_str(new_shape) + " does not preserve the row axis");
    if (a.pv) {  // (a preprocessing-region value: the same columns under another shape)
      Val v = a;
      v.shape = new_shape;
      if (n.op != "Identity") {
        PrepVal p = *a.pv;
        p.add_origin(node_label(n));
        v.pv = std::make_shared<const PrepVal>(std::move(p));
      }
      vals[n.outputs[0]] = v;
      return;
    }
    int buf = a.buf;
    set_act(n, buf, new_shape, true);
  }

  void Lowerer::reshape_like(const NodeDef &n) {
    const Val &a = get_raw(n, 0);
    if (a.is_const) {
      if (n.op == "Identity") { vals[n.outputs[0]] = a; return; }
      if ((n.op == "Unsqueeze" || n.op == "Squeeze") && a.shape.size() <= 1) {  // scalar <-> [1] in shape sub-graphs
        Val v = a;
        auto t = std::make_shared<TensorData>(*a.c);
        t->dims = n.op == "Unsqueeze" ? std::vector<int64_t>{1} : std::vector<int64_t>{};
        if (n.op == "Unsqueeze" && a.shape.size() == 1) unsupported(n, "only scalar constants are unsqueezed");
        v.c = t;
        v.shape = t->dims;
        vals[n.outputs[0]] = v;
        return;
      }
      unsupported(n, "reshaping constants is not supported");
    }
    if (a.ra != 0) return reshape_tagged(n);
    std::vector<int64_t> out;
    const int64_t rank = int64_t(a.shape.size());
    if (n.op == "Identity" || n.op == "Dropout") {
      out = a.shape;
    } else if (n.op == "Flatten") {
      int64_t axis = n.attr_i("axis", 1);
      if (axis < 0) axis += rank;
      if (axis == 2 && rank == 4 && token_view_of_flatten(n, a)) out = {a.shape[0], a.shape[1], prod(a.shape, 2)};
      else if (axis != 1) unsupported(n, "only axis=1 keeps the row axis");
      else out = {a.shape[0], prod(a.shape, 1)};
    } else if (n.op == "Reshape") {
      std::vector<int64_t> tgt;
      if (has_input(n, 1)) {
        const Val &s = get(n, 1);
        if (!s.is_const || s.c->dtype != onnx::kInt64) unsupported(n, "shape must be a constant int64 tensor");
        tgt = s.c->i64;
      } else if (auto *p = n.attr_ints("shape")) tgt = *p;
      else unsupported(n, "missing shape");
      if (tgt.empty()) unsupported(n, "empty target shape");
      int64_t per_row = prod(a.shape, 1);
      // leading entry must denote the row axis: 0 (copy), the fixed batch, or -1 with the rest complete
      int64_t rest = 1;
      int neg = -1;
      for (size_t i = 1; i < tgt.size(); i++) {
        int64_t d = tgt[i];
        if (d == 0) { if (i >= a.shape.size()) unsupported(n, "0 entry out of range"); d = a.shape[i]; tgt[i] = d; }
        if (d == -1) { if (neg >= 0) unsupported(n, "more than one -1"); neg = int(i); continue; }
        rest *= d;
      }
      bool lead_ok = tgt[0] == 0 || (tgt[0] == a.shape[0] && a.shape[0] > 0) || (tgt[0] == -1 && neg < 0 && rest == per_row);
      if (!lead_ok) unsupported(n, "target shape " + shape_str(tgt) + " does not keep the row axis of " + shape_str(a.shape));
      if (neg >= 0) {
        if (rest == 0 || per_row % rest) unsupported(n, "cannot infer -1");
        tgt[size_t(neg)] = per_row / rest;
      }
      tgt[0] = a.shape[0];
      out = tgt;
    } else {  // Squeeze / Unsqueeze
      std::vector<int64_t> axes;
      if (has_input(n, 1)) {
        const Val &s = get(n, 1);
        if (!s.is_const || s.c->dtype != onnx::kInt64) unsupported(n, "axes must be constant");
        axes = s.c->i64;
      } else if (auto *p = n.attr_ints("axes")) axes = *p;
      if (n.op == "Squeeze") {
        for (int64_t i = 0; i < rank; i++) {
          bool drop = axes.empty() ? (a.shape[size_t(i)] == 1 && i != 0) : false;
          for (auto ax : axes) if ((ax < 0 ? ax + rank : ax) == i) drop = true;
          if (drop && i == 0) unsupported(n, "cannot squeeze the row axis");
          if (!drop) out.push_back(a.shape[size_t(i)]);
        }
      } else {
        int64_t nr = rank + int64_t(axes.size());
        size_t src = 0;
        for (int64_t i = 0; i < nr; i++) {
          bool ins = false;
          for (auto ax : axes) if ((ax < 0 ? ax + nr : ax) == i) ins = true;
          if (ins && i == 0) unsupported(n, "cannot insert an axis before the row axis");
          if (!ins && src >= a.shape.size()) unsupported(n, "axes out of range");
          out.push_back(ins ? 1 : a.shape[src++]);
        }
        if (src != a.shape.size()) unsupported(n, "axes out of range");
      }
    }
    alias(n, out);
  }

  // Identity / Squeeze / Unsqueeze / Reshape of a value whose row axis is not axis 0: an alias when the axes in front of the row axis keep
  // their total extent (then the other axes keep their order in the rows-first buffer), else rejected -- it would need data moved
  void Lowerer::reshape_tagged(const NodeDef &n) {
    const Val a = get_raw(n, 0);
    const int64_t rank = int64_t(a.shape.size());
    std::vector<int64_t> out;
    int ra = a.ra;
    auto const_axes = [&]() {
      std::vector<int64_t> axes;
      if (has_input(n, 1)) axes = const_ints(n, 1, "axes");
      else if (auto *p = n.attr_ints("axes")) axes = *p;
      return axes;
    };
    if (n.op == "Identity" || n.op == "Dropout") {
      out = a.shape;
    } else if (n.op == "Squeeze") {
      const std::vector<int64_t> axes = const_axes();
      ra = -1;
      for (int64_t i = 0; i < rank; i++) {
        bool drop = axes.empty() && a.shape[size_t(i)] == 1 && i != a.ra;
        for (auto ax : axes) drop = drop || (ax < 0 ? ax + rank : ax) == i;
        if (drop && i == a.ra) unsupported(n, "cannot squeeze the row axis");
        if (drop && a.shape[size_t(i)] != 1) unsupported(n, "axis " + std::to_string(i) + " of " + shape_str(a.shape) + " is not 1");
        if (i == a.ra) ra = int(out.size());
        if (!drop) out.push_back(a.shape[size_t(i)]);
      }
    } else if (n.op == "Unsqueeze") {
      const std::vector<int64_t> axes = const_axes();
      const int64_t nr = rank + int64_t(axes.size());
      size_t src = 0;
      for (int64_t i = 0; i < nr; i++) {
        bool ins = false;
        for (auto ax : axes) ins = ins || (ax < 0 ? ax + nr : ax) == i;
        if (!ins && src >= a.shape.size()) unsupported(n, "axes out of range");
        if (!ins && int(src) == a.ra) ra = int(i);
        out.push_back(ins ? 1 : a.shape[src++]);
      }
      if (src != a.shape.size()) unsupported(n, "axes out of range");
    } else if (n.op == "Reshape") {
      std::vector<int64_t> tgt = has_input(n, 1) ? const_ints(n, 1, "shape") : n.attr_ints("shape") ? *n.attr_ints("shape") : std::vector<int64_t>{};
      if (tgt.empty()) unsupported(n, "missing shape");
      const int64_t per_row = prod(a.shape, 0) / a.shape[size_t(a.ra)], rows = a.shape[size_t(a.ra)];
      int q = -1, neg = -1;
      for (size_t i = 0; i < tgt.size(); i++) {
        if (tgt[i] == 0) {
          if (i >= a.shape.size()) unsupported(n, "0 entry out of range");
          if (int(i) == a.ra) q = int(i);
          else tgt[i] = a.shape[i];
        } else if (tgt[i] == -1) {
          if (neg >= 0) unsupported(n, "more than one -1");
          neg = int(i);
        } else if (tgt[i] < 0) unsupported(n, "negative extent");
      }
      auto known = [&]() {  // product of the entries that are neither the row axis nor the -1
        int64_t p = 1;
        for (size_t i = 0; i < tgt.size(); i++)
          if (int(i) != q && int(i) != neg) p *= tgt[i];
        return p;
      };
      if (q < 0 && rows > 0) {  // a fixed batch: the entry that equals it behind the same leading extent
        int64_t lead = 1;
        const int64_t pre = prod(a.shape, 0, size_t(a.ra));
        for (size_t i = 0; i < tgt.size() && q < 0; i++) {
          if (lead == pre && tgt[i] == rows) q = int(i);
          else if (tgt[i] > 0) lead *= tgt[i];
        }
      }
      if (q < 0 && rows < 0 && neg >= 0 && known() == per_row) q = neg, neg = -1;  // (the -1 stands for the symbolic row count)
      if (q < 0) unsupported(n, "target shape " + shape_str(tgt) + " does not keep the row axis of " + shape_str(a.shape));
      if (neg >= 0) {
        const int64_t k = known();
        if (k == 0 || per_row % k) unsupported(n, "cannot infer -1");
        tgt[size_t(neg)] = per_row / k;
      }
      tgt[size_t(q)] = rows;
      out = tgt;
      ra = q;
    } else {
      unsupported(n, "on a time-major value (row axis " + std::to_string(a.ra) + " of " + shape_str(a.shape) + ") it would need data moved");
    }
    int64_t rest = 1;
    for (size_t i = 0; i < out.size(); i++)
      if (int(i) != ra) rest *= out[i];
    if (rest != plan.buf_per_row[size_t(a.buf)] || prod(out, 0, size_t(ra)) != prod(a.shape, 0, size_t(a.ra)))
      unsupported(n, "reshape " + shape_str(a.shape) + " -> " + shape_str(out) + " (row axis " + std::to_string(a.ra) + ") would need data moved");
    set_act(n, a.buf, out, true, ra);
  }

  void Lowerer::softmax(const NodeDef &n, bool logsm) {
    const Val &a = get(n, 0);
    if (a.is_const) unsupported(n, "softmax of a constant");
    const int64_t rank = int64_t(a.shape.size());
    int64_t axis = n.attr_i("axis", m.opset >= 13 ? -1 : 1);
    if (axis < 0) axis += rank;
    if (axis < 1 || axis >= rank) unsupported(n, "axis must address a non-row axis");
    Step s;
    s.kind = StepKind::Softmax;
    s.in0 = a.buf;
    s.log_softmax = logsm;
    s.sm_outer = prod(a.shape, 1, size_t(axis));
    if (m.opset >= 13) {
      s.sm_len = a.shape[size_t(axis)];
      s.sm_inner = prod(a.shape, size_t(axis) + 1);
    } else {
      s.sm_len = prod(a.shape, size_t(axis));
      s.sm_inner = 1;
    }
    std::vector<int64_t> shape = a.shape;
    emit(std::move(s), n, shape);
  }

  void Lowerer::spatial(const NodeDef &n, Step &s, int64_t H, int64_t W, const int64_t *extra_pad) {
    s.sh = s.sw = s.dh = s.dw = 1;
    s.pt = s.pl = s.pb = s.pr = 0;
    // (1-D operators run as [N,C,1,L]: one stride / dilation, two pads, all on the W axis)
    if (auto *p = n.attr_ints("strides")) { if (p->size() == 1) s.sw = (*p)[0]; else if (p->size() != 2) unsupported(n, "only 1-D / 2-D"); else { s.sh = (*p)[0]; s.sw = (*p)[1]; } }
    if (auto *p = n.attr_ints("dilations")) { if (p->size() == 1) s.dw = (*p)[0]; else if (p->size() != 2) unsupported(n, "only 1-D / 2-D"); else { s.dh = (*p)[0]; s.dw = (*p)[1]; } }
    if (auto *p = n.attr_ints("pads")) {
      if (p->size() == 2) { s.pl = (*p)[0]; s.pr = (*p)[1]; }
      else if (p->size() != 4) unsupported(n, "only 1-D / 2-D");
      else { s.pt = (*p)[0]; s.pl = (*p)[1]; s.pb = (*p)[2]; s.pr = (*p)[3]; }
    }
    std::string ap = n.attr_s("auto_pad", "NOTSET");
    if (ap == "VALID") s.pt = s.pl = s.pb = s.pr = 0;
    else if (ap == "SAME_UPPER" || ap == "SAME_LOWER") {
      int64_t oh = (H + s.sh - 1) / s.sh, ow = (W + s.sw - 1) / s.sw;
      int64_t ph = std::max<int64_t>(0, (oh - 1) * s.sh + (s.kh - 1) * s.dh + 1 - H);
      int64_t pw = std::max<int64_t>(0, (ow - 1) * s.sw + (s.kw - 1) * s.dw + 1 - W);
      bool up = ap == "SAME_UPPER";
      s.pt = up ? ph / 2 : ph - ph / 2; s.pb = ph - s.pt;
      s.pl = up ? pw / 2 : pw - pw / 2; s.pr = pw - s.pl;
    } else if (ap != "NOTSET") unsupported(n, "auto_pad " + ap);
    if (extra_pad && (extra_pad[0] || extra_pad[1] || extra_pad[2] || extra_pad[3])) {  // a Pad node in front (TF exporters)
      if (ap == "SAME_UPPER" || ap == "SAME_LOWER") unsupported(n, "auto_pad SAME behind an explicit Pad");
      s.pt += extra_pad[0]; s.pl += extra_pad[1]; s.pb += extra_pad[2]; s.pr += extra_pad[3];
    }
    // A model file is untrusted input: attributes that would divide by zero or index backwards are rejected here
    // (the reference's parser returns an error for them; it must never take the host process down).
    if (s.sh < 1 || s.sw < 1) unsupported(n, "strides must be >= 1");
    if (s.dh < 1 || s.dw < 1) unsupported(n, "dilations must be >= 1");
    if (s.kh < 1 || s.kw < 1) unsupported(n, "kernel extents must be >= 1");
    if (s.pt < 0 || s.pl < 0 || s.pb < 0 || s.pr < 0) unsupported(n, "negative pads");
    const int64_t lim = int64_t(1) << 20;  // keeps every extent product below far inside int64
    if (s.sh > lim || s.sw > lim || s.dh > lim || s.dw > lim || s.kh > lim || s.kw > lim || s.pt > lim || s.pl > lim || s.pb > lim || s.pr > lim)
      unsupported(n, "spatial attribute out of range");
    // pooling only: ceil_mode=1 rounds the extent up, and a last window that would start beyond the input plus
    // its leading pad is dropped (ONNX MaxPool / AveragePool); the kernels already ignore out-of-image taps
    const bool ceil_mode = n.attr_i("ceil_mode", 0) != 0;
    auto extent = [&](int64_t in, int64_t p0, int64_t p1, int64_t k, int64_t d, int64_t st) {
      const int64_t num = in + p0 + p1 - (d * (k - 1) + 1);
      int64_t o = (ceil_mode ? (num + st - 1) / st : num / st) + 1;
      if (ceil_mode && (o - 1) * st >= in + p0) o--;
      return o;
    };
    s.OH = extent(H, s.pt, s.pb, s.kh, s.dh, s.sh);
    s.OW = extent(W, s.pl, s.pr, s.kw, s.dw, s.sw);
    if (s.OH <= 0 || s.OW <= 0) unsupported(n, "empty spatial output");
  }

  void Lowerer::conv(const NodeDef &n) {
    const Val &a = get(n, 0);
    const Val &w = get(n, 1);
    const bool one_d = a.shape.size() == 3 && w.shape.size() == 3;  // Conv1d: [N,C,L] as [N,C,1,L], kernel [M,C/g,k] as [M,C/g,1,k]
    if (a.is_const || (a.shape.size() != 4 && !one_d)) unsupported(n, "only [N,C,L] / [N,C,H,W] activations");
    if (!w.is_const || (w.shape.size() != 4 && !one_d)) unsupported(n, "weights must be a constant [M,C/g,kh,kw] (or [M,C/g,k])");
    if (w.c->q_data && qconv_from_qdq(n)) return;
    Step s;
    s.kind = StepKind::Conv2d;
    s.in0 = a.buf;
    conv_geometry(n, s, a, w.shape);
    s.W = cf32(n, w);
    if (has_input(n, 2)) {
      s.bias = cf32(n, get(n, 2));
      if (int64_t(s.bias.size()) != s.Mo) unsupported(n, "bias size mismatch");
    }
    emit(std::move(s), n, conv_out_shape(s, a));
  }
  // the geometry fields of a Conv / QLinearConv node over activation `a` with a kernel of shape `ws` ([M,C/g,kh,kw], or [M,C/g,k]: Conv1d)
  void Lowerer::conv_geometry(const NodeDef &n, Step &s, const Val &a, const std::vector<int64_t> &ws) {
    const bool one_d = a.shape.size() == 3;
    s.C = a.shape[1]; s.H = one_d ? 1 : a.shape[2]; s.Wd = one_d ? a.shape[2] : a.shape[3];
    s.Mo = ws[0]; s.kh = one_d ? 1 : ws[2]; s.kw = one_d ? ws[2] : ws[3];
    s.groups = n.attr_i("group", 1);
    if (s.groups < 1 || s.C != ws[1] * s.groups || s.Mo % s.groups) unsupported(n, "channel/group mismatch");
    spatial(n, s, s.H, s.Wd, a.pend);
    s.K = (s.C / s.groups) * s.kh * s.kw;
    s.M = s.Mo;
  }
  std::vector<int64_t> Lowerer::conv_out_shape(const Step &s, const Val &a) {
    if (a.shape.size() == 3) return {a.shape[0], s.Mo, s.OW};
    return {a.shape[0], s.Mo, s.OH, s.OW};
  }

  // ---- ConvTranspose / Resize / Upsample: the operators that make a tensor spatially larger (host/deconv.hpp) ----
  // scale / shift per output channel into a transposed convolution's weights [C, M/g, kh, kw] and bias, in f64, rounded once
  void Lowerer::convt_fold_affine(Step &p, const std::vector<double> &sc, const std::vector<double> &sh, const std::string &label) {
    const int64_t Cg = p.C / p.groups, Mg = p.Mo / p.groups, taps = p.kh * p.kw;
    for (int64_t c = 0; c < p.C; c++)
      for (int64_t ml = 0; ml < Mg; ml++) {
        const double f = sc[size_t((c / Cg) * Mg + ml)];
        float *w = p.W.data() + (c * Mg + ml) * taps;
        for (int64_t t = 0; t < taps; t++) w[t] = float(f * double(w[t]));
      }
    if (p.bias.empty()) p.bias.assign(size_t(p.Mo), 0.f);
    for (int64_t mo = 0; mo < p.Mo; mo++) p.bias[size_t(mo)] = float(sc[size_t(mo)] * double(p.bias[size_t(mo)]) + sh[size_t(mo)]);
    p.origin += "+" + label;
  }
  void Lowerer::conv_transpose(const NodeDef &n) {
    const Val &a = get(n, 0);
    if (a.is_const || (a.shape.size() != 3 && a.shape.size() != 4)) bad_form(n, "the input must be an [N,C,L] or [N,C,H,W] activation (rank 3 or 4), got " + shape_str(a.shape));
    const bool one_d = a.shape.size() == 3;
    const Val &w = get(n, 1);
    if (!w.is_const || w.c->dtype != onnx::kFloat) bad_form(n, "W must be a constant f32 tensor");
    if (has_input(n, 2) && (!get(n, 2).is_const || get(n, 2).c->dtype != onnx::kFloat)) bad_form(n, "B must be a constant f32 tensor");
    if (w.shape.size() != a.shape.size()) bad_form(n, "W " + shape_str(w.shape) + " does not have the rank of the input " + shape_str(a.shape));
    Step s;
    s.kind = StepKind::ConvTranspose2d;
    s.in0 = a.buf;
    s.C = a.shape[1]; s.H = one_d ? 1 : a.shape[2]; s.Wd = one_d ? a.shape[2] : a.shape[3];
    s.kh = one_d ? 1 : w.shape[2]; s.kw = one_d ? w.shape[2] : w.shape[3];
    s.groups = n.attr_i("group", 1);
    if (s.groups < 1 || s.C % s.groups != 0) bad_form(n, "C = " + std::to_string(s.C) + " is not a multiple of group = " + std::to_string(s.groups));
    if (w.shape[0] != s.C || w.shape[1] < 1) bad_form(n, "W " + shape_str(w.shape) + " disagrees with C = " + std::to_string(s.C) + " input channels ([C, M/group, kh, kw])");
    if (auto *ks = n.attr_ints("kernel_shape")) {
      const bool ok = one_d ? (ks->size() == 1 && (*ks)[0] == s.kw) : (ks->size() == 2 && (*ks)[0] == s.kh && (*ks)[1] == s.kw);
      if (!ok) bad_form(n, "kernel_shape disagrees with W " + shape_str(w.shape));
    }
    s.Mo = w.shape[1] * s.groups;
    const size_t nsp = one_d ? 1 : 2;
    auto two = [&](const char *name, int64_t dflt, int64_t &h, int64_t &wd) {
      h = wd = dflt;
      if (auto *p = n.attr_ints(name)) {
        if (p->size() != nsp) bad_form(n, std::string(name) + " must have one entry per spatial axis");
        if (one_d) wd = (*p)[0]; else { h = (*p)[0]; wd = (*p)[1]; }
      }
    };
    int64_t oph, opw, osh = -1, osw = -1;
    two("strides", 1, s.sh, s.sw);
    two("dilations", 1, s.dh, s.dw);
    two("output_padding", 0, oph, opw);
    const bool has_os = n.attr_ints("output_shape") != nullptr;
    if (has_os) two("output_shape", -1, osh, osw);
    const int64_t lim = int64_t(1) << 20;
    if (s.sh < 1 || s.sw < 1 || s.sh > lim || s.sw > lim) bad_form(n, "strides must be >= 1");
    if (s.dh < 1 || s.dw < 1 || s.dh > lim || s.dw > lim) bad_form(n, "dilations must be >= 1");
    if (s.kh < 1 || s.kw < 1 || s.kh > kConvTMaxKernel || s.kw > kConvTMaxKernel)
      bad_form(n, "kernel extents must be 1.." + std::to_string(kConvTMaxKernel) + " (the cap of the transposed-convolution kernels' tap tables)");
    if (oph < 0 || opw < 0 || oph >= std::max(s.sh, s.dh) || opw >= std::max(s.sw, s.dw))
      bad_form(n, "output_padding must be smaller than max(stride, dilation) on its axis");
    if (s.H > lim || s.Wd > lim) bad_form(n, "spatial extent out of range");
    const std::string ap = n.attr_s("auto_pad", "NOTSET");
    if (ap != "NOTSET" && ap != "VALID" && ap != "SAME_UPPER" && ap != "SAME_LOWER") bad_form(n, "auto_pad " + ap);
    if (auto *p = n.attr_ints("pads")) {
      if (p->size() != 2 * nsp) bad_form(n, "pads must have two entries per spatial axis");
      if (one_d) { s.pl = (*p)[0]; s.pr = (*p)[1]; }
      else { s.pt = (*p)[0]; s.pl = (*p)[1]; s.pb = (*p)[2]; s.pr = (*p)[3]; }
    }
    if (ap == "VALID") s.pt = s.pl = s.pb = s.pr = 0;
    const bool same = ap == "SAME_UPPER" || ap == "SAME_LOWER";
    if (has_os || same) {  // the total padding follows from the wanted extent, split as the operator specification says
      if (one_d) osh = 1;  // (the H axis of the [N,C,1,L] form)
      auto split = [&](int64_t in, int64_t st, int64_t k, int64_t d, int64_t op, int64_t want, int64_t &p0, int64_t &p1) {
        if (!has_os) want = in * st;
        const int64_t total = st * (in - 1) + op + (k - 1) * d + 1 - want;
        if (total < 0) bad_form(n, "negative pads: the output extent " + std::to_string(want) + " cannot be reached (it needs a total padding of " + std::to_string(total) + ")");
        p0 = ap == "SAME_UPPER" ? total / 2 : total - total / 2;
        p1 = total - p0;
      };
      if (!one_d) split(s.H, s.sh, s.kh, s.dh, oph, osh, s.pt, s.pb);
      split(s.Wd, s.sw, s.kw, s.dw, opw, osw, s.pl, s.pr);
    }
    if (s.pt < 0 || s.pl < 0 || s.pb < 0 || s.pr < 0) bad_form(n, "negative pads");
    if (s.pt > lim || s.pl > lim || s.pb > lim || s.pr > lim) bad_form(n, "pads out of range");
    s.OH = (s.H - 1) * s.sh - s.pt - s.pb + s.dh * (s.kh - 1) + oph + 1;
    s.OW = (s.Wd - 1) * s.sw - s.pl - s.pr + s.dw * (s.kw - 1) + opw + 1;
    if (s.OH < 1 || s.OW < 1) bad_form(n, "negative extents: the output would be " + std::to_string(s.OH) + " x " + std::to_string(s.OW));
    s.W = w.c->f32;
    if (int64_t(s.W.size()) != prod({s.C, w.shape[1], s.kh, s.kw})) bad_form(n, "W " + shape_str(w.shape) + " disagrees with its payload");
    if (has_input(n, 2)) {
      s.bias = get(n, 2).c->f32;
      if (int64_t(s.bias.size()) != s.Mo) bad_form(n, "B has " + std::to_string(s.bias.size()) + " entries for M = " + std::to_string(s.Mo) + " output channels");
    }
    s.K = (s.C / s.groups) * s.kh * s.kw;
    s.M = s.Mo;
    auto pack = std::make_shared<DeconvPack>();
    pack->out_pad_h = oph;
    pack->out_pad_w = opw;
    convt_build_phases(s, *pack);
    s.deconv = pack;
    std::vector<int64_t> shape = {a.shape[0], s.Mo, s.OH, s.OW};
    if (one_d) shape = {a.shape[0], s.Mo, s.OW};
    emit(std::move(s), n, shape);
  }

  void Lowerer::resize(const NodeDef &n) {
    const bool upsample = n.op == "Upsample";
    const Val &a = get(n, 0);
    if (a.is_const || (a.shape.size() != 3 && a.shape.size() != 4)) bad_form(n, "the input must be an [N,C,L] or [N,C,H,W] activation, got " + shape_str(a.shape));
    const bool one_d = a.shape.size() == 3;
    const size_t rank = a.shape.size();
    std::string mode = n.attr_s("mode", "nearest");
    if (mode == "bilinear") mode = "linear";  // (the spelling of early Upsample exports)
    if (mode != "nearest" && mode != "linear") bad_form(n, "mode " + mode + " (only nearest and linear)");
    const bool old_form = upsample || m.opset < 11;  // Upsample and Resize-10: asymmetric coordinates, nearest by floor
    const std::string coord = old_form ? "asymmetric" : n.attr_s("coordinate_transformation_mode", "half_pixel");
    const std::string nearest_mode = old_form ? "floor" : n.attr_s("nearest_mode", "round_prefer_floor");
    if (coord != "half_pixel" && coord != "pytorch_half_pixel" && coord != "asymmetric" && coord != "align_corners")
      bad_form(n, "coordinate_transformation_mode " + coord);
    if (nearest_mode != "round_prefer_floor" && nearest_mode != "round_prefer_ceil" && nearest_mode != "floor" && nearest_mode != "ceil")
      bad_form(n, "nearest_mode " + nearest_mode);
    if (n.attr_i("antialias", 0) != 0) bad_form(n, "antialias = 1");
    if (n.attr_i("exclude_outside", 0) != 0) bad_form(n, "exclude_outside = 1");
    if (n.attr_s("keep_aspect_ratio_policy", "stretch") != "stretch") bad_form(n, "keep_aspect_ratio_policy " + n.attr_s("keep_aspect_ratio_policy", "stretch"));
    if (n.attrs.count("axes")) bad_form(n, "the axes attribute");
    // scales (floats) or sizes (integers), one per axis of the input; roi is ignored
    std::vector<double> scales;
    std::vector<int64_t> sizes;
    const size_t scales_at = (upsample || m.opset < 11) ? 1 : 2;
    if (upsample && m.opset < 9) {
      if (auto *at = n.attr("scales")) scales.assign(at->floats.begin(), at->floats.end());
    } else if (has_input(n, scales_at)) {
      const Val &v = get(n, scales_at);
      if (!v.is_const || v.c->dtype != onnx::kFloat) bad_form(n, "scales must be a constant");
      scales.assign(v.c->f32.begin(), v.c->f32.end());
    }
    if (!old_form && has_input(n, 3)) {
      const Val &v = get(n, 3);
      if (!v.is_const || v.c->dtype != onnx::kInt64) bad_form(n, "sizes must be a constant (or fold from the shape of the input)");
      sizes = v.c->i64;
    }
    if (scales.empty() == sizes.empty()) bad_form(n, "exactly one of scales and sizes must be given");
    if ((scales.empty() ? sizes.size() : scales.size()) != rank) bad_form(n, "scales / sizes must have one entry per axis of the input");
    const int64_t in_h = one_d ? 1 : a.shape[2], in_w = one_d ? a.shape[2] : a.shape[3];
    int64_t out_h = 1, out_w;
    double scale_h = 1.0, scale_w;
    const int64_t lim = int64_t(1) << 20;
    auto axis = [&](size_t ax, int64_t in, int64_t &out, double &sc) {
      if (!scales.empty()) {
        sc = scales[ax];
        if (!(sc > 0.0) || !std::isfinite(sc) || sc * double(in) > double(lim)) bad_form(n, "scale out of range");
        out = int64_t(std::floor(double(in) * sc));
      } else {
        out = sizes[ax];
        if (out < 1 || out > lim) bad_form(n, "size out of range");
        sc = double(out) / double(in);
      }
      if (out < 1) bad_form(n, "empty spatial output");
    };
    if (!scales.empty() ? (scales[0] != 1.0 || scales[1] != 1.0) : (sizes[1] != a.shape[1] || (sizes[0] != 0 && sizes[0] != a.shape[0] && a.shape[0] > 0)))
      bad_form(n, "scaling of the N or C axis");
    if (!one_d) axis(2, in_h, out_h, scale_h);
    axis(rank - 1, in_w, out_w, scale_w);
    Step s;
    s.kind = StepKind::Resize2d;
    s.in0 = a.buf;
    s.C = a.shape[1]; s.H = in_h; s.Wd = in_w; s.Mo = s.C; s.OH = out_h; s.OW = out_w;
    auto pack = std::make_shared<DeconvPack>();
    pack->linear = mode == "linear";
    pack->coord_mode = coord;
    pack->nearest_mode = nearest_mode;
    resize_axis_table(in_h, out_h, scale_h, pack->linear, coord, nearest_mode, pack->row_idx, pack->row_wgt);
    resize_axis_table(in_w, out_w, scale_w, pack->linear, coord, nearest_mode, pack->col_idx, pack->col_wgt);
    s.deconv = pack;
    std::vector<int64_t> shape = {a.shape[0], s.C, out_h, out_w};
    if (one_d) shape = {a.shape[0], s.C, out_w};
    emit(std::move(s), n, shape);
  }

  void Lowerer::batchnorm(const NodeDef &n) {
    const Val &a = get(n, 0);
    if (a.is_const || a.shape.size() < 2) unsupported(n, "bad input");
    const auto &sc = cf32(n, get(n, 1)), &bi = cf32(n, get(n, 2)), &mu = cf32(n, get(n, 3)), &var = cf32(n, get(n, 4));
    const int64_t C = a.shape[1];
    if (int64_t(sc.size()) != C || int64_t(bi.size()) != C || int64_t(mu.size()) != C || int64_t(var.size()) != C)
      unsupported(n, "parameter size mismatch");
    float eps = n.attr_f("epsilon", 1e-5f);
    std::vector<float> scale((size_t)C), shift((size_t)C);
    for (int64_t c = 0; c < C; c++) {
      float inv = 1.0f / std::sqrt(var[size_t(c)] + eps);
      scale[size_t(c)] = sc[size_t(c)] * inv;
      shift[size_t(c)] = bi[size_t(c)] - mu[size_t(c)] * scale[size_t(c)];
    }
    std::vector<int64_t> shape = a.shape;
    if (Step *p = fusable_producer(n, 0)) {
      if (p->kind == StepKind::ConvTranspose2d && p->act == Act::None && p->Mo == C) {  // fold into the transposed convolution (f64, one rounding)
        std::vector<double> dsc((size_t)C), dsh((size_t)C);
        for (int64_t c = 0; c < C; c++) {
          dsc[size_t(c)] = double(sc[size_t(c)]) / std::sqrt(double(var[size_t(c)]) + double(eps));
          dsh[size_t(c)] = double(bi[size_t(c)]) - double(mu[size_t(c)]) * dsc[size_t(c)];
        }
        convt_fold_affine(*p, dsc, dsh, "BatchNormalization");
        set_act(n, a.buf, shape, true);
        return;
      }
      if (p->kind == StepKind::Conv2d && p->act == Act::None) {  // fold into conv
        const int64_t per_m = p->K;
        for (int64_t mo = 0; mo < p->Mo; mo++)
          for (int64_t k = 0; k < per_m; k++) p->W[size_t(mo * per_m + k)] *= scale[size_t(mo)];
        if (p->bias.empty()) p->bias.assign(size_t(p->Mo), 0.f);
        for (int64_t mo = 0; mo < p->Mo; mo++) p->bias[size_t(mo)] = p->bias[size_t(mo)] * scale[size_t(mo)] + shift[size_t(mo)];
        p->origin += "+BatchNormalization";
        set_act(n, a.buf, shape, true);
        return;
      }
      if (p->kind == StepKind::Dense && p->act == Act::None && a.shape.size() == 2 && p->M == C) {  // Dense -> BN (Keras MLPs)
        for (int64_t k = 0; k < p->K; k++)
          for (int64_t j = 0; j < C; j++) p->W[size_t(k * C + j)] *= scale[size_t(j)];
        if (p->bias.empty()) p->bias.assign(size_t(C), 0.f);
        for (int64_t j = 0; j < C; j++) p->bias[size_t(j)] = p->bias[size_t(j)] * scale[size_t(j)] + shift[size_t(j)];
        p->origin += "+BatchNormalization";
        set_act(n, a.buf, shape, true);
        return;
      }
    }
    Step s;
    s.kind = StepKind::AffineChannel;
    s.in0 = a.buf;
    s.C = C;
    s.S = prod(a.shape, 2);
    s.scale = std::move(scale);
    s.shift = std::move(shift);
    emit(std::move(s), n, shape);
  }

  // ---- InstanceNormalization / GroupNormalization (host/spatialnorm.hpp): one SpatialNorm step ----------------------
  // `a` [N,C,L] / [N,C,H,W] normalised over each of G channel groups with per-channel scale / shift; the result is bound to `out_name`
  void Lowerer::spatial_norm_step(const NodeDef &n, const Val &a, int64_t G, std::vector<float> scale, std::vector<float> shift, float eps, const std::string &origin,
                                  const std::string &out_name) {
    if (const std::string why = spatialnorm_refusal(a.shape, G, int64_t(scale.size()), int64_t(shift.size()), eps); !why.empty()) bad_form(n, why);
    if (plan.buf_shape[size_t(a.buf)].size() != 4) bad_form(n, "the input " + shape_str(a.shape) + " is a window of a flat table, not an [N,C,L] / [N,C,H,W] tensor");
    Step s;
    s.kind = StepKind::SpatialNorm;
    s.in0 = a.buf;
    s.C = a.shape[1];
    s.S = prod(a.shape, 2);
    s.H = a.shape.size() == 4 ? a.shape[2] : 1;
    s.Wd = a.shape.back();
    s.groups = G;
    s.scale = std::move(scale);
    s.shift = std::move(shift);
    s.ln_eps = eps;
    s.origin = origin;
    const std::vector<int64_t> shape = a.shape;
    Val v;
    v.buf = push_step(std::move(s), shape);
    v.shape = shape;
    vals[out_name] = v;
    buf_names[v.buf].push_back(out_name);
  }
  // the activation input of a normalisation node and its constant scale / B
  Val Lowerer::spatial_norm_input(const NodeDef &n, std::vector<float> *scale, std::vector<float> *bias) {
    const Val a = get(n, 0);
    if (a.is_const) bad_form(n, "the input must be an activation");
    if (a.ra != 0) bad_form(n, "the input " + shape_str(a.shape) + " is a time-major value (its row axis is axis " + std::to_string(a.ra) + ")");
    for (size_t i = 1; i <= 2; i++) {
      if (!has_input(n, i)) bad_form(n, "scale and B are required");
      const Val &c = get(n, i);
      if (!c.is_const || c.c->dtype != onnx::kFloat) bad_form(n, "scale and B must be constant f32 tensors");
      *(i == 1 ? scale : bias) = c.c->f32;
    }
    return a;
  }
  void Lowerer::instance_norm(const NodeDef &n) {
    std::vector<float> sc, bi;
    const Val a = spatial_norm_input(n, &sc, &bi);
    const int64_t C = a.shape.size() >= 2 ? a.shape[1] : 0;
    spatial_norm_step(n, a, std::max<int64_t>(C, 1), std::move(sc), std::move(bi), n.attr_f("epsilon", 1e-5f), node_label(n), n.outputs[0]);
  }
  // GroupNormalization: scale / bias per group under opset 18 (broadcast over the group's channels here), per channel under opset 21;
  // stash_type only names the precision of the statistics, which is f32 here
  void Lowerer::group_norm(const NodeDef &n) {
    std::vector<float> sc, bi, scale, shift;
    const Val a = spatial_norm_input(n, &sc, &bi);
    if (m.opset < 18) bad_form(n, "GroupNormalization needs opset 18 or later");
    const int64_t G = n.attr_i("num_groups", 0), C = a.shape.size() >= 2 ? a.shape[1] : 0;
    if (G < 1) bad_form(n, "the num_groups attribute is required");
    if (C > 0 && C % G != 0) bad_form(n, "num_groups = " + std::to_string(G) + " does not divide C = " + std::to_string(C));
    const bool per_group = m.opset < 21;
    if (C > 0 && (!spatialnorm_per_channel(sc, C, G, per_group, &scale) || !spatialnorm_per_channel(bi, C, G, per_group, &shift) || sc.size() != bi.size()))
      bad_form(n, "scale / bias have " + std::to_string(sc.size()) + " and " + std::to_string(bi.size()) + " entries: opset " + std::to_string(m.opset) + " takes " +
                      (per_group ? "num_groups = " + std::to_string(G) + " (or C = " + std::to_string(C) + ")" : "C = " + std::to_string(C)));
    spatial_norm_step(n, a, G, std::move(scale), std::move(shift), n.attr_f("epsilon", 1e-5f), node_label(n), n.outputs[0]);
  }

  void Lowerer::find_group_norms() {
    for (size_t i = 0; i < m.nodes.size(); i++) {
      const NodeDef &r = m.nodes[i];
      if (!graph->live[i] || absorbed[i] || r.op != "Reshape" || r.inputs.size() != 2 || r.outputs.empty()) continue;
      const NodeDef *in = graph->sole_reader(r.outputs[0], false);
      if (!in || in->op != "InstanceNormalization" || in->inputs.size() != 3 || in->inputs[0] != r.outputs[0]) continue;
      const NodeDef *back = graph->sole_reader(in->outputs[0], false);
      if (!back || back->op != "Reshape" || back->inputs.size() != 2 || back->inputs[0] != in->outputs[0]) continue;
      gn_at[i] = GnMatch{size_t(in - m.nodes.data()), size_t(back - m.nodes.data())};
    }
  }
  // a constant that multiplies / shifts x [N,C,...] per channel: C values shaped [C,1,1] / [1,C,1,1] (one spatial axis: [C,1] / [1,C,1])
  const std::vector<float> *Lowerer::per_channel_const(const Val *c, const std::vector<int64_t> &x_shape) {
    if (!c || !c->is_const || c->c->dtype != onnx::kFloat) return nullptr;
    const size_t r = x_shape.size(), cr = c->shape.size();
    if (cr != r && cr != r - 1) return nullptr;
    for (size_t i = 0; i < cr; i++)
      if (c->shape[i] != (i + (r - cr) == 1 ? x_shape[1] : 1)) return nullptr;
    return &c->c->f32;
  }
  bool Lowerer::exporter_group_norm(const GnMatch &gm, const NodeDef &first) {
    const NodeDef &inorm = m.nodes[gm.inorm], &back = m.nodes[gm.back];
    const Val *xp = find_value(first.inputs[0]);
    if (!xp || xp->is_const || xp->pv || xp->ra != 0 || xp->buf < 0 || (xp->shape.size() != 3 && xp->shape.size() != 4)) return false;
    const Val x = *xp;
    const int64_t C = x.shape[1], S = prod(x.shape, 2);
    const Val *t = find_value(first.inputs[1]);
    if (C < 1 || S < 1 || !t || !t->is_const || t->c->dtype != onnx::kInt64 || t->c->i64.size() != 3) return false;
    const auto &tg = t->c->i64;
    const int64_t G = tg[1];
    if (G < 1 || C % G != 0 || !(tg[0] == 0 || (tg[0] > 0 && tg[0] == x.shape[0])) || !(tg[2] == -1 || tg[2] == (C / G) * S)) return false;
    const Val *sv = find_value(inorm.inputs[1]), *bv = find_value(inorm.inputs[2]);
    if (!sv || !bv || !sv->is_const || !bv->is_const || sv->c->dtype != onnx::kFloat || bv->c->dtype != onnx::kFloat || int64_t(sv->c->f32.size()) != G ||
        int64_t(bv->c->f32.size()) != G)
      return false;
    // the Reshape back: a constant that spells x's shape (0 = copy, -1 / the fixed batch in front), or Shape(x) not folded yet
    if (const Val *bs = find_value(back.inputs[1])) {
      if (!bs->is_const || bs->c->dtype != onnx::kInt64 || bs->c->i64.size() != x.shape.size()) return false;
      const auto &b = bs->c->i64;
      if (!(b[0] == 0 || b[0] == -1 || (b[0] > 0 && b[0] == x.shape[0]))) return false;
      for (size_t i = 1; i < b.size(); i++)
        if (b[i] != x.shape[i] && b[i] != 0) return false;
    } else {
      const NodeDef *shp = graph->producer(back.inputs[1]);
      if (!shp) return false;
      const NodeDef &sh = *shp;
      const Val *of = sh.op == "Shape" && sh.inputs.size() == 1 && sh.attrs.empty() ? find_value(sh.inputs[0]) : nullptr;
      if (!of || of->is_const || of->buf != x.buf || of->shape != x.shape) return false;
    }
    std::vector<const NodeDef *> nodes = {&inorm, &back};
    const NodeDef *last = &back;
    std::vector<float> gamma, beta;
    if (const NodeDef *mul = graph->sole_reader(last->outputs[0], false); mul && mul->op == "Mul")
      if (const std::vector<float> *g = per_channel_const(const_operand(*mul, last->outputs[0]), x.shape)) {
        gamma = *g;
        nodes.push_back(last = mul);
      }
    if (const NodeDef *add = graph->sole_reader(last->outputs[0], false); add && add->op == "Add")
      if (const std::vector<float> *b = per_channel_const(const_operand(*add, last->outputs[0]), x.shape)) {
        beta = *b;
        nodes.push_back(last = add);
      }
    const float eps = inorm.attr_f("epsilon", 1e-5f);
    if (!spatialnorm_refusal(x.shape, G, C, C, eps).empty() || plan.buf_shape[size_t(x.buf)].size() != 4) return false;
    std::vector<float> scale, shift;
    spatialnorm_fold_inner(sv->c->f32, bv->c->f32, gamma, beta, C, &scale, &shift);
    std::string origin = node_label(first);
    for (const NodeDef *q : nodes) {
      absorbed[size_t(q - m.nodes.data())] = 1;
      origin += "+" + node_label(*q);
    }
    spatial_norm_step(first, x, G, std::move(scale), std::move(shift), eps, origin, last->outputs[0]);
    if (cur_half) mark_half(last->outputs[0]);
    return true;
  }

  void Lowerer::pool(const NodeDef &n, bool is_max) {
    const Val &a = get(n, 0);
    const bool one_d = a.shape.size() == 3;
    if (a.is_const || (a.shape.size() != 4 && !one_d)) unsupported(n, "only [N,C,L] / [N,C,H,W] activations");
    auto *ks = n.attr_ints("kernel_shape");
    if (!ks || ks->size() != (one_d ? 1u : 2u)) unsupported(n, "kernel_shape must have one entry per spatial axis");
    Step s;
    s.kind = StepKind::Pool2d;
    s.in0 = a.buf;
    s.is_max = is_max;
    s.count_pad = n.attr_i("count_include_pad", 0) != 0;
    if (!is_max && s.count_pad && n.attr_i("ceil_mode", 0) != 0) unsupported(n, "ceil_mode=1 with count_include_pad=1");
    s.C = a.shape[1]; s.H = one_d ? 1 : a.shape[2]; s.Wd = one_d ? a.shape[2] : a.shape[3];
    s.kh = one_d ? 1 : (*ks)[0]; s.kw = one_d ? (*ks)[0] : (*ks)[1];
    spatial(n, s, s.H, s.Wd);
    std::vector<int64_t> shape = {a.shape[0], s.C, s.OH, s.OW};
    if (one_d) shape = {a.shape[0], s.C, s.OW};
    emit(std::move(s), n, shape);
  }

  // Pad with zeros on the two spatial axes of an [N,C,H,W] activation: no kernel -- the value keeps its buffer and
  // the Conv that consumes it widens its own padding (the form TF / Keras exporters write for 'same' convolutions).
  void Lowerer::pad(const NodeDef &n) {
    const Val &a = get(n, 0);
    if (a.is_const || a.shape.size() != 4) unsupported(n, "only [N,C,H,W] activations");
    if (n.attr_s("mode", "constant") != "constant") unsupported(n, "only constant (zero) padding");
    std::vector<int64_t> pads;
    if (has_input(n, 1)) pads = const_ints(n, 1, "pads");
    else if (auto *p = n.attr_ints("pads")) pads = *p;
    if (pads.size() != 8) unsupported(n, "pads must hold 8 entries for a 4-D tensor");
    float value = n.attr_f("value", 0.f);
    if (has_input(n, 2)) {
      const auto &cv = cf32(n, get(n, 2));
      if (cv.size() != 1) unsupported(n, "constant_value must be a scalar");
      value = cv[0];
    }
    if (value != 0.f) unsupported(n, "only zero padding folds into a convolution");
    if (has_input(n, 3)) unsupported(n, "axes input");
    if (pads[0] || pads[1] || pads[4] || pads[5]) unsupported(n, "padding of the batch / channel axes");
    for (auto v : pads)
      if (v < 0) unsupported(n, "negative pads (cropping)");
    Val v = a;
    v.pend[0] += pads[2]; v.pend[1] += pads[3]; v.pend[2] += pads[6]; v.pend[3] += pads[7];
    vals[n.outputs[0]] = v;
    buf_names[v.buf].push_back(n.outputs[0]);
    alias_edges[v.buf]++;
  }
  void Lowerer::lrn(const NodeDef &n) {
    const Val &a = get(n, 0);
    if (a.is_const || a.shape.size() < 3) unsupported(n, "only [N,C,...] activations");
    Step s;
    s.kind = StepKind::LRN;
    s.in0 = a.buf;
    s.C = a.shape[1];
    s.S = prod(a.shape, 2);
    s.lrn_size = n.attr_i("size", 0);
    if (s.lrn_size < 1) unsupported(n, "size attribute required");
    if (s.lrn_size > (int64_t(1) << 20)) unsupported(n, "size out of range");  // the kernels carry it as int
    s.lrn_alpha = n.attr_f("alpha", 1e-4f);
    s.lrn_beta = n.attr_f("beta", 0.75f);
    s.lrn_bias = n.attr_f("bias", 1.f);
    std::vector<int64_t> shape = a.shape;
    emit(std::move(s), n, shape);
  }
  // Transpose: constants are folded (2-D weight matrices); on activations only the channel shuffle of ShuffleNet-style
  // blocks -- Reshape [N,C,H,W] -> [N,g,C/g,H,W], Transpose(0,2,1,3,4), Reshape back -- which is a channel permutation.
  void Lowerer::transpose(const NodeDef &n) {
    const Val &a = get(n, 0);
    const int64_t rank = int64_t(a.shape.size());
    std::vector<int64_t> perm;
    if (auto *p = n.attr_ints("perm")) perm = *p;
    else for (int64_t i = rank; i-- > 0;) perm.push_back(i);
    if (int64_t(perm.size()) != rank) unsupported(n, "perm length");
    if (a.is_const) {
      if (rank != 2 || a.c->dtype != onnx::kFloat) unsupported(n, "only 2-D f32 constants are folded");
      if (perm[0] == 0 && perm[1] == 1) { vals[n.outputs[0]] = a; return; }
      const int64_t R = a.shape[0], Cc = a.shape[1];
      std::vector<float> t(size_t(R * Cc));
      for (int64_t r = 0; r < R; r++)
        for (int64_t c = 0; c < Cc; c++) t[size_t(c * R + r)] = a.c->f32[size_t(r * Cc + c)];
      vals[n.outputs[0]] = const_f32(std::move(t), {Cc, R});
      return;
    }
    // Transpose(0,2,3,1) of the [N,C,H,W] tensor a step wrote moves nothing: the result is a channels-last view of that tensor (lower_on_view)
    if (rank == 4 && perm == std::vector<int64_t>{0, 2, 3, 1} && nchw_tensor(a)) {
      const int buf = a.buf;
      const std::vector<int64_t> shape = {a.shape[0], a.shape[2], a.shape[3], a.shape[1]};
      set_act(n, buf, shape, true);
      vals[n.outputs[0]].cl = true;
      return;
    }
    const bool shuffle = a.ra == 0 && rank >= 4 && perm[0] == 0 && perm[1] == 2 && perm[2] == 1 && [&] {
      for (int64_t i = 3; i < rank; i++)
        if (perm[size_t(i)] != i) return false;
      return true;
    }();
    // (with C = 1 or S = 1 the crossing moves nothing: it stays the alias below, and only a class-token Concat makes it a step: tokens_concat)
    if (rank == 3 && perm[0] == 0 && perm[1] == 2 && perm[2] == 1 && conv_tensor_view(a) && a.shape[1] != 1 && a.shape[2] != 1) return tokens_step(n, a);
    if (!shuffle && (a.ra != 0 || rank == 3)) {
      // (time-major values, and the rank-3 rows-first values a Transpose(1,0,2) makes time-major; other tensors are not touched) a permutation that only moves (or keeps) the row axis and leaves the other axes in the order they lie in memory: an alias with a
      // new row-axis tag (the Transposes exporters put around time-major recurrent layers)
      for (int64_t i = 0; i < rank; i++)
        if (perm[size_t(i)] < 0 || perm[size_t(i)] >= rank) unsupported(n, "perm entry out of range");
      int ra = -1;
      int64_t last = -1;
      bool in_order = true;
      std::vector<int64_t> out;
      for (int64_t i = 0; i < rank; i++) {
        const int64_t src = perm[size_t(i)];
        out.push_back(a.shape[size_t(src)]);
        if (src == a.ra) { ra = int(i); continue; }
        if (a.shape[size_t(src)] == 1) continue;
        in_order = in_order && src > last;
        last = src;
      }
      if (ra < 0 || !in_order)
        unsupported(n, "on activations only the channel shuffle (0,2,1,3,...) or a permutation that moves nothing but the row axis is supported: this one would need data moved");
      const int buf = a.buf;
      set_act(n, buf, out, true, ra);
      return;
    }
    if (!shuffle) unsupported(n, "on activations only the channel shuffle (0,2,1,3,...) keeps rows independent and is supported");
    Step s;
    s.kind = StepKind::ChannelShuffle;
    s.in0 = a.buf;
    s.groups = a.shape[1];
    s.C = a.shape[1] * a.shape[2];
    s.S = prod(a.shape, 3);
    // the buffer is registered as the [N,C,spatial...] tensor it is for the layout rules; the value carries the 5-D shape
    std::vector<int64_t> bshape = {a.shape[0], s.C};
    for (int64_t i = 3; i < rank; i++) bshape.push_back(a.shape[size_t(i)]);
    std::vector<int64_t> vshape = a.shape;
    std::swap(vshape[1], vshape[2]);
    s.origin = node_label(n);
    set_act(n, push_step(std::move(s), bshape), vshape);
  }

  // ---- channels-last views and ChannelNorm (host/channelnorm.hpp): ConvNeXt's permute -> LayerNorm -> Linear -> GELU ->
  // Linear -> permute.  Transpose(0,2,3,1) of an [N,C,H,W] tensor a step wrote emits nothing: its result is a VIEW (Val::cl) that names the
  // same buffer.  The operators below read a view as the NCHW tensor it is and lower as they do on one; Transpose(0,3,1,2) ends it ----
  // Is the rank-4 rows-first value `a` the [N,C,H,W] tensor a step wrote?  (The model input is not: buffer 0 has no producer.)
  bool Lowerer::nchw_tensor(const Val &a) const {
    if (a.is_const || a.pv || a.nn || a.q || a.cl || a.ra != 0 || a.padded() || a.buf <= 0 || a.shape.size() != 4 || !producer.count(a.buf)) return false;
    const auto &bs = plan.buf_shape[size_t(a.buf)];
    return bs.size() == 4 && bs[1] == a.shape[1] && bs[2] == a.shape[2] && bs[3] == a.shape[3] && bs[1] > 0 && bs[2] > 0 && bs[3] > 0;
  }
  bool Lowerer::reads_view(const NodeDef &n) const {
    for (const auto &in_name : n.inputs) {
      auto it = vals.find(in_name);
      if (it != vals.end() && it->second.cl) return true;
    }
    return false;
  }
  // a copy of `n` whose input `i` is the constant `c`
  NodeDef Lowerer::with_const_input(const NodeDef &n, size_t i, Val c) {
    NodeDef r = n;
    r.inputs[i] = n.inputs[i] + "#" + std::to_string(view_consts++);
    vals[r.inputs[i]] = std::move(c);
    return r;
  }
  // the constant `c` with the dims `dims` (the same elements: type and half tag kept)
  Val Lowerer::redimensioned(const Val &c, std::vector<int64_t> dims, std::vector<float> f32) {
    auto t = std::make_shared<TensorData>();
    t->dtype = c.c->dtype;
    t->elem = c.c->elem;
    t->dims = std::move(dims);
    t->f32 = std::move(f32);
    return const_val(std::move(t));
  }
  void Lowerer::lower_on_view(const NodeDef &n) {
    const std::string &op = n.op;
    static const std::set<std::string> unary_ops = {"Relu", "Sigmoid", "Tanh", "LeakyRelu", "Clip", "Exp", "Log", "Sqrt", "Neg", "Abs", "Elu", "Selu", "Softplus",
                                                    "HardSigmoid", "HardSwish", "Erf", "Gelu", "Reciprocal", "Floor", "Ceil", "Softsign", "Round"};
    static const std::map<std::string, char> binary_ops = {{"Add", '+'}, {"Sub", '-'}, {"Mul", '*'}, {"Div", '/'}};
    if (op == "Transpose") {
      const Val a = get(n, 0);
      const auto *perm = n.attr_ints("perm");
      if (!perm || *perm != std::vector<int64_t>{0, 3, 1, 2})
        bad_form(n, "it reads the channels-last view '" + n.inputs[0] + "' " + shape_str(a.shape) + "; only Transpose(0,3,1,2), which ends the view, moves no data");
      set_act(n, a.buf, {a.shape[0], a.shape[3], a.shape[1], a.shape[2]}, true);
      return;
    }
    if (op == "LayerNormalization") return channel_norm_node(n);
    if (op == "MatMul") return view_matmul(n);
    if (unary_ops.count(op)) {
      if (!get(n, 0).cl) bad_form(n, "it reads the channels-last view among its parameters");
      return as_nchw(n, [&] { unary(n); });
    }
    if (auto bo = binary_ops.find(op); bo != binary_ops.end() && n.inputs.size() == 2) {
      const Val a = get(n, 0), b = get(n, 1);
      if (!a.is_const && !b.is_const) {
        if (!(a.cl && b.cl)) {
          const bool a_view = a.cl;
          bad_form(n, "it mixes the channels-last view '" + n.inputs[a_view ? 0 : 1] + "' " + shape_str((a_view ? a : b).shape) + " with '" + n.inputs[a_view ? 1 : 0] + "' " +
                          shape_str((a_view ? b : a).shape) + ", which is not one; Transpose(0,3,1,2) ends a view");
        }
        if (a.shape != b.shape) bad_form(n, "two channels-last views must have one shape, got " + shape_str(a.shape) + " and " + shape_str(b.shape));
        return as_nchw(n, [&] { binary(n, bo->second); });
      }
      const size_t ci = a.is_const ? 0 : 1;
      const Val &v = a.is_const ? b : a, &c = a.is_const ? a : b;
      if (c.c->dtype != onnx::kFloat) bad_form(n, "the constant operand of an operator on a channels-last view must be f32");
      const int64_t C = v.shape[3];
      if (c.c->f32.size() == 1) return as_nchw(n, [&] { binary(n, bo->second); });  // a scalar
      const bool per_channel = int64_t(c.c->f32.size()) == C && !c.shape.empty() && c.shape.back() == C && c.shape.size() <= 4;
      if (!per_channel)
        bad_form(n, "the constant " + shape_str(c.shape) + " is neither a scalar nor one value per channel ([" + std::to_string(C) + "] or [1,1,1," + std::to_string(C) +
                        "]) of the channels-last view " + shape_str(v.shape));
      // one value per channel, read as [C,1,1]: the per-channel rule of an [N,C,H,W] tensor
      const NodeDef r = with_const_input(n, ci, redimensioned(c, {C, 1, 1}, c.c->f32));
      return as_nchw(r, [&] { binary(r, bo->second); });
    }
    for (size_t i = 0; i < n.inputs.size(); i++)
      if (auto it = vals.find(n.inputs[i]); it != vals.end() && it->second.cl)
        bad_form(n, "it reads the channels-last view '" + n.inputs[i] + "' " + shape_str(it->second.shape) + " (a Transpose(0,2,3,1) that moved no data); only LayerNormalization(axis = -1), "
                    "MatMul by a constant, elementwise operators and Transpose(0,3,1,2) read one");
  }
  // ONE ChannelNorm step on the [N,C,H,W] tensor `x`; the result is bound to `out_name`, as a view or not
  void Lowerer::channel_norm_step(const NodeDef &n, const Val &x, std::vector<float> scale, std::vector<float> shift, bool has_shift, float eps, const std::string &origin,
                                  const std::string &out_name, bool as_view) {
    const int64_t C = x.shape[1], S = x.shape[2] * x.shape[3];
    if (const std::string why = channelnorm_refusal(C, S, int64_t(scale.size()), has_shift ? int64_t(shift.size()) : -1, eps); !why.empty()) bad_form(n, why);
    Step s;
    s.kind = StepKind::ChannelNorm;
    s.in0 = x.buf;
    s.C = C;
    s.S = S;
    s.H = x.shape[2];
    s.Wd = x.shape[3];
    s.scale = std::move(scale);
    if (has_shift) s.shift = std::move(shift);
    s.ln_eps = eps;
    s.origin = origin;
    const std::vector<int64_t> shape = x.shape;
    Val v;
    v.buf = push_step(std::move(s), shape);
    v.shape = as_view ? std::vector<int64_t>{shape[0], shape[2], shape[3], shape[1]} : shape;
    v.cl = as_view;
    vals[out_name] = v;
    buf_names[v.buf].push_back(out_name);
  }
  // LayerNormalization(axis = -1) on a view: over the channels at each pixel
  void Lowerer::channel_norm_node(const NodeDef &n) {
    const Val a = get(n, 0);
    if (!a.cl) bad_form(n, "it reads the channels-last view among its parameters");
    int64_t axis = n.attr_i("axis", -1);
    if (axis < 0) axis += 4;
    if (axis != 3)
      bad_form(n, "on the channels-last view " + shape_str(a.shape) + " only normalisation over the channel axis (axis = -1) is supported, got axis " + std::to_string(n.attr_i("axis", -1)));
    for (size_t o = 1; o < n.outputs.size(); o++)
      if (!n.outputs[o].empty() && uses.count(n.outputs[o]) && uses[n.outputs[o]] > 0)
        bad_form(n, std::string("output ") + (o == 1 ? "Mean" : "InvStdDev") + " is consumed; only Y is served");
    if (!has_input(n, 1)) bad_form(n, "Scale is required");
    const Val &g = get(n, 1);
    if (!g.is_const || g.c->dtype != onnx::kFloat) bad_form(n, "Scale and B must be constant f32 tensors");
    std::vector<float> scale = g.c->f32, shift;
    const bool has_b = has_input(n, 2);
    if (has_b) {
      const Val &b = get(n, 2);
      if (!b.is_const || b.c->dtype != onnx::kFloat) bad_form(n, "Scale and B must be constant f32 tensors");
      shift = b.c->f32;
    }
    Val x = a;
    x.shape = {a.shape[0], a.shape[3], a.shape[1], a.shape[2]};
    x.cl = false;
    channel_norm_step(n, x, std::move(scale), std::move(shift), has_b, n.attr_f("epsilon", 1e-5f), node_label(n), n.outputs[0], true);
  }
  // MatMul of a view by a constant [C, M]: the 1x1 convolution [M, C, 1, 1] it is, through the path a Conv node takes
  void Lowerer::view_matmul(const NodeDef &n) {
    const Val a = get(n, 0);
    const Val &b = get(n, 1);
    if (!a.cl) bad_form(n, "the channels-last view '" + n.inputs[1] + "' is its right operand; only view x constant [C, M] is supported");
    const int64_t C = a.shape[3];
    if (!b.is_const || b.c->dtype != onnx::kFloat || b.shape.size() != 2 || b.shape[0] != C || b.c->q_data)
      bad_form(n, "a MatMul on the channels-last view " + shape_str(a.shape) + " needs a constant f32 [" + std::to_string(C) + ", M] right operand" +
                      (b.is_const ? ", got " + shape_str(b.shape) : ", got an activation"));
    const int64_t M = b.shape[1];
    std::vector<float> w(size_t(M * C));
    for (int64_t c = 0; c < C; c++)
      for (int64_t mo = 0; mo < M; mo++) w[size_t(mo * C + c)] = b.c->f32[size_t(c * M + mo)];
    NodeDef r = with_const_input(n, 1, redimensioned(b, {M, C, 1, 1}, std::move(w)));
    r.attrs.clear();
    as_nchw(r, [&] { conv(r); });
  }
  // Hugging Face's ConvNextLayerNorm(data_format = "channels_first") on an [N,C,H,W] tensor a step wrote:
  //   ReduceMean(axes = [1]) -> Sub -> Pow(2) | Mul(d, d) -> ReduceMean(axes = [1]) -> Add(eps) -> Sqrt -> Div [-> Mul(w [C,1,1])] [-> Add(b [C,1,1])]
  // matched forward from the first ReduceMean as decomposed_layer_norm matches the [N,E] form; the nodes up to the Div emit nothing, and the
  // Mul / Add behind it compose into gamma and beta by the per-channel rule (binary).  false: not that chain
  bool Lowerer::channel_axis_mean(const NodeDef &n) {
    if (n.op != "ReduceMean" || n.attr_i("keepdims", 1) == 0) return false;
    std::vector<int64_t> axes;
    if (has_input(n, 1)) {
      const Val *c = find_value(n.inputs[1]);
      if (!c || !c->is_const || c->c->dtype != onnx::kInt64) return false;
      axes = c->c->i64;
    } else if (auto *p = n.attr_ints("axes")) axes = *p;
    return axes.size() == 1 && (axes[0] == 1 || axes[0] == -3);
  }
  bool Lowerer::channels_first_norm(const NodeDef &mean, const Val &x) {
    if (!nchw_tensor(x) || !channel_axis_mean(mean)) return false;
    const NodeDef *sub = only_reader(mean.outputs[0]);
    if (!sub || sub->op != "Sub" || sub->inputs.size() != 2 || sub->inputs[0] != mean.inputs[0] || sub->inputs[1] != mean.outputs[0]) return false;
    const std::string &d = sub->outputs[0];
    for (const auto &o : m.outputs)
      if (o.name == d) return false;
    auto dit = graph->consumers_of.find(d);
    if (dit == graph->consumers_of.end()) return false;
    const std::set<size_t> readers(dit->second.begin(), dit->second.end());
    if (readers.size() != 2) return false;
    const NodeDef *sq = nullptr, *div = nullptr;
    for (size_t c : readers) {
      const NodeDef &r = m.nodes[c];
      if (r.op == "Div" && r.inputs.size() == 2 && r.inputs[0] == d) div = &r;
      else if (r.op == "Mul" && r.inputs.size() == 2 && r.inputs[0] == d && r.inputs[1] == d) sq = &r;
      else if (r.op == "Pow") {
        const Val *e = const_operand(r, d, true);
        if (e && e->c->f32.size() == 1 && e->c->f32[0] == 2.f) sq = &r;
      }
    }
    if (!sq || !div) return false;
    const NodeDef *var = only_reader(sq->outputs[0]);
    if (!var || !channel_axis_mean(*var)) return false;
    const NodeDef *add = only_reader(var->outputs[0]);
    const Val *eps = add && add->op == "Add" ? const_operand(*add, var->outputs[0]) : nullptr;
    if (!eps || eps->c->f32.size() != 1 || !(eps->c->f32[0] >= 0.f) || !std::isfinite(eps->c->f32[0])) return false;
    const NodeDef *sq_rt = only_reader(add->outputs[0]);
    if (!sq_rt || sq_rt->op != "Sqrt" || only_reader(sq_rt->outputs[0]) != div || div->inputs[1] != sq_rt->outputs[0]) return false;
    const int64_t C = x.shape[1];
    if (!channelnorm_refusal(C, x.shape[2] * x.shape[3], C, -1, eps->c->f32[0]).empty()) return false;
    for (const NodeDef *q : {sub, sq, var, add, sq_rt, div}) absorbed[size_t(q - m.nodes.data())] = 1;
    channel_norm_step(mean, x, std::vector<float>(size_t(C), 1.f), {}, false, eps->c->f32[0], node_label(mean) + "+...+" + node_label(*div), div->outputs[0], false);
    if (cur_half) mark_half(div->outputs[0]);
    return true;
  }

  // ---- the crossing from the image path to the table path (host/tokens.hpp): Conv -> Flatten(2) / Reshape [N,E,S] ->
  // Transpose(0,2,1) [-> Concat(class tokens, .)] [-> Add(position table)] is ONE Tokens step.  The Transpose emits it; a Concat and an
  // Add behind it move their constants into its tables (tokens_concat, binary) ----
  // Is the rank-3 rows-first value `a` the [N, C, S] tensor a step wrote -- itself ([N,C,L], held as [N,C,1,L]) or a view of [N,C,H,W]?
  // (The model input and its views are not: buffer 0 has no producer.)
  bool Lowerer::conv_tensor_view(const Val &a) const {
    if (a.is_const || a.pv || a.nn || a.ra != 0 || a.buf <= 0 || a.shape.size() != 3 || !producer.count(a.buf)) return false;
    const auto &bs = plan.buf_shape[size_t(a.buf)];
    return bs.size() == 4 && bs[1] == a.shape[1] && bs[2] > 0 && bs[3] > 0 && bs[2] * bs[3] == a.shape[2];
  }
  // Flatten(axis = 2) of an [N,C,H,W] tensor a step wrote, read by Transpose(0,2,1) nodes only: the [N, C, H*W] view torch's flatten(2)
  // stands for (the [N*C, H*W] matrix the operator specification gives has the same elements in the same order)
  bool Lowerer::token_view_of_flatten(const NodeDef &n, const Val &a) const {
    if (a.is_const || a.pv || a.ra != 0 || a.buf <= 0 || !producer.count(a.buf) || plan.buf_shape[size_t(a.buf)].size() != 4) return false;
    auto it = graph->consumers_of.find(n.outputs[0]);
    if (it == graph->consumers_of.end() || it->second.empty()) return false;
    for (const auto &o : m.outputs)
      if (o.name == n.outputs[0]) return false;
    for (size_t c : it->second) {
      const NodeDef &r = m.nodes[c];
      const auto *perm = r.attr_ints("perm");
      if (r.op != "Transpose" || !perm || *perm != std::vector<int64_t>{0, 2, 1}) return false;
    }
    return true;
  }
  void Lowerer::tokens_step(const NodeDef &n, const Val &a) {
    const auto &bs = plan.buf_shape[size_t(a.buf)];
    if (const std::string why = tokens_refusal(bs); !why.empty()) bad_form(n, why);
    Step s;
    s.kind = StepKind::Tokens;
    s.in0 = a.buf;
    s.C = s.K = a.shape[1];
    s.S = s.rep = a.shape[2];
    emit_window(std::move(s), n, {a.shape[0], a.shape[2], a.shape[1]});
  }
  // the Tokens step whose result `v` is, as that step left it
  Step *Lowerer::tokens_producer(const Val &v) {
    if (v.is_const || v.buf <= 0 || v.ra != 0 || v.shape.size() != 3) return nullptr;
    auto it = producer.find(v.buf);
    if (it == producer.end()) return nullptr;
    Step &p = plan.steps[size_t(it->second)];
    return p.kind == StepKind::Tokens && p.out == v.buf && v.shape[1] == p.rep && v.shape[2] == p.K ? &p : nullptr;
  }
  // Concat with a token value among its operands: constants per row in front of it become the step's prefix rows.  false: no operand is one
  bool Lowerer::tokens_concat(const NodeDef &n) {
    size_t at = SIZE_MAX;
    for (size_t i = 0; i < n.inputs.size(); i++)
      if (const Val *v = find_value(n.inputs[i]); v && tokens_producer(*v)) at = i;
    // a crossing that moved nothing (C = 1 or S = 1) was left an alias of the convolutional tensor; constants joined to it make it a step
    // here, written as this node's result (without a constant among the operands the Concat lowers as it always did)
    bool promoted = false;
    if (at == SIZE_MAX) {
      bool any_const = false;
      Val view;
      for (size_t i = 0; i < n.inputs.size(); i++) {
        const Val *v = find_value(n.inputs[i]);
        if (!v) continue;
        any_const = any_const || v->is_const;
        if (v->is_const || v->shape.size() != 3 || (v->shape[1] != 1 && v->shape[2] != 1)) continue;
        Val u = *v;
        std::swap(u.shape[1], u.shape[2]);
        if (conv_tensor_view(u)) { at = i; view = u; }
      }
      if (at == SIZE_MAX || !any_const) return false;
      tokens_step(n, view);
      promoted = true;
    }
    const Val tok = promoted ? *find_value(n.outputs[0]) : get(n, at);
    Step *p = tokens_producer(tok);
    int64_t axis = n.attr_i("axis", 1);
    if (axis < 0) axis += 3;
    if (axis != 1) bad_form(n, "axis = " + std::to_string(n.attr_i("axis", 1)) + ": constant rows join a token window [N, T, E] along the token axis (1) only");
    if (at + 1 != n.inputs.size()) bad_form(n, "operand " + std::to_string(at + 1) + " stands behind the tokens; only class tokens in front of them are folded");
    const int64_t N = tok.shape[0], E = p->K;
    std::vector<float> rows = p->prefix;
    for (size_t i = 0; i < at; i++) {
      const Val &c = get(n, i);
      if (!c.is_const) bad_form(n, "operand " + std::to_string(i) + " in front of the tokens is not a constant; only constant class tokens are folded");
      if (c.c->dtype != onnx::kFloat) bad_form(n, "operand " + std::to_string(i) + " is not an f32 constant");
      auto ex = expanded_lead.find(n.inputs[i]);
      if (ex != expanded_lead.end()) {  // an Expand to [batch, p, E]: the batch entry is the folded row count (0) or the fixed batch
        if (!(ex->second == 0 ? N < 0 : ex->second == N))
          bad_form(n, "operand " + std::to_string(i) + " was expanded to " + std::to_string(ex->second) + " rows, the tokens have " + (N < 0 ? std::string("a symbolic row count") : std::to_string(N)));
      } else if (!(N == 1 && c.shape.size() == 3 && c.shape[0] == 1)) {
        bad_form(n, "operand " + std::to_string(i) + " " + shape_str(c.shape) + " is a constant that was not expanded over the rows (Expand); as it stands it joins a batch of 1 only");
      }
      int64_t np = 0, width = 0;
      std::vector<float> r;
      if (!tokens_prefix_rows(c.shape, c.c->f32, &np, &width, &r)) bad_form(n, "operand " + std::to_string(i) + " " + shape_str(c.shape) + " is not [1, p, E] / [p, E] constant rows, the same for every image");
      if (const std::string why = tokens_prefix_refusal(int64_t(rows.size()) / E, np, width, E); !why.empty()) bad_form(n, why);
      rows.insert(rows.end(), r.begin(), r.end());
    }
    if (!p->cst.empty()) bad_form(n, "the position table is already added to the tokens");
    if (!promoted && live_uses(tok.buf) != 1) bad_form(n, "the tokens '" + n.inputs[at] + "' have a second reader");
    const int64_t T = int64_t(rows.size()) / E + p->S;
    if (prod({T, E}) > kMaxPerRow) throw InferaError::onnx("activation of " + std::to_string(T * E) + " elements per row is too large");
    p->prefix = std::move(rows);
    p->rep = T;
    if (!promoted) p->origin += "+" + node_label(n);
    plan.buf_per_row[size_t(tok.buf)] = T * E;
    plan.buf_shape[size_t(tok.buf)] = {N, T * E};
    if (promoted) vals[n.outputs[0]].shape = {N, T, E};  // (tokens_step registered the result under this node's name already)
    else set_act(n, tok.buf, {N, T, E}, true);
    return true;
  }

  // ---- the decomposed LayerNorm older exporters write, on [rows, E] (where nothing else serves it):
  //   ReduceMean(-1) -> Sub -> Pow(2) | Mul(d, d) -> ReduceMean(-1) -> Add(eps) -> Sqrt -> Div [-> Mul(gamma)] [-> Add(beta)]
  // matched forward from the first ReduceMean when it is met; the nodes behind it emit nothing and the last one's output is the step's.
  const NodeDef *Lowerer::only_reader(const std::string &v) const { return graph->sole_reader(v, true); }
  bool Lowerer::last_axis_mean(const NodeDef &n, int64_t rank) {
    if (n.op != "ReduceMean" || n.attr_i("keepdims", 1) == 0) return false;
    std::vector<int64_t> axes;
    if (has_input(n, 1)) {
      const Val *c = find_value(n.inputs[1]);
      if (!c || !c->is_const || c->c->dtype != onnx::kInt64) return false;
      axes = c->c->i64;
    } else if (auto *p = n.attr_ints("axes")) axes = *p;
    return axes.size() == 1 && (axes[0] == -1 || axes[0] == rank - 1);
  }
  // the f32 constant other operand of a two-input node reading `v`, or null
  const Val *Lowerer::const_operand(const NodeDef &n, const std::string &v, bool second_only) {
    if (n.inputs.size() != 2) return nullptr;
    const bool left = n.inputs[0] == v;
    if (!left && (second_only || n.inputs[1] != v)) return nullptr;
    const Val *c = find_value(n.inputs[left ? 1 : 0]);
    return c && c->is_const && c->c->dtype == onnx::kFloat ? c : nullptr;
  }
  bool Lowerer::decomposed_layer_norm(const NodeDef &mean, const Val &x) {
    const int64_t rank = int64_t(x.shape.size()), E = x.shape.back();
    if (rank != 2 || x.ra != 0 || E < 1 || E > kLnMaxE || !last_axis_mean(mean, rank)) return false;
    std::vector<const NodeDef *> nodes;
    const NodeDef *sub = only_reader(mean.outputs[0]);
    if (!sub || sub->op != "Sub" || sub->inputs.size() != 2 || sub->inputs[0] != mean.inputs[0] || sub->inputs[1] != mean.outputs[0]) return false;
    const std::string &d = sub->outputs[0];
    for (const auto &o : m.outputs)
      if (o.name == d) return false;
    auto dit = graph->consumers_of.find(d);
    if (dit == graph->consumers_of.end()) return false;
    const std::set<size_t> readers(dit->second.begin(), dit->second.end());
    if (readers.size() != 2) return false;
    const NodeDef *sq = nullptr, *div = nullptr;
    for (size_t c : readers) {
      const NodeDef &r = m.nodes[c];
      if (r.op == "Div" && r.inputs.size() == 2 && r.inputs[0] == d) div = &r;
      else if (r.op == "Mul" && r.inputs.size() == 2 && r.inputs[0] == d && r.inputs[1] == d) sq = &r;
      else if (r.op == "Pow") {
        const Val *e = const_operand(r, d, true);
        if (e && e->c->f32.size() == 1 && e->c->f32[0] == 2.f) sq = &r;
      }
    }
    if (!sq || !div) return false;
    const NodeDef *var = only_reader(sq->outputs[0]);
    if (!var || !last_axis_mean(*var, rank)) return false;
    const NodeDef *add = only_reader(var->outputs[0]);
    const Val *eps = add && add->op == "Add" ? const_operand(*add, var->outputs[0]) : nullptr;
    if (!eps || eps->c->f32.size() != 1 || !(eps->c->f32[0] >= 0.f) || !std::isfinite(eps->c->f32[0])) return false;
    const NodeDef *sq_rt = only_reader(add->outputs[0]);
    if (!sq_rt || sq_rt->op != "Sqrt" || only_reader(sq_rt->outputs[0]) != div || div->inputs[1] != sq_rt->outputs[0]) return false;
    Step s;
    s.kind = StepKind::LayerNorm;
    s.in0 = x.buf;
    s.K = E;
    s.rep = 1;
    s.ln_eps = eps->c->f32[0];
    s.scale.assign(size_t(E), 1.f);
    nodes = {sub, sq, var, add, sq_rt, div};
    const NodeDef *last = div;
    if (const NodeDef *mul = only_reader(div->outputs[0]); mul && mul->op == "Mul") {
      const Val *g = const_operand(*mul, div->outputs[0]);
      if (g && int64_t(g->c->f32.size()) == E && g->shape.size() <= 2 && (g->shape.size() < 2 || g->shape[0] == 1)) {
        s.scale = g->c->f32;
        nodes.push_back(last = mul);
      }
    }
    if (const NodeDef *bad = only_reader(last->outputs[0]); bad && bad->op == "Add") {
      const Val *b = const_operand(*bad, last->outputs[0]);
      if (b && int64_t(b->c->f32.size()) == E && b->shape.size() <= 2 && (b->shape.size() < 2 || b->shape[0] == 1)) {
        s.shift = b->c->f32;
        nodes.push_back(last = bad);
      }
    }
    for (const NodeDef *q : nodes) absorbed[size_t(q - m.nodes.data())] = 1;
    s.origin = node_label(mean) + "+...+" + node_label(*last);
    const std::vector<int64_t> shape = x.shape;
    Val v;
    v.buf = push_step(std::move(s), shape);
    v.shape = shape;
    vals[last->outputs[0]] = v;
    buf_names[v.buf].push_back(last->outputs[0]);
    return true;
  }

  // LayerNormalization (opset 17) over the last axis of [rows, E] / [rows, T, E]: one LayerNorm step (hip/layernorm.hip)
  void Lowerer::layer_norm(const NodeDef &n) {
    const Val a = get(n, 0);
    const int64_t rank = int64_t(a.shape.size());
    if (a.is_const || rank < 2) unsupported(n, "unsupported operator form: the input must be a [rows, E] or [rows, T, E] activation");
    int64_t axis = n.attr_i("axis", -1);
    if (axis < 0) axis += rank;
    if (axis != rank - 1)
      unsupported(n, "unsupported operator form: only normalisation over the last axis (axis = -1) is supported, got axis " + std::to_string(n.attr_i("axis", -1)) +
                         " of " + shape_str(a.shape));
    for (size_t o = 1; o < n.outputs.size(); o++)
      if (!n.outputs[o].empty() && uses.count(n.outputs[o]) && uses[n.outputs[o]] > 0)
        unsupported(n, std::string("unsupported operator form: output ") + (o == 1 ? "Mean" : "InvStdDev") + " is consumed; only Y is served");
    if (!has_input(n, 1)) unsupported(n, "unsupported operator form: Scale is required");
    const int64_t E = a.shape[size_t(rank - 1)];
    if (E < 1 || E > kLnMaxE) unsupported(n, "unsupported operator form: E = " + std::to_string(E) + " is beyond the LayerNorm kernel's cap of " + std::to_string(kLnMaxE));
    Step s;
    s.kind = StepKind::LayerNorm;
    s.in0 = a.buf;
    s.K = E;
    s.rep = prod(a.shape, 1) / E;
    s.scale = cf32(n, get(n, 1));
    if (has_input(n, 2)) s.shift = cf32(n, get(n, 2));
    if (int64_t(s.scale.size()) != E || (!s.shift.empty() && int64_t(s.shift.size()) != E)) unsupported(n, "unsupported operator form: Scale / B must have E = " + std::to_string(E) + " elements");
    s.ln_eps = n.attr_f("epsilon", 1e-5f);
    if (!(s.ln_eps >= 0.f) || !std::isfinite(s.ln_eps)) unsupported(n, "unsupported operator form: epsilon must be a finite number >= 0");
    if (rank == 3) emit_window(std::move(s), n, a.shape);
    else emit(std::move(s), n, a.shape);
  }

  // a constant known before the walk (an initializer or a Constant node): its first element and its element count
  bool Lowerer::graph_const_scalar(const std::string &name, double *v, size_t *count) const {
    const GraphIndex::Const c = graph->constant(name);
    const TensorData *t = c.t.get();
    if (!t) {
      if (!c.node) return false;
      if (auto *i = c.node->attr("value_int")) { *v = double(i->i); if (count) *count = 1; return true; }
      else if (auto *f = c.node->attr("value_float")) { *v = double(f->f); if (count) *count = 1; return true; }
      else return false;
    }
    const size_t n = t->count();
    if (count) *count = n;
    if (n < 1) return false;
    *v = t->dtype == onnx::kInt64 ? double(t->i64[0]) : double(t->f32[0]);
    return true;
  }
  // `v0` as a row mask; "" or why it is none.  lens: as the length column of a recurrent layer's sequence_lens (find_seq_lens): the same
  // source tracing through Cast / Reshape / Flatten only, and the source may be a rank-1 value
  std::string Lowerer::trace_row_mask(const std::string &v0, RowMask *rm, bool lens) const {
    const std::string what = lens ? "sequence_lens" : "mask";
    std::vector<size_t> chain;
    std::string v = v0;
    for (int hop = 0; hop < 32; hop++) {
      auto pi = graph->producer_of.find(v);
      if (pi == graph->producer_of.end()) break;
      const NodeDef &p = m.nodes[pi->second];
      if (!graph->std_dom(p) || p.inputs.empty()) break;
      double c;
      if (lens) {
        if (p.op != "Reshape" && p.op != "Cast" && p.op != "Flatten") break;
        v = p.inputs[0];
      } else if (p.op == "Unsqueeze" || p.op == "Reshape" || p.op == "Cast" || p.op == "Expand" || p.op == "Not") v = p.inputs[0];
      else if (p.op == "Equal" && p.inputs.size() == 2) v = p.inputs[graph_const_scalar(p.inputs[0], &c) ? 1 : 0];
      else break;
      chain.push_back(pi->second);
    }
    if (auto pi = graph->producer_of.find(v); pi != graph->producer_of.end() && m.nodes[pi->second].op == "Transpose")
      return "a time-major " + what + " source (the Transpose '" + node_label(m.nodes[pi->second]) + "' in front of it); only a rows-first " +
             (lens ? "[N] or [N, 1]" : "[N, T]") + " graph input";
    if (auto pi = graph->producer_of.find(v); lens && pi != graph->producer_of.end() && m.nodes[pi->second].op == "ReduceSum")
      return "sequence_lens computed by the ReduceSum '" + node_label(m.nodes[pi->second]) + "' (lengths derived from a mask are not supported; pass the length column itself)";
    EmbedCols cols;
    if (!embed_cols(v, &cols).empty() || (!cols.rank2 && !lens) || !cols.off.empty())
      return "the " + what + " source '" + v + "' is not a column range of a graph input (a " + (lens ? "length" : "mask") + " computed from activations is not supported)";
    rm->src0 = cols.src0, rm->k = cols.k;
    rm->is_int = cols.int_input || cols.truncated;
    rm->nodes = cols.chain;
    rm->shape = cols.rank2 ? std::vector<int64_t>{-1, cols.k} : std::vector<int64_t>{-1};
    rm->state = 0;
    rm->cmp = 0.f;
    bool expanded = false;
    for (auto it = chain.rbegin(); it != chain.rend(); ++it) {
      const NodeDef &p = m.nodes[*it];
      const std::string at = "'" + node_label(p) + "' in the " + what + " sub-graph: ";
      rm->nodes.push_back(*it);
      std::vector<int64_t> &sh = rm->shape;
      if (p.op == "Cast") {
        const int64_t to = p.attr_i("to", onnx::kFloat);
        if (rm->state == 0 && (to == onnx::kInt64 || to == onnx::kInt32)) rm->is_int = true;
      } else if (p.op == "Not") {
        if (rm->state == 0) return at + "Not of a value that no Equal produced";
        rm->state = 3 - rm->state;
      } else if (p.op == "Equal") {
        double c = 0;
        size_t cnt = 0;
        const bool c0 = graph_const_scalar(p.inputs[0], &c, &cnt);
        if (rm->state != 0 || (!c0 && !graph_const_scalar(p.inputs[1], &c, &cnt)) || cnt != 1) return at + "only Equal(source, one constant)";
        if (double(float(c)) != c) return at + "the compare value is no f32 number (values arrive as f32)";
        rm->cmp = float(c);
        rm->state = 1;
      } else if (expanded) {
        return at + "a " + p.op + " behind the Expand";
      } else if (p.op == "Flatten") {  // (lens only) [N, k] stays [N, k]
        const int64_t axis = p.attr_i("axis", 1);
        if (sh.size() != 2 || (axis != 1 && axis != -1)) return at + "only Flatten(axis = 1) of an [N, k] value";
      } else if (p.op == "Unsqueeze") {
        std::vector<int64_t> ax;
        if (!graph_ints_arg(p, 1, "axes", &ax) || ax.empty()) return at + "axes must be constant";
        const int64_t r = int64_t(sh.size() + ax.size());
        for (auto &a : ax) a = a < 0 ? a + r : a;
        std::sort(ax.begin(), ax.end());
        for (int64_t a : ax) {
          if (a < 1 || a > int64_t(sh.size())) return at + "an axis in front of the rows or out of range";
          sh.insert(sh.begin() + a, 1);
        }
      } else if (p.op == "Reshape") {
        std::vector<int64_t> tgt, tdims;
        if (p.inputs.size() != 2 || !graph_const_ints(p.inputs[1], &tgt, &tdims) || tgt.empty()) return at + "the target shape must be constant";
        if (!(tgt[0] == 0 || tgt[0] == -1 || (tgt[0] > 0 && tgt[0] == plan.input_shape[0]))) return at + "the target " + shape_str(tgt) + " does not keep the row axis";
        int64_t per = 1, known = 1, neg = -1;
        for (size_t i = 1; i < sh.size(); i++) per *= sh[i];
        for (size_t i = 1; i < tgt.size(); i++) {
          if (tgt[i] == 0 && i < sh.size()) tgt[i] = sh[i];
          if (tgt[i] == -1 && neg < 0 && tgt[0] != -1) neg = int64_t(i);
          else if (tgt[i] <= 0) return at + "the target " + shape_str(tgt);
          else known *= tgt[i];
        }
        if (neg >= 0) {
          if (per % known) return at + "the target " + shape_str(tgt);
          tgt[size_t(neg)] = per / known, known = per;
        }
        if (known != per) return at + "the target " + shape_str(tgt) + " does not keep the " + std::to_string(per) + " " + (lens ? "length" : "mask") + " values of a row";
        tgt[0] = -1;
        sh = tgt;
      } else {  // Expand: a constant target is checked; one computed from a Shape broadcasts to its reader's shape, as ONNX would anyway
        std::vector<int64_t> tgt, tdims;
        if (p.inputs.size() != 2) return at + "no target";
        if (graph_const_ints(p.inputs[1], &tgt, &tdims)) {
          if (tgt.size() < sh.size()) return at + "the target " + shape_str(tgt) + " has a lower rank than the mask";
          const size_t lead = tgt.size() - sh.size();
          for (size_t i = 1; i < sh.size(); i++)
            if (tgt[lead + i] != 1 && tgt[lead + i] != sh[i] && sh[i] != 1) return at + "the target " + shape_str(tgt) + " does not broadcast from " + shape_str(sh);
        } else {
          if (graph->row_data.count(p.inputs[1])) return at + "the target depends on the rows";
          std::vector<std::string> work{p.inputs[1]};
          while (!work.empty()) {  // the Shape sub-graph behind the target: it emits nothing either
            const std::string w = work.back();
            work.pop_back();
            auto pi = graph->producer_of.find(w);
            if (pi == graph->producer_of.end() || m.nodes[pi->second].op == "Constant" || std::count(rm->aux.begin(), rm->aux.end(), pi->second)) continue;
            rm->aux.push_back(pi->second);
            if (m.nodes[pi->second].op != "Shape")
              for (const auto &in : m.nodes[pi->second].inputs) work.push_back(in);
          }
        }
        expanded = true;
      }
    }
    return "";
  }
  // the negative constant scalar b of masked keys
  float Lowerer::row_mask_fill(const NodeDef &n, const std::string &name, bool add) {
    double b = 0;
    size_t cnt = 0;
    if (graph->row_data.count(name) || !graph_const_scalar(name, &b, &cnt)) bad_form(n, "the fill '" + name + "' of masked keys is not a constant");
    if (cnt != 1) bad_form(n, "the fill '" + name + "' of masked keys has " + std::to_string(cnt) + " elements; only one scalar");
    const float f = float(b);
    if (!(f < 0.f)) bad_form(n, "the fill of masked keys is " + std::to_string(b) + "; only a negative number or -inf");
    if (add && f == -INFINITY) bad_form(n, "the fill of masked keys is -inf in the additive form (1 - mask) * fill, which is NaN at every kept key; use a finite fill or Where");
    return f;
  }
  // Add(scores, other): other = Mul(Sub(1, float(mask [N,1,1,T])), b) (BERT); false: no such form
  bool Lowerer::match_add_row_mask(const NodeDef &add, const std::string &other, AttnMatch &am) {
    auto pi = graph->producer_of.find(other);
    if (pi == graph->producer_of.end()) return false;
    const NodeDef &mul = m.nodes[pi->second];
    if (mul.op != "Mul" || mul.inputs.size() != 2) return false;
    int side = -1;
    const NodeDef *sub = nullptr;
    for (int j = 0; j < 2; j++) {
      auto si = graph->producer_of.find(mul.inputs[size_t(j)]);
      double one = 0;
      size_t cnt = 0;
      if (si != graph->producer_of.end() && m.nodes[si->second].op == "Sub" && m.nodes[si->second].inputs.size() == 2 &&
          graph_const_scalar(m.nodes[si->second].inputs[0], &one, &cnt) && cnt == 1 && one == 1.0)
        side = j, sub = &m.nodes[si->second];
    }
    if (!sub) return false;
    auto rm = std::make_shared<RowMask>();
    rm->at = &add;
    rm->mode = kRowMaskAdd;
    rm->fill = row_mask_fill(add, mul.inputs[size_t(1 - side)], true);
    if (const std::string why = trace_row_mask(sub->inputs[1], rm.get()); !why.empty()) bad_form(add, why);
    if (rm->state == 1) bad_form(add, "(1 - Equal(source, c)) * fill puts the fill on the keys that differ from c; write Not(Equal(...)) or mask the equal ones with Where");
    rm->nodes.push_back(graph->producer_of.at(mul.inputs[size_t(side)]));
    rm->nodes.push_back(pi->second);
    if (!am.mask.empty() || am.rm) bad_form(add, "a row mask and another mask on one attention (causal and padding masks together are not supported)");
    am.rm = std::move(rm);
    return true;
  }
  // Where(masked, b, scores) or Where(kept, scores, b) (masked_fill)
  void Lowerer::match_where_row_mask(const NodeDef &wh, const std::string &scores, AttnMatch &am) {
    const bool scores_last = wh.inputs[2] == scores;
    auto rm = std::make_shared<RowMask>();
    rm->at = &wh;
    rm->mode = kRowMaskReplace;
    rm->fill = row_mask_fill(wh, wh.inputs[scores_last ? 1 : 2], false);
    if (const std::string why = trace_row_mask(wh.inputs[0], rm.get()); !why.empty()) bad_form(wh, why);
    if (rm->state == 0) {  // the mask itself as the condition (a Cast to bool): true = kept
      if (scores_last) bad_form(wh, "the condition is the mask itself, so the fill would land on the kept keys");
    } else if ((rm->state == 1) != scores_last) {
      bad_form(wh, "the condition is true at the kept keys, so the fill would land on them");
    }
    if (!am.mask.empty() || am.rm) bad_form(wh, "a row mask and another mask on one attention (causal and padding masks together are not supported)");
    am.rm = std::move(rm);
  }

  void Lowerer::find_attention() {
    const size_t N = m.nodes.size();
    const std::vector<char> &live = graph->live;
    const std::set<std::string> &graph_outs = graph->graph_outs;
    auto is_const = [&](const std::string &v) { return graph->row_data.count(v) == 0; };
    auto perm_of = [&](const NodeDef &t) {
      std::vector<int64_t> p;
      if (auto *q = t.attr_ints("perm")) p = *q;
      return p;
    };
    auto sole_reader = [&](const std::string &v) { return graph->sole_reader(v, false); };
    auto producer = [&](const std::string &v) { return graph->producer(v); };
    const std::string generic = "MatMul of two activations outside a recognised self-attention pattern (Reshape [N,T,h,dh] -> Transpose(0,2,1,3), Q K^T, "
                                "scale, constant mask, Softmax(-1), P V, Transpose(0,2,1,3) -> Reshape [N,T,E]); the right operand must otherwise be a constant weight matrix";
    for (size_t qi = 0; qi < N; qi++) {
      const NodeDef &qk = m.nodes[qi];
      if (!live[qi] || qk.op != "MatMul" || !(qk.domain.empty() || qk.domain == "ai.onnx") || qk.inputs.size() != 2 || is_const(qk.inputs[0]) || is_const(qk.inputs[1])) continue;
      if (absorbed[qi] || interact_at.count(qi)) continue;  // (the P V product of a pattern already matched; T . T^T of an Interact step)
      AttnMatch am;
      am.qk = &qk;
      am.nodes.push_back(qi);
      std::string why;
      // constant scalar Mul / Div hops towards the producer: v = the value behind them
      auto strip_scales = [&](std::string v) {
        for (;;) {
          const NodeDef *p = producer(v);
          if (!p || (p->op != "Mul" && p->op != "Div") || p->inputs.size() != 2 || sole_reader(v) == nullptr) return v;
          const bool c0 = is_const(p->inputs[0]), c1 = is_const(p->inputs[1]);
          if (c0 == c1 || (p->op == "Div" && c0)) return v;
          am.scales.push_back({p->op == "Mul" ? '*' : '/', p->inputs[c0 ? 0 : 1]});
          am.nodes.push_back(graph->producer_of.at(v));
          v = p->inputs[c0 ? 1 : 0];
        }
      };
      // one operand back to its head split; kt: the K^T operand
      auto match_head = [&](const std::string &operand, AttnSide &side, bool kt) -> bool {
        std::string v = strip_scales(operand);
        if (!sole_reader(v)) return why = generic, false;
        // (a rotary embedding on the head-major value, lower_rotary.cpp: the split is looked for behind it, and its readers are the embedding's)
        std::shared_ptr<const RotaryMatch> rot;
        v = behind_rotary(v, &rot);
        const NodeDef *t = producer(v);
        if (!t || t->op != "Transpose") return why = generic, false;
        std::vector<int64_t> perm = perm_of(*t);
        if (perm.size() == 3)
          return why = "PyTorch nn.MultiheadAttention's time-major export (heads folded into the row axis, [T, N*h, dh]) is not supported yet; "
                       "export batch-first projections with the head split Reshape [N,T,h,dh] -> Transpose(0,2,1,3)", false;
        if (perm == std::vector<int64_t>{2, 0, 3, 1, 4})
          return why = "the packed head split [N,T,3,h,dh] -> Transpose(2,0,3,1,4) is not supported yet; split Q, K and V on the last axis first", false;
        am.nodes.push_back(graph->producer_of.at(v));
        if (kt && perm == std::vector<int64_t>{0, 1, 3, 2}) {  // (0,2,1,3) first, then the last two axes
          v = strip_scales(t->inputs[0]);
          if (!sole_reader(v)) return why = generic, false;
          if (!rot) v = behind_rotary(v, &rot);
          t = producer(v);
          if (!t || t->op != "Transpose" || perm_of(*t) != std::vector<int64_t>{0, 2, 1, 3}) return why = generic, false;
          am.nodes.push_back(graph->producer_of.at(v));
        } else if (perm != (kt ? std::vector<int64_t>{0, 2, 3, 1} : std::vector<int64_t>{0, 2, 1, 3})) {
          return why = generic, false;
        }
        v = t->inputs[0];
        const NodeDef *r = producer(v);
        if (!r || r->op != "Reshape" || r->inputs.size() != 2 || !sole_reader(v)) {
          if (r && r->op == "Transpose" && perm_of(*r) == std::vector<int64_t>{2, 0, 3, 1, 4})
            return why = "the packed head split [N,T,3,h,dh] -> Transpose(2,0,3,1,4) is not supported yet; split Q, K and V on the last axis first", false;
          return why = generic, false;
        }
        am.nodes.push_back(graph->producer_of.at(v));
        if (rot) am.nodes.insert(am.nodes.end(), rot->nodes.begin(), rot->nodes.end());
        side.rot = rot;
        side.src = r->inputs[0];
        side.shape = r->inputs[1];
        const NodeDef *c = producer(side.src);
        if (c && (c->op == "Split" || c->op == "Slice") && (c->domain.empty() || c->domain == "ai.onnx")) {
          int64_t axis = -100;
          if (c->op == "Split") axis = c->attr_i("axis", 0);
          else if (c->inputs.size() >= 4 && is_const(c->inputs[3])) {
            auto ci = m.initializers.find(c->inputs[3]);
            if (ci != m.initializers.end() && ci->second->dtype == onnx::kInt64 && ci->second->i64.size() == 1) axis = ci->second->i64[0];
          }
          if (axis == 2 || axis == -1) {
            side.cut = c;
            side.cut_out = size_t(std::find(c->outputs.begin(), c->outputs.end(), side.src) - c->outputs.begin());
            side.src = c->inputs[0];
            am.nodes.push_back(graph->producer_of.at(r->inputs[0]));
          }
        }
        return true;
      };
      bool ok = true;
      // forward: scale / mask hops, Softmax, P V, merge
      std::string cur = qk.outputs[0];
      const NodeDef *sm = nullptr;
      while (ok && !sm) {
        const NodeDef *c = sole_reader(cur);
        size_t ci = c ? graph->consumers_of.at(cur)[0] : 0;
        if (!c && !graph_outs.count(cur) && graph->consumers_of.count(cur)) {  // a Where beside the Shape nodes that size its condition's Expand
          std::set<size_t> others;
          for (size_t r : graph->consumers_of.at(cur))
            if (m.nodes[r].op != "Shape") others.insert(r);
          if (others.size() == 1 && m.nodes[*others.begin()].op == "Where") c = &m.nodes[*others.begin()], ci = *others.begin();
        }
        if (!c || !(c->domain.empty() || c->domain == "ai.onnx")) { ok = false; why = generic; break; }
        if (c->op == "Where" && c->inputs.size() == 3 && c->inputs[0] != cur && (c->inputs[1] == cur) != (c->inputs[2] == cur)) {
          match_where_row_mask(*c, cur, am);
          am.nodes.push_back(ci);
          cur = c->outputs[0];
        } else if ((c->op == "Mul" || c->op == "Div" || c->op == "Add") && c->inputs.size() == 2) {
          const bool left = c->inputs[0] == cur;
          const std::string &other = c->inputs[left ? 1 : 0];
          if (!is_const(other) && c->op == "Add" && match_add_row_mask(*c, other, am)) {
            am.nodes.push_back(ci);
            cur = c->outputs[0];
            continue;
          }
          if (!is_const(other)) {
            ok = false;
            why = c->op == "Add" ? "the attention mask '" + other + "' is not a constant (a mask computed in the graph or depending on the row is not supported)"
                                 : "the scale '" + other + "' of the attention scores is not a constant (a scale computed from the rows is not supported)";
            break;
          }
          if (c->op == "Add") {
            if (!am.mask.empty()) { ok = false; why = "more than one mask is added to the attention scores"; break; }
            if (am.rm) bad_form(*c, "a row mask and a constant mask on one attention (causal and padding masks together are not supported)");
            am.mask = other;
          } else {
            if (c->op == "Div" && !left) { ok = false; why = generic; break; }
            am.scales.push_back({c->op == "Mul" ? '*' : '/', other});
          }
          am.nodes.push_back(ci);
          cur = c->outputs[0];
        } else if (c->op == "Softmax") {
          const int64_t axis = c->attr_i("axis", m.opset >= 13 ? -1 : 1);
          if (axis != -1 && axis != 3) {
            ok = false;
            why = "Softmax over axis " + std::to_string(axis) + " inside an attention pattern: only the key axis (-1) is supported";
            break;
          }
          sm = c;
          am.nodes.push_back(ci);
        } else {
          ok = false;
          why = generic;
        }
      }
      size_t anchor = 0;
      if (ok) {
        const NodeDef *pv = sole_reader(sm->outputs[0]);
        if (!pv || pv->op != "MatMul" || pv->inputs.size() != 2 || pv->inputs[0] != sm->outputs[0] || is_const(pv->inputs[1])) ok = false, why = generic;
        if (ok) {
          am.nodes.push_back(graph->consumers_of.at(sm->outputs[0])[0]);
          ok = match_head(pv->inputs[1], am.side[2], false);
        }
        if (ok) {
          const NodeDef *t = sole_reader(pv->outputs[0]);
          if (!t || t->op != "Transpose" || perm_of(*t) != std::vector<int64_t>{0, 2, 1, 3}) ok = false, why = generic;
          else {
            am.nodes.push_back(graph->consumers_of.at(pv->outputs[0])[0]);
            const NodeDef *r = sole_reader(t->outputs[0]);
            if (!r || r->op != "Reshape" || r->inputs.size() != 2 || r->inputs[0] != t->outputs[0]) ok = false, why = generic;
            else anchor = graph->consumers_of.at(t->outputs[0])[0];
          }
        }
      }
      ok = ok && match_head(qk.inputs[0], am.side[0], false) && match_head(qk.inputs[1], am.side[1], true);
      // (nothing else serves a product of two activations, so the load fails here, naming this node, rather than at whichever
      // Transpose / Split of the unrecognised pattern the walk would meet first)
      if (!ok && (why.empty() || why == generic)) {
        // the two export forms named as not supported yet, wherever their Transpose sits behind the operands of Q K^T
        for (const std::string &operand : qk.inputs) {
          std::string v = operand;
          for (int hop = 0; hop < 12; hop++) {
            const NodeDef *p = producer(v);
            if (!p || p->inputs.empty()) break;
            if (p->op == "Transpose") {
              const std::vector<int64_t> perm = perm_of(*p);
              if (perm == std::vector<int64_t>{2, 0, 3, 1, 4})
                why = "the packed head split [N,T,3,h,dh] -> Transpose(2,0,3,1,4) is not supported yet; split Q, K and V on the last axis first";
              else if (perm.size() == 3 && why.find("packed") == std::string::npos)
                why = "PyTorch nn.MultiheadAttention's time-major export (heads folded into the row axis, [T, N*h, dh]) is not supported yet; "
                      "export batch-first projections with the head split Reshape [N,T,h,dh] -> Transpose(0,2,1,3)";
            }
            v = p->inputs[0];
          }
        }
      }
      if (!ok) unsupported(qk, "unsupported operator form: " + (why.empty() ? generic : why));
      for (size_t i : am.nodes) absorbed[i] = 1;
      attn_at[anchor] = std::move(am);
    }
    // a Split / Slice stays absorbed only when patterns read all of it
    for (auto &kv : attn_at)
      for (const AttnSide &sd : kv.second.side) {
        if (!sd.cut) continue;
        for (const auto &o : sd.cut->outputs) {
          auto it = graph->consumers_of.find(o);
          bool all = !graph_outs.count(o);
          if (it != graph->consumers_of.end())
            for (size_t c : it->second) all = all && absorbed[c];
          if (!all) absorbed[size_t(sd.cut - m.nodes.data())] = 0;
        }
      }
    find_masked_means();
    // The nodes of the mask sub-graphs emit nothing.  The mask value may feed every layer (exporters compute it once), so a node counts
    // once; what a node reads is read by the steps from the input buffer itself (a mask input nothing else reads gets no SliceCols).
    std::set<size_t> rm_nodes, rm_aux;
    auto collect = [&](const RowMask &r) {
      rm_nodes.insert(r.nodes.begin(), r.nodes.end());
      rm_aux.insert(r.aux.begin(), r.aux.end());
    };
    for (auto &kv : attn_at)
      if (kv.second.rm) collect(*kv.second.rm);
    for (auto &kv : mmean_at) collect(kv.second.rm);
    for (size_t i : rm_nodes) absorbed[i] = 1;
    for (size_t i : rm_aux) absorbed[i] = 1;
    auto readers_absorbed = [&](size_t i) {
      bool all = true;
      for (const auto &o : m.nodes[i].outputs) {
        all = all && !graph_outs.count(o);
        if (auto it = graph->consumers_of.find(o); it != graph->consumers_of.end())
          for (size_t c : it->second) all = all && (absorbed[c] || mmean_at.count(c));  // (the closing Div emits the step)
      }
      return all;
    };
    for (auto it = rm_aux.rbegin(); it != rm_aux.rend(); ++it)
      if (!rm_nodes.count(*it) && !readers_absorbed(*it)) absorbed[*it] = 0;  // (a Shape something else reads too is lowered for that reader)
    for (auto it = rm_nodes.rbegin(); it != rm_nodes.rend(); ++it)
      if (!readers_absorbed(*it)) bad_form(m.nodes[*it], "this node of a row mask's sub-graph also feeds nodes outside the attention / masked mean patterns");
    rm_nodes.insert(rm_aux.begin(), rm_aux.end());
    for (size_t i : rm_nodes) {
      if (!absorbed[i]) continue;
      for (const auto &in : m.nodes[i].inputs)
        if (!in.empty()) uses[in]--;
      region[i] = 0;
    }
  }

  // The masked mean over time (the sentence-embedding head): Div(ReduceSum(Mul(x, m), 1), Clip(ReduceSum(m or mask, 1), min = c)) with
  // m = float(mask [N, T, 1]), traced like an attention's row mask, becomes ONE MeanTime step with a row mask (lower_masked_mean)
  void Lowerer::find_masked_means() {
    auto sum_over_time = [&](const NodeDef &r) {
      std::vector<int64_t> ax;
      return r.op == "ReduceSum" && graph->std_dom(r) && !r.inputs.empty() && graph_ints_arg(r, 1, "axes", &ax) && ax == std::vector<int64_t>{1};
    };
    auto made_by = [&](const std::string &v) { return graph->producer(v); };
    auto idx = [&](const NodeDef *n) { return size_t(n - m.nodes.data()); };
    for (size_t i = 0; i < m.nodes.size(); i++) {
      const NodeDef &mul = m.nodes[i];
      if (!graph->live[i] || absorbed[i] || mul.op != "Mul" || !graph->std_dom(mul) || mul.inputs.size() != 2 || mul.outputs.empty()) continue;
      const NodeDef *rs = only_reader(mul.outputs[0]);
      if (!rs || !sum_over_time(*rs) || rs->attr_i("keepdims", 1) != 0 || rs->inputs[0] != mul.outputs[0]) continue;
      const NodeDef *div = only_reader(rs->outputs[0]);
      if (!div || div->op != "Div" || !graph->std_dom(*div) || div->inputs.size() != 2 || div->inputs[0] != rs->outputs[0]) continue;
      const NodeDef *clip = made_by(div->inputs[1]);
      if (!clip || clip->op != "Clip" || !graph->std_dom(*clip) || only_reader(clip->outputs[0]) != div) continue;
      MaskedMean mm;
      double lo = 0;
      size_t cnt = 0;
      if (has_input(*clip, 2)) continue;
      if (has_input(*clip, 1)) {
        if (!graph_const_scalar(clip->inputs[1], &lo, &cnt) || cnt != 1) continue;
      } else if (clip->attr("min") && !clip->attr("max")) {
        lo = double(clip->attr_f("min", 0.f));
      } else {
        continue;
      }
      int side = -1;
      for (int j = 0; j < 2 && side < 0; j++) {
        RowMask r;
        if (graph->row_data.count(mul.inputs[size_t(1 - j)]) && trace_row_mask(mul.inputs[size_t(j)], &r).empty() && r.state != 1 && r.shape.size() == 3 && r.shape[2] == 1)
          side = j, mm.rm = std::move(r);
      }
      if (side < 0) continue;
      // from here on the pattern is a masked mean, served or refused in its own words
      std::vector<size_t> tail{i, idx(rs), idx(clip)};
      const NodeDef *cs = made_by(clip->inputs[0]);
      if (cs && cs->op == "Cast" && only_reader(cs->outputs[0]) == clip) tail.push_back(idx(cs)), cs = made_by(cs->inputs[0]);
      RowMask cr;
      if (!cs || !sum_over_time(*cs) || !only_reader(cs->outputs[0])) bad_form(*div, "the divisor of a masked mean must be Clip(ReduceSum(mask, axis 1), min = c)");
      if (const std::string why = trace_row_mask(cs->inputs[0], &cr); !why.empty()) bad_form(*div, why);
      if (cr.src0 != mm.rm.src0 || cr.k != mm.rm.k || cr.state == 1 || cr.cmp != mm.rm.cmp || (cr.state == 0) != (mm.rm.state == 0))
        bad_form(*div, "the divisor of a masked mean counts another mask than the one that multiplies the window");
      if (!(lo > 0) || !std::isfinite(lo)) bad_form(*clip, "the lower bound of a masked mean's count must be a positive finite constant");
      tail.push_back(idx(cs));
      mm.rm.nodes.insert(mm.rm.nodes.end(), cr.nodes.begin(), cr.nodes.end());
      mm.rm.aux.insert(mm.rm.aux.end(), cr.aux.begin(), cr.aux.end());
      mm.rm.nodes.insert(mm.rm.nodes.end(), tail.begin(), tail.end());
      mm.rm.at = div;
      mm.x = mul.inputs[size_t(1 - side)];
      mm.clip = float(lo);
      mm.mul = i;
      mmean_at[idx(div)] = std::move(mm);
    }
  }
  void Lowerer::lower_masked_mean(const MaskedMean &mm, const NodeDef &div) {
    const Val *x = find_value(mm.x);
    if (!x) bad_form(div, "the window '" + mm.x + "' of the masked mean is produced by no earlier node");
    if (x->pv) materialize(mm.x, &div), x = find_value(mm.x);
    if (x->is_const || x->ra != 0 || x->shape.size() != 3 || x->padded() || x->buf < 0)
      bad_form(div, "the masked mean reads " + shape_str(x->shape) + (x->ra ? " (time-major)" : "") + "; only a rows-first window [N, T, E]");
    const int64_t T = x->shape[1], E = x->shape[2];
    if (mm.rm.k != T) bad_form(div, "the row mask has T = " + std::to_string(mm.rm.k) + ", the window T = " + std::to_string(T));
    if (plan.input_declared_type == "float16") bad_form(div, "a row mask taken from a float16 graph input");
    Step s;
    s.kind = StepKind::MeanTime;
    s.in0 = x->buf;
    s.rep = T;
    s.K = E;
    s.in3 = 0;
    s.rm_off = mm.rm.src0;
    s.rm_cmp = mm.rm.cmp;
    s.rm_int = mm.rm.is_int;
    s.rm_clip = mm.clip;
    s.origin = node_label(m.nodes[mm.mul]) + "+...+" + node_label(div);
    emit_window(std::move(s), div, {x->shape[0], E});
  }

  const Val *Lowerer::find_value(const std::string &name) {
    auto it = vals.find(name);
    if (it != vals.end()) {
      if (it->second.nn) materialize_nearest(name);
      return &it->second;
    }
    auto ci = m.initializers.find(name);
    if (ci != m.initializers.end()) return &(vals[name] = const_val(ci->second));
    return nullptr;
  }

  void Lowerer::lower_attention(const AttnMatch &am, const NodeDef &anchor) {
    const NodeDef &qk = *am.qk;
    auto bad = [&](const std::string &why) { unsupported(qk, "unsupported operator form: " + why); };
    static const char *names[3] = {"Q", "K", "V"};
    struct View {
      int buf;
      int64_t N, T, E, ld, off;
    } vw[3];
    int64_t heads = 0, dh = 0, kv_heads = 0, split_h[3] = {0, 0, 0};  // split_h: the heads each operand's own split gives it
    const NodeDef *op = am.op;  // the Attention operator (lower_attention_op.cpp); null: the pattern form
    for (int i = 0; i < 3; i++) {
      const AttnSide &sd = am.side[i];
      const Val *src = find_value(sd.src);
      if (!src) bad(std::string(names[i]) + " reads '" + sd.src + "', which no earlier node produces");
      if (src->pv) materialize(sd.src, &qk), src = find_value(sd.src);
      if (src->is_const || src->ra != 0 || src->shape.size() != 3 || src->padded())
        bad(std::string(names[i]) + " must be a rows-first [N, T, E] activation, got " + shape_str(src->shape) + (src->ra ? " (time-major)" : ""));
      View &v = vw[i];
      v = {src->buf, src->shape[0], src->shape[1], src->shape[2], src->shape[2], 0};
      if (sd.cut && !absorbed[size_t(sd.cut - m.nodes.data())]) bad("the " + sd.cut->op + " that feeds " + names[i] + " also feeds nodes outside the attention pattern");
      if (sd.cut && sd.cut->op == "Split") {
        const NodeDef &c = *sd.cut;
        std::vector<int64_t> sizes;
        if (has_input(c, 1)) sizes = const_ints(c, 1, "split");
        else if (auto *p = c.attr_ints("split")) sizes = *p;
        const int64_t nout = int64_t(c.outputs.size());
        if (sizes.empty()) {
          const int64_t parts = c.attr_i("num_outputs", nout), each = (v.ld + parts - 1) / parts;
          for (int64_t k = 0; k < parts; k++) sizes.push_back(std::min(each, v.ld - k * each));
        }
        if (int64_t(sizes.size()) != nout || std::accumulate(sizes.begin(), sizes.end(), int64_t(0)) != v.ld) unsupported(c, "split sizes do not cover the axis");
        for (int64_t s : sizes)
          if (s <= 0) unsupported(c, "empty split piece");
        v.off = std::accumulate(sizes.begin(), sizes.begin() + int64_t(sd.cut_out), int64_t(0));
        v.E = sizes[sd.cut_out];
      } else if (sd.cut) {
        const NodeDef &c = *sd.cut;
        const std::vector<int64_t> st = const_ints(c, 1, "starts"), en = const_ints(c, 2, "ends");
        if (st.size() != 1 || en.size() != 1 || (has_input(c, 4) && const_ints(c, 4, "steps") != std::vector<int64_t>{1})) unsupported(c, "one axis, step 1");
        int64_t b = st[0] < 0 ? st[0] + v.ld : st[0], e = en[0] < 0 ? en[0] + v.ld : en[0];
        b = std::clamp<int64_t>(b, 0, v.ld);
        e = std::clamp<int64_t>(e, b, v.ld);
        if (e == b) unsupported(c, "empty slice");
        v.off = b;
        v.E = e - b;
      }
      if (op && am.form3) {  // the 3-D operands of the operator: the head counts are its attributes
        const int64_t h = op->attr_i(i == 0 ? "q_num_heads" : "kv_num_heads", 0);
        if (h < 1 || v.E % h != 0) bad("E = " + std::to_string(v.E) + " of " + names[i] + " is not divisible by " + (i == 0 ? "q_num_heads" : "kv_num_heads") + " = " + std::to_string(h));
        if (i == 0) heads = h, dh = v.E / h;
        else if (i == 1) kv_heads = h;
        if (i == 1 && v.E / h != dh) bad("K has heads of " + std::to_string(v.E / h) + " columns, Q of " + std::to_string(dh));
        if (i == 2 && v.E / h != dh) bad("v_head_size = " + std::to_string(v.E / h) + " differs from head_size = " + std::to_string(dh));
        continue;
      }
      // the head split [N, T, h, dh]
      const Val *sh = find_value(sd.shape);
      if (!sh || !sh->is_const || sh->c->dtype != onnx::kInt64) bad("the head split of " + std::string(names[i]) + " needs a constant target shape");
      std::vector<int64_t> tgt = sh->c->i64;
      if (tgt.size() != 4) bad("the head split of " + std::string(names[i]) + " must reshape to [N, T, h, dh], got a target of " + std::to_string(tgt.size()) + " entries");
      if (tgt[1] == 0) tgt[1] = v.T;
      if (tgt[2] == 0) tgt[2] = v.E;
      int neg = -1;
      for (int k = 1; k < 4; k++) {
        if (tgt[size_t(k)] == -1 && neg < 0) neg = k;
        else if (tgt[size_t(k)] <= 0) bad("the head split of " + std::string(names[i]) + " has the extent " + std::to_string(tgt[size_t(k)]) + " in " + shape_str(sh->c->i64));
      }
      if (!(tgt[0] == 0 || tgt[0] == -1 || (tgt[0] == v.N && v.N > 0)) || (tgt[0] == -1 && neg >= 0))
        bad("the head split target " + shape_str(sh->c->i64) + " does not keep the row axis");
      int64_t h = tgt[2], d = tgt[3], t = tgt[1];
      if (neg == 1) t = v.T;
      if (t != v.T) bad("the head split " + shape_str(sh->c->i64) + " of " + names[i] + " " + shape_str(src->shape) + " does not keep the T steps (heads folded over time are not supported)");
      if (neg == 2 && v.E % d == 0) h = v.E / d;
      if (neg == 3 && v.E % h == 0) d = v.E / h;
      if (h <= 0 || d <= 0 || v.E / h != d || v.E % h != 0)
        bad("E = " + std::to_string(v.E) + " is not divisible by h = " + std::to_string(tgt[2] > 0 ? tgt[2] : h) + " (head split " + shape_str(sh->c->i64) + ")");
      split_h[i] = h;
      if (i == 0) heads = h, dh = d;
      else if (op) {
        if (i == 2 && d != dh) bad("v_head_size = " + std::to_string(d) + " differs from head_size = " + std::to_string(dh));
        if (d != dh) bad("K has heads of " + std::to_string(d) + " columns, Q of " + std::to_string(dh));
        if (i == 1) kv_heads = h;
        else if (h != kv_heads) bad("V has " + std::to_string(h) + " heads, K " + std::to_string(kv_heads));
      } else if (h != heads || d != dh) bad(std::string(names[i]) + " is split into " + std::to_string(h) + " heads of " + std::to_string(d) + ", Q into " + std::to_string(heads) + " of " + std::to_string(dh));
    }
    if (op) {
      if (vw[2].T != vw[1].T) bad("K and V have different window lengths (" + std::to_string(vw[1].T) + ", " + std::to_string(vw[2].T) + ")");
      if (kv_heads < 1 || heads % kv_heads != 0)
        bad("q_num_heads = " + std::to_string(heads) + " is no multiple of kv_num_heads = " + std::to_string(kv_heads));
    } else if (vw[1].T != vw[0].T || vw[2].T != vw[0].T)
      bad("Q, K and V have different window lengths T (" + std::to_string(vw[0].T) + ", " + std::to_string(vw[1].T) + ", " + std::to_string(vw[2].T) +
          "): cross-attention is not supported");
    const int64_t N = vw[0].N, T = vw[0].T, E = vw[0].E, Tk = vw[1].T;  // (the pattern form: Tk = T)
    const bool causal = op && op->attr_i("is_causal", 0) != 0;
    if (Tk < 1 || Tk > kAttnMaxT) bad("Tk = " + std::to_string(Tk) + " is beyond the attention kernel's cap of " + std::to_string(kAttnMaxT) + " steps");
    if (T < 1 || T > kAttnMaxT) bad("T = " + std::to_string(T) + " is beyond the attention kernel's cap of " + std::to_string(kAttnMaxT) + " steps");
    if (dh > kAttnMaxDh) bad("dh = " + std::to_string(dh) + " is beyond the attention kernel's cap of " + std::to_string(kAttnMaxDh) + " columns per head");
    if (heads > kAttnMaxHeads) bad("h = " + std::to_string(heads) + " is beyond the attention kernel's cap of " + std::to_string(kAttnMaxHeads) + " heads");
    for (const View &v : vw)
      if (v.ld * std::max(T, Tk) > kMaxPerRow) bad("window too large");
    // the scale: every constant scalar Mul / Div on Q, K^T and the scores, folded into one factor applied to the f32 scores
    double scale = 1.0;
    for (const AttnScale &sc : am.scales) {
      const Val *c = find_value(sc.cst);
      if (!c || !c->is_const || c->c->dtype != onnx::kFloat || c->c->f32.size() != 1 || !(c->c->f32[0] > 0.f) || !std::isfinite(c->c->f32[0]))
        bad("the scale '" + sc.cst + "' must be one positive finite f32 constant");
      scale = sc.op == '*' ? scale * double(c->c->f32[0]) : scale / double(c->c->f32[0]);
    }
    if (op) {  // ONE f32 factor on the f32 scores: the attribute, or 1 / sqrt(dh)
      const float sc = op->attr("scale") ? op->attr_f("scale", 0.f) : float(1.0 / std::sqrt(double(dh)));
      if (!(sc > 0.f) || !std::isfinite(sc)) bad("scale must be a positive finite f32 number");
      scale = double(sc);
    }
    if (!(float(scale) > 0.f) || !std::isfinite(float(scale))) bad("the folded scale is not a positive finite f32 number");
    Step s;
    s.kind = StepKind::Attention;
    if (!am.mask.empty()) {
      const Val *c = find_value(am.mask);
      const bool bool_mask = op && c && c->is_const && c->c->elem == onnx::kBool;  // true = kept: 0, false: -inf
      if (!c || !c->is_const || (c->c->dtype != onnx::kFloat && !bool_mask)) bad("the attention mask '" + am.mask + "' must be an f32 " + (op ? "or bool " : "") + "constant");
      std::vector<float> from_bool;
      if (bool_mask)
        for (int64_t b : c->c->i64) from_bool.push_back(b ? 0.f : -INFINITY);
      const std::vector<float> &mvals = bool_mask ? from_bool : c->c->f32;
      if (op && c->shape.size() > 2 && std::any_of(c->shape.begin(), c->shape.end() - 2, [](int64_t x) { return x != 1; }))
        bad("the attention mask " + shape_str(c->shape) + " depends on the row or the head; only [Tq,Tk], [1,Tq,Tk] or [1,1,Tq,Tk]");
      std::vector<int64_t> d = c->shape;
      while (d.size() > 2 && d[0] == 1) d.erase(d.begin());
      while (d.size() < 2) d.insert(d.begin(), 1);
      if (d.size() != 2 || (d[0] != 1 && d[0] != T) || (d[1] != 1 && d[1] != Tk) || int64_t(mvals.size()) != d[0] * d[1])
        bad("the attention mask " + shape_str(c->shape) + " does not broadcast to [T, T] = [" + std::to_string(T) + "," + std::to_string(Tk) +
            "] (a mask that depends on the row or the head is not supported)");
      s.cst.resize(size_t(T * Tk));
      for (int64_t q = 0; q < T; q++) {
        bool any = false;
        for (int64_t k = 0; k < Tk; k++) {
          const float mv = mvals[size_t((d[0] == 1 ? 0 : q) * d[1] + (d[1] == 1 ? 0 : k))];
          if (std::isnan(mv) || mv == INFINITY) bad("the attention mask holds NaN or +inf");
          any = any || (mv != -INFINITY && !(causal && k > q));
          s.cst[size_t(q * Tk + k)] = mv;
        }
        if (!any) bad("row " + std::to_string(q) + " of the attention mask is -inf everywhere (a fully masked query has no softmax)");
      }
    }
    if (am.rm) {
      const RowMask &r = *am.rm;
      const NodeDef &at = *r.at;
      if (!am.mask.empty()) bad_form(at, "a row mask and a constant mask on one attention (causal and padding masks together are not supported)");
      const std::vector<int64_t> &sh = r.shape;
      if (sh.size() == 4 && sh[3] == Tk && (sh[1] != 1 || sh[2] != 1))
        bad_form(at, "the mask " + shape_str(sh) + " depends on the head or the query; only one key mask per row, [N,1,1,T]");
      if (sh.size() != 4 || sh[1] != 1 || sh[2] != 1) bad_form(at, "the row mask meets the scores as " + shape_str(sh) + "; only [N,1,1,T]");
      if (sh[3] != Tk) bad_form(at, "the row mask has T = " + std::to_string(sh[3]) + ", the attention T = " + std::to_string(Tk));
      if (plan.input_declared_type == "float16") bad_form(at, "a row mask taken from a float16 graph input");
      if (r.src0 < 0 || r.src0 + Tk > plan.buf_per_row[0]) bad_form(at, "the row mask's columns lie outside the input");
      s.in3 = 0;
      s.rm_off = r.src0;
      s.rm_cmp = r.cmp;
      s.rm_fill = r.fill;
      s.rm_mode = r.mode;
      s.rm_int = r.is_int;
      s.rm_excl = r.fill <= kRowMaskExcludingFill;
    }
    if (!(op && am.form3)) {  // the merge Reshape must give [N, T, E]
      const std::vector<int64_t> tgt = const_ints(anchor, 1, "shape");
      bool okm = tgt.size() == 3 && (tgt[0] == 0 || tgt[0] == -1 || (tgt[0] == N && N > 0)) && (tgt[1] == 0 || tgt[1] == T || tgt[1] == -1) &&
                 (tgt[2] == E || tgt[2] == -1) && !(tgt[0] == -1 && (tgt[1] == -1 || tgt[2] == -1)) && !(tgt[1] == -1 && tgt[2] == -1);
      if (!okm) bad("the merge Reshape '" + node_label(anchor) + "' must give [N, T, E] = [N," + std::to_string(T) + "," + std::to_string(E) + "], got " + shape_str(tgt));
    }
    s.attn_T = T;
    s.attn_heads = heads;
    s.attn_dh = dh;
    s.attn_scale = float(scale);
    if (op) s.attn_Tk = Tk, s.attn_kv_heads = kv_heads, s.attn_causal = causal;
    // Three window Dense projections of ONE value, each read by this pattern alone: merged into one Dense of width 3E, so the value is
    // read once and the kernel reads one packed [rows, T, 3E] buffer
    const std::set<size_t> mine(am.nodes.begin(), am.nodes.end());  // (another pattern over the same q, k, v must still find its buffers)
    auto private_proj = [&](const View &v) -> int {
      auto pit = producer.find(v.buf);
      if (v.buf <= 0 || pit == producer.end() || v.off != 0 || v.ld != E) return -1;
      const Step &p = plan.steps[size_t(pit->second)];
      if (p.kind != StepKind::Dense || p.rep != T || p.act != Act::None || p.out != v.buf || p.M != E) return -1;
      for (const auto &nm : buf_names[v.buf]) {
        if (nm == m.outputs[out_index].name) return -1;
        auto it = graph->consumers_of.find(nm);
        if (it == graph->consumers_of.end()) continue;
        for (size_t c : it->second) {  // readers: THIS pattern's nodes, Shape, and nodes folded into the step (its bias Add)
          const NodeDef &cn = m.nodes[c];
          auto ov = cn.outputs.empty() ? vals.end() : vals.find(cn.outputs[0]);
          const bool folded = ov != vals.end() && !ov->second.is_const && ov->second.buf == v.buf;
          if (!mine.count(c) && cn.op != "Shape" && !folded) return -1;
        }
      }
      return pit->second;
    };
    const int pq = private_proj(vw[0]), pk = private_proj(vw[1]), pv = private_proj(vw[2]);
    if (pq >= 0 && pk >= 0 && pv >= 0 && pq != pk && pk != pv && pq != pv && plan.steps[size_t(pq)].in0 == plan.steps[size_t(pk)].in0 &&
        plan.steps[size_t(pq)].in0 == plan.steps[size_t(pv)].in0 && plan.steps[size_t(pq)].K == plan.steps[size_t(pk)].K &&
        plan.steps[size_t(pq)].K == plan.steps[size_t(pv)].K) {
      const int idx[3] = {pq, pk, pv};
      const int64_t K = plan.steps[size_t(pq)].K;
      Step d = plan.steps[size_t(pq)];
      d.M = 3 * E;
      d.W.assign(size_t(K * 3 * E), 0.f);
      bool any_bias = false;
      for (int i : idx) any_bias = any_bias || !plan.steps[size_t(i)].bias.empty();
      d.bias.assign(any_bias ? size_t(3 * E) : 0, 0.f);
      d.origin.clear();
      for (int j = 0; j < 3; j++) {
        const Step &p = plan.steps[size_t(idx[j])];
        for (int64_t k = 0; k < K; k++) std::copy_n(p.W.begin() + k * E, E, d.W.begin() + k * 3 * E + j * E);
        if (!p.bias.empty()) std::copy(p.bias.begin(), p.bias.end(), d.bias.begin() + j * E);
        d.origin += (j ? "|" : "") + p.origin;
      }
      const int first = std::min({pq, pk, pv});
      d.out = vw[0].buf;
      plan.steps[size_t(first)] = std::move(d);
      for (int i : {std::max({pq, pk, pv}), pq + pk + pv - first - std::max({pq, pk, pv})}) plan.steps.erase(plan.steps.begin() + i);
      producer.clear();
      for (size_t i = 0; i < plan.steps.size(); i++) producer[plan.steps[i].out] = int(i);
      plan.buf_per_row[size_t(vw[0].buf)] = T * 3 * E;
      plan.buf_shape[size_t(vw[0].buf)] = {N, T * 3 * E};
      for (int j = 1; j < 3; j++) {  // the K and V buffers have no writer and no reader any more: they take no scratch
        plan.buf_per_row[size_t(vw[j].buf)] = 0;
        plan.buf_shape[size_t(vw[j].buf)] = {N, 0};
      }
      for (int j = 0; j < 3; j++) vw[j].buf = vw[0].buf, vw[j].ld = 3 * E, vw[j].off = j * E;
    }
    // A rotary embedding between a head split and the attention (lower_rotary.cpp): one Rotary step per rotated operand reads the operand's
    // view -- a cut of a packed projection where it lies -- and the attention reads its dense [N, T, h * dh] result
    for (int j = 0; j < 3; j++) {
      const std::shared_ptr<const RotaryMatch> &rot = am.side[j].rot;
      if (!rot) continue;
      bool seen = false;
      for (int i = 0; i < j && !seen; i++)
        if (am.side[i].rot && am.side[i].rot->at == rot->at) vw[j] = vw[i], seen = true;  // (one rotated value read as two operands: matched once per operand)
      if (seen) continue;
      Step r = rotary_step(*rot, vw[j].T, split_h[j], dh);
      r.in0 = vw[j].buf;
      r.attn_ld[0] = vw[j].ld, r.attn_off[0] = vw[j].off;
      const size_t first = *std::min_element(rot->nodes.begin(), rot->nodes.end());
      r.origin = rot->spelling ? node_label(m.nodes[first]) + "+...+" + node_label(*rot->at) : node_label(*rot->at);
      vw[j].buf = push_step(std::move(r), {vw[j].N, vw[j].T * vw[j].E});
      vw[j].ld = vw[j].E, vw[j].off = 0;
    }
    s.in0 = vw[0].buf;
    s.in1 = vw[1].buf;
    s.in2 = vw[2].buf;
    for (int j = 0; j < 3; j++) s.attn_ld[j] = vw[j].ld, s.attn_off[j] = vw[j].off;
    s.origin = &qk == &anchor ? node_label(qk) : node_label(qk) + "+...+" + node_label(anchor);
    emit_window(std::move(s), anchor, {N, T, E});
  }

  // Sum of any number of equal-shaped activations: a chain of residual adds
  void Lowerer::sum(const NodeDef &n) {
    if (n.inputs.empty()) unsupported(n, "no inputs");
    if (n.inputs.size() == 1) { lower_node(std_node(n, "Identity", {n.inputs[0]}, n.outputs[0])); return; }
    std::string cur = n.inputs[0];
    for (size_t i = 1; i < n.inputs.size(); i++) {
      const bool last = i + 1 == n.inputs.size();
      const std::string out = last ? n.outputs[0] : n.outputs[0] + "\x01sum" + std::to_string(i);
      if (!last) uses[out] = 1;
      lower_node(std_node(n, "Add", {cur, n.inputs[i]}, out));
      cur = out;
    }
  }
  void Lowerer::global_avgpool(const NodeDef &n, bool is_max) {
    const Val &a = get(n, 0);
    if (a.is_const || a.shape.size() < 3) unsupported(n, "bad input");
    Step s;
    s.kind = StepKind::GlobalAvgPool;
    s.is_max = is_max;
    s.in0 = a.buf;
    s.C = a.shape[1];
    s.S = prod(a.shape, 2);
    std::vector<int64_t> shape = a.shape;
    for (size_t i = 2; i < shape.size(); i++) shape[i] = 1;
    emit(std::move(s), n, shape);
  }

  // ------------------------------------------------------------------------------------------
  // Quantised graphs.  A QuantizeLinear of an activation emits nothing: its output is a quantised value over the
  // same buffer (Val::q).  DequantizeLinear of a constant folds to f32 and remembers its integers; of a quantised activation it becomes
  // a FakeQuant step -- or the output quantisation of the QDense step in front of it.  MatMul / Gemm between a FakeQuant (or a
  // quantised QDense) and dequantised int8 weights, and QLinearMatMul, become QDense.
  [[noreturn]] void Lowerer::bad_form(const NodeDef &n, const std::string &why) { unsupported(n, "unsupported operator form: " + why); }

  Lowerer::QArgs Lowerer::quant_args(const NodeDef &n, size_t si, size_t zi, const char *what) {
    QArgs qa;
    if (n.attr_i("block_size", 0) != 0) bad_form(n, "block_size (blocked quantisation) is not supported");
    const Val &sv = get(n, si);
    if (!sv.is_const) bad_form(n, std::string("the ") + what + " scale is not a constant");
    if (sv.c->dtype != onnx::kFloat) bad_form(n, std::string("the ") + what + " scale must be f32");
    qa.scale = sv.c->f32;
    if (qa.scale.empty()) bad_form(n, std::string("the ") + what + " scale is empty");
    for (float v : qa.scale)
      if (!std::isfinite(v) || !(v > 0.f)) bad_form(n, std::string("the ") + what + " scale must be finite and positive");
    if (has_input(n, zi)) {
      const Val &zv = get(n, zi);
      if (!zv.is_const) bad_form(n, std::string("the ") + what + " zero point is not a constant");
      if (zv.c->elem != onnx::kUint8 && zv.c->elem != onnx::kInt8 && zv.c->elem != onnx::kInt32)
        bad_form(n, std::string("the ") + what + " zero point has element type " + std::to_string(zv.c->elem) + "; only uint8, int8 (and int32 for a bias) are supported");
      if (zv.c->i64.size() != qa.scale.size()) bad_form(n, std::string("the ") + what + " scale and zero point differ in size");
      qa.zp = zv.c->i64;
      qa.elem = zv.c->elem;
    } else {
      qa.zp.assign(qa.scale.size(), 0);
    }
    return qa;
  }
  Quant Lowerer::act_quant(const NodeDef &n, const QArgs &qa, const char *what) {
    if (qa.scale.size() != 1) bad_form(n, std::string("per-axis quantisation of an activation (") + what + ") is not supported");
    if (qa.elem != onnx::kUint8 && qa.elem != onnx::kInt8) bad_form(n, std::string(what) + " has element type " + std::to_string(qa.elem) + "; only uint8 and int8 are supported");
    Quant q;
    q.on = true;
    q.scale = qa.scale[0];
    q.zp = int(qa.zp[0]);
    q.is_signed = qa.elem == onnx::kInt8;
    return q;
  }

  void Lowerer::set_quant(const NodeDef &n, int buf, const std::vector<int64_t> &shape, int ra, const Quant &q, bool done, bool folded) {
    set_act(n, buf, shape, folded, ra);
    Val &v = vals[n.outputs[0]];
    v.q = std::make_shared<const Quant>(q);
    v.q_done = done;
    quant_node[n.outputs[0]] = &n;
  }

  void Lowerer::quantize_linear(const NodeDef &n) {
    const Val x = get(n, 0);
    if (x.is_const) bad_form(n, "quantising a constant is not supported");
    if (x.q) bad_form(n, "the input is a quantised tensor already");
    if (auto *a = n.attr("output_dtype"); a && a->i != 0 && a->i != onnx::kUint8 && a->i != onnx::kInt8)
      bad_form(n, "output_dtype " + std::to_string(a->i) + "; only uint8 and int8 are supported");
    const Quant q = act_quant(n, quant_args(n, 1, 2, "activation"), "the activation");
    set_quant(n, x.buf, x.shape, x.ra, q, false, true);
  }

  void Lowerer::dequantize_linear(const NodeDef &n) {
    const Val x = get_raw(n, 0);
    if (x.pv) bad_form(n, "the input is not a quantised tensor");
    const QArgs qa = quant_args(n, 1, 2, x.is_const ? "constant's" : "activation");
    if (x.is_const) {
      const TensorData &t = *x.c;
      if (t.elem != onnx::kUint8 && t.elem != onnx::kInt8 && t.elem != onnx::kInt32)
        bad_form(n, "the data has element type " + std::to_string(t.elem) + "; only uint8, int8 (and int32 for a bias) are supported");
      if (has_input(n, 2) && qa.elem != t.elem) bad_form(n, "the zero point's element type differs from the data's");
      int64_t axis = n.attr_i("axis", 1);
      const int64_t rank = int64_t(t.dims.size());
      int64_t outer = 1, len = 1, inner = int64_t(t.i64.size());
      if (qa.scale.size() > 1) {
        if (axis < 0) axis += rank;
        if (axis < 0 || axis >= rank || int64_t(qa.scale.size()) != t.dims[size_t(axis)]) bad_form(n, "the scale does not match the axis it quantises");
        len = t.dims[size_t(axis)];
        inner = prod(t.dims, size_t(axis) + 1);
        outer = prod(t.dims, 0, size_t(axis));
      }
      auto out = std::make_shared<TensorData>();
      out->dtype = out->elem = onnx::kFloat;
      out->dims = t.dims;
      out->f32.resize(t.i64.size());
      for (int64_t o = 0; o < outer; o++)
        for (int64_t j = 0; j < len; j++)
          for (int64_t i = 0; i < inner; i++) {
            const size_t at = size_t((o * len + j) * inner + i);
            out->f32[at] = float(t.i64[at] - qa.zp[size_t(qa.scale.size() > 1 ? j : 0)]) * qa.scale[size_t(qa.scale.size() > 1 ? j : 0)];
          }
      out->q_data = x.c;
      out->q_scale = qa.scale;
      out->q_zp = qa.zp;
      out->q_axis = axis;
      vals[n.outputs[0]] = const_val(std::move(out));
      return;
    }
    if (!x.q) bad_form(n, "the input is not a quantised tensor");
    const Quant q = act_quant(n, qa, "the activation");
    if (!(q == *x.q)) bad_form(n, "it dequantises with another scale, zero point or type than the tensor was quantised with");
    if (x.q_done) {  // a QLinearMatMul's result: the buffer holds these values already
      set_act(n, x.buf, x.shape, true, x.ra);
      return;
    }
    if (Step *p = fusable_producer(n, 0); p && quantised_layer(*p) && !p->qy.on && (p->act == Act::None || p->act == Act::Relu || p->act == Act::Clip)) {
      p->qy = q;
      qdense_canonical_act(*p);
      p->origin += "+" + node_label(n);
      set_act(n, x.buf, x.shape, true, x.ra);
      return;
    }
    Step s;
    s.kind = StepKind::FakeQuant;
    s.in0 = x.buf;
    s.qx = q;
    if (x.ra != 0) bad_form(n, "quantisation of a time-major value");
    emit(std::move(s), n, x.shape);
  }

  // QDense and QConv2d share their quantisation fields and the helpers below
  bool Lowerer::quantised_layer(const Step &s) { return s.kind == StepKind::QDense || s.kind == StepKind::QConv2d; }

  // A Relu in front of a quantisation whose range starts at 0 (zp == qmin) changes nothing: sat() does the same.  Dropping it makes
  // the QDQ spelling (which writes the Relu) and the QLinear spelling (which cannot) one plan.
  void Lowerer::qdense_canonical_act(Step &s) {
    if (s.qy.on && s.act == Act::Relu && s.qy.zp == s.qy.qmin()) s.act = Act::None;
  }

  void Lowerer::qdense_check_k(const NodeDef &n, const Step &s) {
    int64_t mb = 0;
    for (int32_t b : s.q_bias) mb = std::max<int64_t>(mb, std::llabs(int64_t(b)));
    if (!qdense_k_fits(s.K, mb))
      bad_form(n, "K = " + std::to_string(s.K) + " is beyond the cap of the int32 accumulator (K * 255 * 255 + max|bias| must stay below 2^31)");
  }

  // the bias of a QDense step: DequantizeLinear(int32, scale = x_scale * w_scale[m], zero point 0) is added to the accumulator as it
  // is; any other f32 constant after the scaling
  void Lowerer::qdense_take_bias(const NodeDef &n, Step &s, const Val &c) {
    const auto &cv = cf32(n, c);
    const TensorData &t = *c.c;
    bool as_int = t.q_data && t.q_data->elem == onnx::kInt32 && int64_t(t.q_data->i64.size()) == s.M && (t.q_scale.size() == 1 || int64_t(t.q_scale.size()) == s.M);
    for (int64_t j = 0; as_int && j < s.M; j++) {
      const size_t qi = t.q_scale.size() == 1 ? 0 : size_t(j);
      const int64_t v = t.q_data->i64[size_t(j)];
      as_int = t.q_zp[qi] == 0 && t.q_scale[qi] == s.q_mult[size_t(j)] && v >= INT32_MIN && v <= INT32_MAX;
    }
    if (as_int) {
      s.q_bias.resize(size_t(s.M));
      for (int64_t j = 0; j < s.M; j++) s.q_bias[size_t(j)] = int32_t(t.q_data->i64[size_t(j)]);
      qdense_check_k(n, s);
    } else {
      s.bias = cv;
    }
  }

  // the QDense step of X[.., K] (quantised as xq) times the integer matrix `w` ([K, M], or [M, K] under trans) with scales ws and zero
  // points wz (one, or M of them)
  Step Lowerer::make_qdense(const NodeDef &n, int in_buf, int64_t rep, const TensorData &w, bool trans, const std::vector<float> &ws, const std::vector<int64_t> &wz,
                            const Quant &xq) {
    if (w.elem != onnx::kUint8 && w.elem != onnx::kInt8) bad_form(n, "the weights have element type " + std::to_string(w.elem) + "; only uint8 and int8 are supported");
    if (w.dims.size() != 2) bad_form(n, "the weights must be a [K, M] matrix");
    Step s;
    s.kind = StepKind::QDense;
    s.in0 = in_buf;
    s.K = trans ? w.dims[1] : w.dims[0];
    s.M = trans ? w.dims[0] : w.dims[1];
    s.rep = rep;
    take_quant_weights(n, s, w, trans, ws, wz, xq);
    return s;
  }
  // the quantisation fields of a QDense / QConv2d step whose K and M are set: `w` holds K * M integers as [K, M] (or [M, K] under trans: a
  // Gemm's transB, a convolution's [M, C, kh, kw])
  void Lowerer::take_quant_weights(const NodeDef &n, Step &s, const TensorData &w, bool trans, const std::vector<float> &ws, const std::vector<int64_t> &wz, const Quant &xq) {
    if (w.elem != onnx::kUint8 && w.elem != onnx::kInt8) bad_form(n, "the weights have element type " + std::to_string(w.elem) + "; only uint8 and int8 are supported");
    const int64_t K = s.K, M = s.M;
    if (K <= 0 || M <= 0 || int64_t(w.i64.size()) != K * M) bad_form(n, "weight tensor " + shape_str(w.dims) + " does not match its data");
    if ((ws.size() != 1 && int64_t(ws.size()) != M) || wz.size() != ws.size())
      bad_form(n, "the weights' scale must be one value or one per output " + std::string(s.kind == StepKind::QConv2d ? "channel" : "column"));
    s.qx = xq;
    s.q_w_signed = w.elem == onnx::kInt8;
    s.q_per_channel = ws.size() > 1;
    const int shift = s.q_w_signed ? 0 : 128;
    s.qW.resize(size_t(K * M));
    for (int64_t k = 0; k < K; k++)
      for (int64_t j = 0; j < M; j++) s.qW[size_t(k * M + j)] = int8_t((trans ? w.i64[size_t(j * K + k)] : w.i64[size_t(k * M + j)]) - shift);
    s.q_wzp.resize(size_t(M));
    s.q_mult.resize(size_t(M));
    for (int64_t j = 0; j < M; j++) {
      const size_t qi = ws.size() == 1 ? 0 : size_t(j);
      s.q_wzp[size_t(j)] = int32_t(wz[qi] - shift);
      s.q_mult[size_t(j)] = xq.scale * ws[qi];
    }
    qdense_check_k(n, s);
  }

  // MatMul / Gemm whose weights were dequantised from int8 / uint8 and whose input was just quantised: QDense.  false: not that
  // pattern (a weight-only model, a per-row weight scale ...) -- the float layer on the dequantised weights serves it
  bool Lowerer::qdense_from_qdq(const NodeDef &n, bool gemm) {
    const Val a = get(n, 0);
    const Val &b = get(n, 1);
    const TensorData &bt = *b.c;
    if (a.is_const || a.ra != 0 || b.shape.size() != 2) return false;
    if (bt.q_data->elem != onnx::kUint8 && bt.q_data->elem != onnx::kInt8) return false;
    const bool window = !gemm && a.shape.size() == 3;
    if (!window && a.shape.size() != 2) return false;
    const bool tB = gemm && n.attr_i("transB", 0) != 0;
    if (gemm && (n.attr_i("transA", 0) != 0 || n.attr_f("alpha", 1.f) != 1.f || n.attr_f("beta", 1.f) != 1.f)) return false;
    if (bt.q_scale.size() > 1 && bt.q_axis != (tB ? 0 : 1)) return false;  // (scales along K: no integer form)
    auto pit = producer.find(a.buf);
    if (pit == producer.end()) return false;
    const Step &ps = plan.steps[size_t(pit->second)];
    Quant xq;
    if (ps.kind == StepKind::FakeQuant) xq = ps.qx;
    else if (quantised_layer(ps) && ps.qy.on) xq = ps.qy;
    else return false;
    const int64_t K = tB ? b.shape[1] : b.shape[0], M = tB ? b.shape[0] : b.shape[1];
    if (a.shape.back() != K) unsupported(n, "inner dimensions differ: " + shape_str(a.shape) + " x " + shape_str(b.shape));
    int in_buf = a.buf;
    std::string head;
    if (ps.kind == StepKind::FakeQuant) {  // the layer rounds its input itself: read what the FakeQuant read (and drop it when nothing else reads it)
      in_buf = ps.in0;
      head = ps.origin + "+";
      if (sole_tail(a.buf)) drop_tail();
    }
    const int64_t rep = window ? a.shape[1] : 1;
    if (window) prod({rep, std::max(K, M) + 3});
    Step s = make_qdense(n, in_buf, rep, *bt.q_data, tB, bt.q_scale, bt.q_zp, xq);
    if (gemm && has_input(n, 2)) {
      const Val &c = get(n, 2);
      if (int64_t(cf32(n, c).size()) != M) unsupported(n, "bias C must have M elements");
      qdense_take_bias(n, s, c);
    }
    s.origin = head + node_label(n);
    if (window) emit_window(std::move(s), n, {a.shape[0], rep, M});
    else {
      const std::string origin = s.origin;
      emit(std::move(s), n, {a.shape[0], M}).origin = origin;
    }
    return true;
  }

  // QLinearMatMul(a, a_scale, a_zp, b, b_scale, b_zp, y_scale, y_zp): the same step, spelled in one node; its result stays a quantised value
  void Lowerer::qlinear_matmul(const NodeDef &n) {
    if (n.inputs.size() != 8) bad_form(n, "needs its eight inputs");
    const Val a = get_raw(n, 0);
    if (a.is_const || a.pv || !a.q) bad_form(n, "input a must be a quantised activation (the output of QuantizeLinear or QLinearMatMul)");
    const Quant xq = act_quant(n, quant_args(n, 1, 2, "input a's"), "input a");
    if (!(xq == *a.q)) bad_form(n, "a_scale / a_zero_point differ from what input a was quantised with");
    const Val &b = get(n, 3);
    if (!b.is_const) bad_form(n, "input b must be a constant weight matrix");
    const QArgs qb = quant_args(n, 4, 5, "weights'");
    if (qb.elem != b.c->elem) bad_form(n, "the weights' zero point's element type differs from the data's");
    const Quant yq = act_quant(n, quant_args(n, 6, 7, "output's"), "the output");
    const bool window = a.shape.size() == 3;
    if ((!window && a.shape.size() != 2) || a.ra != 0) bad_form(n, "input a must be [rows, K] or [rows, T, K]");
    if (b.shape.size() != 2 || a.shape.back() != b.shape[0]) unsupported(n, "inner dimensions differ: " + shape_str(a.shape) + " x " + shape_str(b.shape));
    const int64_t rep = window ? a.shape[1] : 1, M = b.shape[1];
    if (window) prod({rep, std::max(b.shape[0], M) + 3});
    Step s = make_qdense(n, a.buf, rep, *b.c, false, qb.scale, qb.zp, xq);
    s.qy = yq;
    s.origin = node_label(n);
    const std::vector<int64_t> shape = window ? std::vector<int64_t>{a.shape[0], rep, M} : std::vector<int64_t>{a.shape[0], M};
    const int out = push_step(std::move(s), window ? flat_shape(shape) : shape);
    set_quant(n, out, shape, 0, yq, true, false);
  }

  // A QConv2d step over activation `a` (read from in_buf, quantised as xq) with the integer kernel `w` [M, C, kh, kw] (or [M, C, k])
  Step Lowerer::make_qconv(const NodeDef &n, const Val &a, int in_buf, const TensorData &w, const std::vector<float> &ws, const std::vector<int64_t> &wz, const Quant &xq) {
    Step s;
    s.kind = StepKind::QConv2d;
    s.in0 = in_buf;
    conv_geometry(n, s, a, w.dims);
    take_quant_weights(n, s, w, true, ws, wz, xq);  // [M, K] with k = (c, ky, kx) -> qW [K, M]
    return s;
  }

  // Conv whose kernel was dequantised from int8 / uint8 (per tensor or per output channel) and whose input was just quantised: QConv2d.
  // false: not that pattern (weight-only quantisation, a grouped or depthwise layer, scales along another axis) -- the float
  // convolution on the dequantised kernel serves it
  bool Lowerer::qconv_from_qdq(const NodeDef &n) {
    const Val a = get(n, 0);
    const Val &w = get(n, 1);
    const TensorData &wt = *w.c;
    if (a.ra != 0 || n.attr_i("group", 1) != 1) return false;
    if (wt.q_data->elem != onnx::kUint8 && wt.q_data->elem != onnx::kInt8) return false;
    if (wt.q_scale.size() > 1 && wt.q_axis != 0) return false;
    // a BatchNormalization behind the layer folds into FLOAT weights (batchnorm()); it is not folded into integer ones
    for (const NodeDef &c : m.nodes)
      if (c.op == "BatchNormalization" && !c.inputs.empty() && c.inputs[0] == n.outputs[0]) return false;
    auto pit = producer.find(a.buf);
    if (pit == producer.end()) return false;
    const Step &ps = plan.steps[size_t(pit->second)];
    Quant xq;
    if (ps.kind == StepKind::FakeQuant) xq = ps.qx;
    else if (quantised_layer(ps) && ps.qy.on) xq = ps.qy;
    else return false;
    int in_buf = a.buf;
    std::string head;
    if (ps.kind == StepKind::FakeQuant) {  // the layer rounds its input itself (as QDense does)
      in_buf = ps.in0;
      head = ps.origin + "+";
      if (sole_tail(a.buf)) drop_tail();
    }
    Step s = make_qconv(n, a, in_buf, *wt.q_data, wt.q_scale, wt.q_zp, xq);
    if (has_input(n, 2)) {
      const Val &c = get(n, 2);
      if (int64_t(cf32(n, c).size()) != s.M) unsupported(n, "bias size mismatch");
      qdense_take_bias(n, s, c);
    }
    const std::string origin = head + node_label(n);
    const std::vector<int64_t> shape = conv_out_shape(s, a);
    emit(std::move(s), n, shape).origin = origin;
    return true;
  }

  // QLinearConv(x, x_scale, x_zp, w, w_scale, w_zp, y_scale, y_zp[, B]): QConv2d spelled in one node; its result stays a quantised value.
  // A grouped / depthwise one keeps float semantics, as its QDQ spelling does: FakeQuant -> Conv2d on the dequantised kernel -> FakeQuant
  void Lowerer::qlinear_conv(const NodeDef &n) {
    if (n.inputs.size() < 8) bad_form(n, "needs at least its eight inputs (x, x_scale, x_zero_point, w, w_scale, w_zero_point, y_scale, y_zero_point)");
    const Val a = get_raw(n, 0);
    if (a.is_const || a.pv || !a.q) bad_form(n, "input x must be a quantised activation (the output of QuantizeLinear, QLinearConv or QLinearMatMul)");
    const Quant xq = act_quant(n, quant_args(n, 1, 2, "input x's"), "input x");
    if (!(xq == *a.q)) bad_form(n, "x_scale / x_zero_point differ from what input x was quantised with");
    const Val &w = get(n, 3);
    if (!w.is_const) bad_form(n, "input w must be a constant kernel");
    const QArgs qw = quant_args(n, 4, 5, "weights'");
    if (qw.elem != w.c->elem) bad_form(n, "the weights' zero point's element type differs from the data's");
    const Quant yq = act_quant(n, quant_args(n, 6, 7, "output's"), "the output");
    const bool one_d = a.shape.size() == 3 && w.shape.size() == 3;
    if (a.ra != 0 || (a.shape.size() != 4 && !one_d)) bad_form(n, "input x must be [N,C,L] or [N,C,H,W]");
    if (w.shape.size() != 4 && !one_d) bad_form(n, "the kernel must be [M,C/g,kh,kw] (or [M,C/g,k])");
    if (w.c->elem != onnx::kUint8 && w.c->elem != onnx::kInt8) bad_form(n, "the weights have element type " + std::to_string(w.c->elem) + "; only uint8 and int8 are supported");
    const int64_t M = w.shape[0];
    if ((qw.scale.size() != 1 && int64_t(qw.scale.size()) != M)) bad_form(n, "the weights' scale must be one value or one per output channel");
    std::vector<int64_t> bq;
    if (has_input(n, 8)) {
      const Val &b = get(n, 8);
      if (!b.is_const) bad_form(n, "the bias B is not a constant");
      if (b.c->elem != onnx::kInt32) bad_form(n, "the bias B has element type " + std::to_string(b.c->elem) + "; QLinearConv carries an int32 bias");
      if (int64_t(b.c->i64.size()) != M) bad_form(n, "the bias B must have one value per output channel");
      bq = b.c->i64;
    }
    if (n.attr_i("group", 1) == 1) {
      Step s = make_qconv(n, a, a.buf, *w.c, qw.scale, qw.zp, xq);
      s.qy = yq;
      if (!bq.empty()) {
        s.q_bias.assign(bq.begin(), bq.end());
        qdense_check_k(n, s);
      }
      s.origin = node_label(n);
      const std::vector<int64_t> shape = conv_out_shape(s, a);
      set_quant(n, push_step(std::move(s), shape), shape, 0, yq, true, false);
      return;
    }
    int in_buf = a.buf;
    if (!a.q_done) {  // the values the float layer reads: what the quantisation in front leaves of x
      Step f;
      f.kind = StepKind::FakeQuant;
      f.in0 = a.buf;
      f.qx = xq;
      f.origin = node_label(n) + "[input]";
      in_buf = push_step(std::move(f), a.shape);
    }
    Step s;
    s.kind = StepKind::Conv2d;
    s.in0 = in_buf;
    conv_geometry(n, s, a, w.shape);
    s.W.resize(w.c->i64.size());
    const int64_t per_m = s.K;
    if (int64_t(w.c->i64.size()) != per_m * M) bad_form(n, "weight tensor " + shape_str(w.shape) + " does not match its data");
    for (int64_t mo = 0; mo < M; mo++) {
      const size_t qi = qw.scale.size() == 1 ? 0 : size_t(mo);
      for (int64_t k = 0; k < per_m; k++) s.W[size_t(mo * per_m + k)] = float(w.c->i64[size_t(mo * per_m + k)] - qw.zp[qi]) * qw.scale[qi];
    }
    if (!bq.empty()) {
      s.bias.resize(size_t(M));
      for (int64_t mo = 0; mo < M; mo++) s.bias[size_t(mo)] = float(bq[size_t(mo)]) * (xq.scale * qw.scale[qw.scale.size() == 1 ? 0 : size_t(mo)]);
    }
    s.origin = node_label(n) + "[float]";
    const std::vector<int64_t> shape = conv_out_shape(s, a);
    const int conv_out = push_step(std::move(s), shape);
    Step f;
    f.kind = StepKind::FakeQuant;
    f.in0 = conv_out;
    f.qx = yq;
    f.origin = node_label(n) + "[output]";
    set_quant(n, push_step(std::move(f), shape), shape, 0, yq, true, false);
  }

  // ------------------------------------------------------------------------------------------
  // float16 graphs.  Activations stay f32 buffers; a value the graph types float16 carries Val::half, and the
  // result of every plan step that yields such a value is rounded once to half by a RoundHalf step (insert_half_roundings, after all
  // fusions have been made).  MatMul / Gemm on half weights become HDense, which rounds for itself.
  std::vector<uint16_t> Lowerer::half_bits(const std::vector<float> &v) {
    std::vector<uint16_t> o(v.size());
    for (size_t i = 0; i < v.size(); i++) o[i] = onnx::float_to_half(v[i]);
    return o;
  }
  void Lowerer::mark_half(const std::string &name) {
    auto it = vals.find(name);
    if (it == vals.end()) return;
    Val &v = it->second;
    if (v.is_const) {
      if (v.c->dtype != onnx::kFloat || v.c->elem == onnx::kFloat16) return;
      auto t = std::make_shared<TensorData>(*v.c);  // a folded half constant: rounded as the operator's half result would be
      for (float &f : t->f32) f = onnx::round_to_half(f);
      t->elem = onnx::kFloat16;
      t->q_data.reset();
      v.c = std::move(t);
      return;
    }
    v.half = true;
    if (v.buf >= 0) half_bufs.insert(v.buf);
  }

  // does the result of this step need a rounding to be a half value, given half inputs?  Not when it only selects, moves or negates them
  bool Lowerer::half_exact(const Step &s) {
    auto is_half_value = [](float v) { return std::isinf(v) || onnx::round_to_half(v) == v; };
    switch (s.kind) {
      case StepKind::RoundHalf:
      case StepKind::HDense:
      case StepKind::CopyCols:
      case StepKind::SliceCols:
      case StepKind::PadCols:
      case StepKind::ChannelShuffle:
      case StepKind::PixelShuffle:
      case StepKind::ArgMax:
      case StepKind::ArgMin:
      case StepKind::TopK:
      case StepKind::NearestReduce: return true;
      case StepKind::NearestVote: return s.out_mode == kVoteLabel;  // (a class value picked from a table; the other modes divide)
      case StepKind::Tokens: return s.cst.empty();  // (movement alone; a half graph's position Add is never folded)
      case StepKind::RowReduce: return s.out_mode == kReduceMax || s.out_mode == kReduceMin;
      case StepKind::Pool2d:
      case StepKind::GlobalAvgPool: return s.is_max && s.act == Act::None;
      case StepKind::Unary:
        return s.act == Act::Relu || s.act == Act::Neg || s.act == Act::Abs || (s.act == Act::Clip && is_half_value(s.act_a) && is_half_value(s.act_b));
      default: return false;
    }
  }
  // A RoundHalf step behind every step that writes a float16-typed buffer and is not exact on halves; the readers (and the served
  // output) move to the rounded buffer.  Runs once, after the last node: fusions into a producing step (an activation, a folded
  // BatchNormalization, a scaler) have happened by then, so a fused step is rounded once, at its result.
  void Lowerer::insert_half_roundings() {
    if (half_bufs.empty()) return;
    std::map<int, size_t> last_writer;
    for (size_t i = 0; i < plan.steps.size(); i++) last_writer[plan.steps[i].out] = i;
    std::map<int, int> moved;
    auto at = [&](int b) { auto it = moved.find(b); return it == moved.end() ? b : it->second; };
    std::vector<Step> out;
    for (size_t i = 0; i < plan.steps.size(); i++) {
      Step s = std::move(plan.steps[i]);
      s.in0 = at(s.in0), s.in1 = at(s.in1), s.in2 = at(s.in2);  // (in3 is the model input: never a rounded buffer)
      const bool round = half_bufs.count(s.out) && last_writer[s.out] == i && !half_exact(s);
      Step r;
      if (round) {
        r.kind = StepKind::RoundHalf;
        r.in0 = s.out;
        r.origin = s.origin + "[half]";
        plan.buf_shape.push_back(plan.buf_shape[size_t(s.out)]);
        plan.buf_per_row.push_back(plan.buf_per_row[size_t(s.out)]);
        r.out = int(plan.buf_shape.size()) - 1;
        moved[s.out] = r.out;
      }
      out.push_back(std::move(s));
      if (round) out.push_back(std::move(r));
    }
    plan.steps = std::move(out);
    plan.out_buf = at(plan.out_buf);
  }

  // MatMul / Gemm of a float16 activation by constant float16 weights: the HDense step (plan.hpp, hip/hdense.hip).  false: not that
  // form (alpha / beta other than 1, a float bias, INFERA_HDENSE=0 ...) -- the float path serves it: Dense on the widened weights + RoundHalf
  bool Lowerer::hdense(const NodeDef &n, bool gemm) {
    if (!cur_half || !hdense_enabled) return false;
    const Val a = get(n, 0);
    const Val &b = get(n, 1);
    if (a.is_const || !a.half || a.ra != 0 || b.c->dtype != onnx::kFloat || b.c->elem != onnx::kFloat16 || b.shape.size() != 2) return false;
    const bool window = !gemm && a.shape.size() == 3;
    if (!window && a.shape.size() != 2) return false;
    if (gemm && (n.attr_i("transA", 0) != 0 || n.attr_f("alpha", 1.f) != 1.f || n.attr_f("beta", 1.f) != 1.f)) return false;
    const bool tB = gemm && n.attr_i("transB", 0) != 0;
    const int64_t K = tB ? b.shape[1] : b.shape[0], M = tB ? b.shape[0] : b.shape[1];
    if (K <= 0 || M <= 0 || int64_t(b.c->f32.size()) != prod({K, M}) || K > (int64_t(1) << 24) || M > (int64_t(1) << 24)) return false;
    if (a.shape.back() != K) unsupported(n, "inner dimensions differ: " + shape_str(a.shape) + " x " + shape_str(b.shape));
    Step s;
    s.kind = StepKind::HDense;
    s.K = K;
    s.M = M;
    if (gemm && has_input(n, 2)) {
      const Val &c = get(n, 2);
      if (!c.is_const || c.c->dtype != onnx::kFloat || c.c->elem != onnx::kFloat16 || (int64_t(c.c->f32.size()) != M && c.c->f32.size() != 1)) return false;
      s.h_bias.resize(size_t(M));
      for (int64_t j = 0; j < M; j++) s.h_bias[size_t(j)] = onnx::float_to_half(c.c->f32[c.c->f32.size() == 1 ? 0 : size_t(j)]);
      s.h_bias_mode = kHalfBiasGemm;
    }
    const auto &w = b.c->f32;
    s.hW.resize(size_t(K * M));
    for (int64_t k = 0; k < K; k++)
      for (int64_t j = 0; j < M; j++) s.hW[size_t(k * M + j)] = onnx::float_to_half(tB ? w[size_t(j * K + k)] : w[size_t(k * M + j)]);
    int in_buf = a.buf;
    std::string head;
    if (const Step *t = sole_tail(a.buf); t && t->kind == StepKind::RoundHalf) {  // the layer rounds its input on load: read what the RoundHalf read
      in_buf = t->in0;
      head = t->origin + "+";
      drop_tail();
    }
    s.in0 = in_buf;
    const int64_t rep = window ? a.shape[1] : 1;
    if (window) prod({rep, std::max(K, M) + 3});
    s.rep = rep;
    s.origin = head + node_label(n);
    if (window) emit_window(std::move(s), n, {a.shape[0], rep, M});
    else {
      const std::string origin = s.origin;
      emit(std::move(s), n, {a.shape[0], M}).origin = origin;
    }
    return true;
  }

  // ------------------------------------------------------------------------------------------
  void Lowerer::lower_node(const NodeDef &n) {
    const std::string &op = n.op;
    if (op != "Conv")
      for (const auto &in_name : n.inputs) {
        auto it = vals.find(in_name);
        if (it != vals.end() && it->second.padded()) unsupported(n, "the output of a Pad node can only feed a Conv (its padding is folded into the convolution)");
      }
    static const std::set<std::string> reads_time_major = {"Transpose", "Squeeze", "Unsqueeze", "Reshape", "Identity", "Dropout", "Flatten", "Shape",
                                                           "Gather", "Slice", "LSTM", "GRU", "RNN",
                                                           "InstanceNormalization", "GroupNormalization"};  // (refused in their own words)
    check_row_axis(n, reads_time_major.count(op) > 0);
    if (op == "DynamicQuantizeLinear")
      bad_form(n, "its scale spans all rows of a call, so a row's result would depend on its chunk; quantise statically (QuantizeLinear with constant scales)");
    if (op != "DequantizeLinear" && op != "QLinearMatMul" && op != "QLinearConv")
      for (const auto &in_name : n.inputs) {
        auto it = vals.find(in_name);
        if (it != vals.end() && it->second.q) bad_form(n, "it reads the quantised tensor '" + in_name + "'; only DequantizeLinear, QLinearMatMul and QLinearConv do");
      }
    if ((op == "ArgMin" || op == "TopK" || op == "Sqrt" || op == "Identity") && nearest_reader(n)) return;
    if (reads_view(n)) return lower_on_view(n);
    if (op == "QuantizeLinear") quantize_linear(n);
    else if (op == "DequantizeLinear") dequantize_linear(n);
    else if (op == "QLinearMatMul") qlinear_matmul(n);
    else if (op == "QLinearConv") qlinear_conv(n);
    else if (op == "LSTM" || op == "GRU" || op == "RNN") recurrent(n);
    else if (op == "ConstantOfShape" || op == "Expand") constant_fill(n);
    else if (op == "MatMul") dense(n, false);
    else if (op == "Gemm") dense(n, true);
    else if (op == "Add") binary(n, '+');
    else if (op == "Sub") binary(n, '-');
    else if (op == "Mul") binary(n, '*');
    else if (op == "Div") binary(n, '/');
    else if (op == "Min") binary(n, 'm');
    else if (op == "Max") binary(n, 'M');
    else if (op == "Pow") binary(n, '^');
    else if (op == "PRelu") binary(n, 'p');
    else if (op == "Relu" || op == "Sigmoid" || op == "Tanh" || op == "LeakyRelu" || op == "Clip" || op == "Exp" || op == "Log" ||
             op == "Sqrt" || op == "Neg" || op == "Abs" || op == "Elu" || op == "Selu" || op == "Softplus" || op == "HardSigmoid" ||
             op == "HardSwish" || op == "Erf" || op == "Gelu" || op == "Reciprocal" || op == "Floor" || op == "Ceil" ||
             op == "Softsign" || op == "Round")
      unary(n);
    else if (op == "Shape") shape_op(n);
    else if (op == "Gather") gather(n);
    else if (op == "Slice") slice(n);
    else if (op == "Split") split(n);
    else if (op == "Cast") cast(n);
    else if (op == "Concat") concat(n);
    else if (op == "ReduceMean") reduce_mean(n);
    else if (op == "ReduceSum" || op == "ReduceMax" || op == "ReduceMin" || op == "ReduceProd" || op == "ReduceL1" || op == "ReduceL2" ||
             op == "ReduceSumSquare" || op == "ReduceLogSum" || op == "ReduceLogSumExp")
      row_reduce(n);
    else if (op == "ArgMin") argmin(n);
    else if (op == "TopK") topk(n);
    else if (op == "LayerNormalization") layer_norm(n);
    else if (op == "RMSNormalization") rms_norm(n);
    else if (op == "RotaryEmbedding") rotary_embedding(n);
    else if (op == "InstanceNormalization") instance_norm(n);
    else if (op == "GroupNormalization") group_norm(n);
    else if (op == "ArgMax") argmax(n);
    else if (op == "Identity" || op == "Dropout" || op == "Flatten" || op == "Reshape" || op == "Squeeze" || op == "Unsqueeze") reshape_like(n);
    else if (op == "Softmax") softmax(n, false);
    else if (op == "LogSoftmax") softmax(n, true);
    else if (op == "Conv") conv(n);
    else if (op == "ConvTranspose") conv_transpose(n);
    else if (op == "Resize" || op == "Upsample") resize(n);
    else if (op == "DepthToSpace" || op == "SpaceToDepth") depth_space(n);
    else if (op == "BatchNormalization") batchnorm(n);
    else if (op == "MaxPool") pool(n, true);
    else if (op == "AveragePool") pool(n, false);
    else if (op == "GlobalAveragePool") global_avgpool(n, false);
    else if (op == "GlobalMaxPool") global_avgpool(n, true);
    else if (op == "Pad") pad(n);
    else if (op == "Sum") sum(n);
    else if (op == "LRN") lrn(n);
    else if (op == "Transpose") transpose(n);
    else if (op == "Constant") {
      if (auto *a = n.attr("value"); a && a->t) vals[n.outputs[0]] = const_val(a->t);
      // scalar / 1-D attribute forms (opset 12+)
      else if (auto *f = n.attr("value_float")) vals[n.outputs[0]] = const_f32({f->f}, {});
      else if (auto *i = n.attr("value_int")) set_const_i64(n, {i->i}, {});
      else if (auto *is = n.attr_ints("value_ints")) set_const_i64(n, *is, {int64_t(is->size())});
      else unsupported(n, "only the value / value_float / value_int / value_ints forms are supported");
    } else {
      unsupported(n, "unsupported operator");
    }
  }

  // every operator but the few that understand the row-axis tag reads rows-first values only
  void Lowerer::check_row_axis(const NodeDef &n, bool understands) {
    if (understands) return;
    for (const auto &in_name : n.inputs) {
      auto it = vals.find(in_name);
      if (it != vals.end() && !it->second.is_const && it->second.ra != 0)
        unsupported(n, "input '" + in_name + "' " + shape_str(it->second.shape) + " is time-major (its row axis is axis " + std::to_string(it->second.ra) +
                           "); only a Transpose / Squeeze / Reshape that moves no data, one time step or a recurrent layer can read it");
    }
  }
  // ConstantOfShape / Expand over constants: the sub-graph exporters write for a zero (or constant) initial state of a recurrent layer,
  // [D, rows, H] with the row count taken from Shape(X).  The symbolic row count (0 in a folded shape) becomes extent 1: one row, the same
  // for all.  (An extent that is 0 in the model file itself -- an empty tensor -- cannot be told from the folded row count and would become
  // one element too; the only consumer of these constants, a recurrent layer's initial state, checks the shape it gets.)
  void Lowerer::constant_fill(const NodeDef &n) {
    const bool expand = n.op == "Expand";
    std::vector<int64_t> dims = const_ints(n, expand ? 1 : 0, "shape");
    const int64_t lead = dims.size() == 3 ? dims[0] : -1;  // (a [batch, p, E] target: tokens_concat)
    for (auto &d : dims) {
      if (d == 0) d = 1;
      if (d < 0) unsupported(n, "negative extent");
    }
    std::vector<int64_t> src_dims;
    std::vector<float> src{0.f};
    if (expand) {
      const Val &v = get(n, 0);
      if (!v.is_const || v.c->dtype != onnx::kFloat) unsupported(n, "only constant f32 data is expanded");
      src = v.c->f32;
      src_dims = v.shape;
    } else if (const onnx::Attribute *a = n.attr("value"); a && a->t) {
      if (a->t->count() != 1) unsupported(n, "value must hold one element");
      if (a->t->dtype != onnx::kFloat) unsupported(n, "only an f32 fill value");
      src = a->t->f32;
    }
    if (src_dims.size() > dims.size()) dims.insert(dims.begin(), src_dims.size() - dims.size(), 1);
    while (src_dims.size() < dims.size()) src_dims.insert(src_dims.begin(), 1);
    for (size_t i = 0; i < dims.size(); i++) {
      if (src_dims[i] != 1 && dims[i] != 1 && src_dims[i] != dims[i]) unsupported(n, shape_str(src_dims) + " does not broadcast to " + shape_str(dims));
      if (dims[i] == 1) dims[i] = src_dims[i];
    }
    const int64_t total = prod(dims);
    if (total > (int64_t(1) << 24)) unsupported(n, "constant too large");
    std::vector<float> o(static_cast<size_t>(total));
    for (int64_t flat = 0; flat < total; flat++) {
      int64_t rem = flat, idx = 0, stride = 1;
      for (size_t i = dims.size(); i-- > 0;) {
        const int64_t coord = rem % dims[i];
        rem /= dims[i];
        if (src_dims[i] != 1) idx += coord * stride;
        stride *= src_dims[i];
      }
      o[size_t(flat)] = src[size_t(idx)];
    }
    if (expand && dims.size() == 3 && lead >= 0) expanded_lead[n.outputs[0]] = lead;
    vals[n.outputs[0]] = const_f32(std::move(o), dims);
  }
  // the columns an input of a multi-input model takes in the input buffer: k of [rows, k]; a rank-1 [rows] integer input is one column
  int64_t Lowerer::input_cols(const onnx::ValueDef &v) { return v.dims.size() == 1 ? 1 : v.dims[1]; }

  // lax: a Reshape whose target is computed (from Shape nodes) counts too; lower_interact evaluates it
  bool Lowerer::interact_is_view(const NodeDef &r, const std::string &cur, InteractView *v, bool lax) const {
    if (!graph->std_dom(r) || r.outputs.empty() || r.inputs.empty() || r.inputs[0] != cur) return false;
    v->target.clear();
    if (r.op == "Identity") return true;
    if (r.op == "Flatten") return v->target = {r.attr_i("axis", 1)}, true;
    std::vector<int64_t> dims;
    if (r.op != "Reshape" || r.inputs.size() != 2) return false;
    return (graph_const_ints(r.inputs[1], &v->target, &dims) && !v->target.empty()) || (lax && !graph->row_data.count(r.inputs[1]));
  }
  // x * x or x ^ 2: the value squared ("" = n is no square)
  std::string Lowerer::interact_squared(const NodeDef &n) const {
    if (!graph->std_dom(n) || n.inputs.size() != 2) return "";
    if (n.op == "Mul" && n.inputs[0] == n.inputs[1]) return n.inputs[0];
    double e = 0;
    size_t cnt = 0;
    if (n.op == "Pow" && graph_const_scalar(n.inputs[1], &e, &cnt) && cnt == 1 && e == 2.0) return n.inputs[0];
    return "";
  }
  // ReduceSum over exactly `axis_a` or `axis_b`
  bool Lowerer::interact_sum_over(const NodeDef &n, int64_t axis_a, int64_t axis_b) const {
    std::vector<int64_t> ax;
    if (!graph->std_dom(n) || n.op != "ReduceSum" || n.inputs.empty() || n.attr_i("noop_with_empty_axes", 0) != 0 || !graph_ints_arg(n, 1, "axes", &ax)) return false;
    return ax.size() == 1 && (ax[0] == axis_a || ax[0] == axis_b);
  }

  // the node that alone reads the DATA of `v`: Shape nodes read its shape only and do not count (null: several, none, a graph output)
  const NodeDef *Lowerer::interact_data_reader(const std::string &v) const {
    auto it = graph->consumers_of.find(v);
    if (it == graph->consumers_of.end() || graph->graph_outs.count(v)) return nullptr;
    const NodeDef *one = nullptr;
    for (size_t c : it->second) {
      if (m.nodes[c].op == "Shape") continue;
      if (one) return nullptr;
      one = &m.nodes[c];
    }
    return one;
  }
  // The values the step absorbs exist nowhere: the Shape nodes that read them, and everything computed from those and constants alone (the
  // targets of the pattern's Reshapes, TorchScript's li * k + lj), must feed the pattern only.  They join im.nodes.  false: something else reads one
  bool Lowerer::interact_shape_closure(InteractMatch &im, size_t anchor) const {
    std::set<size_t> mine(im.nodes.begin(), im.nodes.end());
    std::set<std::string> gone, derived;
    for (size_t i : im.nodes)
      for (const auto &o : m.nodes[i].outputs) gone.insert(o);
    std::set<size_t> extra;
    for (size_t i = 0; i < m.nodes.size(); i++) {
      const NodeDef &n = m.nodes[i];
      if (!graph->live[i] || mine.count(i) || i == anchor || n.inputs.empty()) continue;
      bool any = false, all = true;
      if (n.op == "Shape") {
        any = gone.count(n.inputs[0]) > 0 || derived.count(n.inputs[0]) > 0;
      } else {
        for (const auto &in : n.inputs) {
          if (in.empty()) continue;
          any = any || derived.count(in);
          all = all && (derived.count(in) || !graph->row_data.count(in));
        }
      }
      if (!any || !all) continue;
      extra.insert(i);
      for (const auto &o : n.outputs) derived.insert(o);
    }
    for (const auto &v : gone)  // an absorbed value: read by the pattern, or by a Shape node of the closure
      if (auto it = graph->consumers_of.find(v); it != graph->consumers_of.end())
        for (size_t c : it->second)
          if (!mine.count(c) && c != anchor && !extra.count(c)) return false;
    for (const auto &v : derived) {
      if (graph->graph_outs.count(v)) return false;
      if (auto it = graph->consumers_of.find(v); it != graph->consumers_of.end())
        for (size_t c : it->second)
          if (!mine.count(c) && c != anchor && !extra.count(c)) return false;
    }
    im.nodes.insert(im.nodes.end(), extra.begin(), extra.end());
    return true;
  }
  // an integer tensor known at load once k is: constants, Shape of the product ([rows, k, k], rows = kInteractDyn), Gather / Concat /
  // Mul / Add / Sub and the shape-preserving operators over those.  false: something else
  bool Lowerer::interact_eval(const std::string &v, const std::string &z, int64_t k, std::vector<int64_t> *out, int depth) const {
    std::vector<int64_t> dims;
    if (graph_const_ints(v, out, &dims)) return true;
    const NodeDef *p = graph->producer(v);
    if (!p || depth > 32 || !graph->std_dom(*p) || p->inputs.empty()) return false;
    std::vector<int64_t> a, b;
    if (p->op == "Shape") {
      if (p->inputs[0] == z) return *out = {kInteractDyn, k, k}, true;
      if (!interact_eval(p->inputs[0], z, k, &a, depth + 1)) return false;
      return *out = {int64_t(a.size())}, true;  // (of a list)
    }
    if (p->op == "Cast" || p->op == "Identity" || p->op == "Unsqueeze" || p->op == "Squeeze" || p->op == "Reshape") return interact_eval(p->inputs[0], z, k, out, depth + 1);
    if (p->op == "Concat") {
      out->clear();
      for (const auto &in : p->inputs) {
        if (!interact_eval(in, z, k, &a, depth + 1)) return false;
        out->insert(out->end(), a.begin(), a.end());
      }
      return true;
    }
    if (p->inputs.size() != 2 || !interact_eval(p->inputs[0], z, k, &a, depth + 1) || !interact_eval(p->inputs[1], z, k, &b, depth + 1)) return false;
    out->clear();
    if (p->op == "Gather") {
      if (p->attr_i("axis", 0) != 0) return false;
      for (int64_t ix : b) {
        if (ix < 0) ix += int64_t(a.size());
        if (ix < 0 || ix >= int64_t(a.size())) return false;
        out->push_back(a[size_t(ix)]);
      }
      return true;
    }
    if (p->op != "Mul" && p->op != "Add" && p->op != "Sub") return false;
    if (a.size() != b.size() && a.size() != 1 && b.size() != 1) return false;
    for (size_t i = 0; i < std::max(a.size(), b.size()); i++) {
      const int64_t x = a[a.size() == 1 ? 0 : i], y = b[b.size() == 1 ? 0 : i];
      int64_t r = 0;
      if (x == kInteractDyn || y == kInteractDyn) return false;
      if (p->op == "Mul" ? __builtin_mul_overflow(x, y, &r) : p->op == "Add" ? __builtin_add_overflow(x, y, &r) : __builtin_sub_overflow(x, y, &r)) return false;
      out->push_back(r);
    }
    return true;
  }

  void Lowerer::find_interactions() {
    const size_t N = m.nodes.size();
    auto claim = [&](const InteractMatch &im, size_t anchor) {
      for (size_t i : im.nodes) absorbed[i] = 1, region[i] = 0;
      region[anchor] = 0;
    };
    for (size_t i = 0; i < N; i++) {
      const NodeDef &n = m.nodes[i];
      if (!graph->live[i] || absorbed[i] || !graph->std_dom(n) || n.inputs.size() != 2 || n.outputs.empty()) continue;
      if (n.op == "MatMul" && graph->row_data.count(n.inputs[0]) && graph->row_data.count(n.inputs[1])) {
        size_t ti = 0;
        const NodeDef *tp = graph->producer(n.inputs[1], &ti);
        const auto *perm = tp ? tp->attr_ints("perm") : nullptr;
        // both operands are one value, the right one through Transpose(0,2,1) that nothing else reads: anything else keeps its refusal
        if (!tp || tp->op != "Transpose" || !graph->std_dom(*tp) || tp->inputs.size() != 1 || tp->inputs[0] != n.inputs[0] || !perm ||
            *perm != std::vector<int64_t>{0, 2, 1} || graph->sole_reader(n.inputs[1], false) != &n)
          continue;
        InteractMatch im;
        im.T = n.inputs[0];
        im.product = i;
        im.nodes = {ti};
        // Flatten / Reshape / Identity hops to a Gather(axis = 1) by a constant list, or TorchScript's Z[:, li, lj]: Transpose(1,2,0) ->
        // Flatten(2) -> Gather(axis = 0) -> Reshape -> Transpose(1,0) -> Reshape, matched by the data it moves (the Shape sub-graphs that
        // feed its Reshapes and its index are checked below).  Without either the product itself is the step
        std::string cur = n.outputs[0];
        std::vector<InteractView> views;
        size_t anchor = i;
        auto hop_views = [&](std::vector<InteractView> *vs, bool lax = false) {
          for (;;) {
            const NodeDef *r = interact_data_reader(cur);
            InteractView v;
            if (!r || !interact_is_view(*r, cur, &v, lax)) return r;
            v.node = size_t(r - m.nodes.data());
            vs->push_back(v);
            cur = r->outputs[0];
          }
        };
        auto is_gather = [&](const NodeDef *r) { return r && r->op == "Gather" && graph->std_dom(*r) && r->inputs.size() == 2 && r->inputs[0] == cur && !r->outputs.empty(); };
        auto is_transpose = [&](const NodeDef *r, const std::vector<int64_t> &want) {
          const auto *pm = r && r->op == "Transpose" && graph->std_dom(*r) && r->inputs.size() == 1 && r->inputs[0] == cur && !r->outputs.empty() ? r->attr_ints("perm") : nullptr;
          return pm && *pm == want;
        };
        const NodeDef *r = hop_views(&views);
        std::vector<int64_t> dims;
        if (is_gather(r) && graph_const_ints(r->inputs[1], &im.idx, &dims) && dims.size() == 1) {
          im.gather = size_t(r - m.nodes.data());
          im.views = views;
          im.nodes.push_back(i);
          for (const InteractView &w : views) im.nodes.push_back(w.node);
          anchor = im.gather;
        } else if (views.empty() && is_transpose(r, {1, 2, 0})) {
          InteractMatch t3 = im;
          t3.nodes.push_back(i);
          t3.nodes.push_back(size_t(r - m.nodes.data()));
          cur = r->outputs[0];
          const NodeDef *g = hop_views(&t3.views, true);
          if (is_gather(g) && !graph->row_data.count(g->inputs[1])) {
            t3.gather = size_t(g - m.nodes.data());
            t3.index_value = g->inputs[1];
            cur = g->outputs[0];
            const NodeDef *tb = hop_views(&t3.views_after, true);
            if (is_transpose(tb, {1, 0})) {
              for (const InteractView &w : t3.views) t3.nodes.push_back(w.node);
              t3.nodes.push_back(t3.gather);
              for (const InteractView &w : t3.views_after) t3.nodes.push_back(w.node);
              size_t last = size_t(tb - m.nodes.data());
              cur = tb->outputs[0];
              // the Reshape to [N, P] behind it (and nothing that flattens further)
              for (;;) {
                const NodeDef *v = interact_data_reader(cur);
                InteractView w;
                if (!v || (v->op != "Reshape" && v->op != "Identity") || !graph->std_dom(*v) || v->inputs.empty() || v->inputs[0] != cur || v->outputs.empty()) break;
                w.node = size_t(v - m.nodes.data());
                w.back = true;
                t3.views_after.push_back(w);
                t3.nodes.push_back(last);
                last = w.node;
                cur = v->outputs[0];
              }
              t3.advanced = true;
              im = std::move(t3);
              anchor = last;
              im.selection_value = cur;
            }
          }
        }
        if (im.gather != SIZE_MAX) {
          // pass-through: the selection's only reader is an axis-1 Concat whose other inputs are inputs of the Concat that built T
          const std::string selv = im.advanced ? im.selection_value : m.nodes[im.gather].outputs[0];
          const NodeDef *oc = graph->sole_reader(selv, false);
          std::string tv = im.T;
          size_t tci = 0;
          const NodeDef *tc = graph->producer(tv, &tci);
          InteractView ignore;
          while (tc && tc->op != "Concat" && !tc->inputs.empty() && interact_is_view(*tc, tc->inputs[0], &ignore)) tc = graph->producer(tc->inputs[0], &tci);
          auto axis1 = [&](const NodeDef *c) { return c && c->op == "Concat" && graph->std_dom(*c) && !c->outputs.empty() && (c->attr_i("axis", 1) == 1 || c->attr_i("axis", 1) == -1); };
          if (axis1(oc) && axis1(tc) && oc->inputs.size() > 1) {
            bool ok = true;
            int mine = 0;
            for (const auto &in : oc->inputs) {
              if (in == selv) mine++;
              else ok = ok && std::find(tc->inputs.begin(), tc->inputs.end(), in) != tc->inputs.end();
            }
            if (ok && mine == 1) {
              im.out_concat = size_t(oc - m.nodes.data());
              im.t_concat = tci;
              im.nodes.push_back(anchor);
              anchor = im.out_concat;
              im.selection_value = selv;
            }
          }
        }
        if (!interact_shape_closure(im, anchor)) continue;  // (an absorbed value has a reader the step does not stand for)
        claim(im, anchor);
        interact_at[anchor] = std::move(im);
        continue;
      }
      if (n.op != "Sub") continue;
      // fm: Sub(square(S), QS), S = ReduceSum(T, [1]), QS = ReduceSum(square(T), [1]); every inner value has this one reader
      size_t ssi = 0, qsi = 0, si = 0, qi = 0;
      const NodeDef *ss = graph->producer(n.inputs[0], &ssi), *qs = graph->producer(n.inputs[1], &qsi);
      if (!ss || !qs || !interact_sum_over(*qs, 1, -2)) continue;
      const std::string sv = interact_squared(*ss);
      const NodeDef *s = sv.empty() ? nullptr : graph->producer(sv, &si);
      const NodeDef *q = graph->producer(qs->inputs[0], &qi);
      if (!s || !q || !interact_sum_over(*s, 1, -2)) continue;
      const std::string tv = interact_squared(*q);
      if (tv.empty() || tv != s->inputs[0] || !graph->row_data.count(tv)) continue;
      if (s->attr_i("keepdims", 1) != qs->attr_i("keepdims", 1)) continue;
      if (graph->sole_reader(sv, true) != ss || graph->sole_reader(n.inputs[0], false) != &n || graph->sole_reader(n.inputs[1], false) != &n ||
          graph->sole_reader(qs->inputs[0], false) != qs)
        continue;  // (an inner value with a second reader: the operators keep their own lowering and refusals)
      InteractMatch im;
      im.mode = kInteractFm;
      im.T = tv;
      im.product = i;
      im.keep = s->attr_i("keepdims", 1) != 0;
      im.nodes = {si, ssi, qi, qsi};
      size_t anchor = i;
      // behind it: a constant scalar Mul and a ReduceSum over the last axis, in either order, each at most once
      for (;;) {
        const NodeDef &a = m.nodes[anchor];
        const NodeDef *r = graph->sole_reader(a.outputs[0], false);
        if (!r || !graph->std_dom(*r) || r->outputs.empty()) break;
        const size_t ri = size_t(r - m.nodes.data());
        double hv = 0;
        size_t cnt = 0;
        if (!im.has_h && r->op == "Mul" && r->inputs.size() == 2 && r->inputs[0] != r->inputs[1] &&
            graph_const_scalar(r->inputs[r->inputs[0] == a.outputs[0] ? 1 : 0], &hv, &cnt) && cnt == 1) {
          im.has_h = true, im.h = hv, im.h_after = im.last_sum != SIZE_MAX;
        } else if (im.last_sum == SIZE_MAX && interact_sum_over(*r, -1, im.keep ? 2 : 1) && r->inputs[0] == a.outputs[0]) {
          im.last_sum = ri;
        } else {
          break;
        }
        im.nodes.push_back(anchor);
        anchor = ri;
      }
      claim(im, anchor);
      interact_at[anchor] = std::move(im);
    }
  }

  // The fm pattern is claimed by structure, before any shape is known.  On anything but a plain rank-3 activation it is not the
  // bi-interaction of a window -- on [N, k] axis 1 is the last axis and the same operators are the FM term over scalar fields, which the
  // single-operator lowering serves (RowReduce, BinaryAct) -- so the claim is given up and the nodes lower as they always did.  (T . T^T
  // has no such reading: Transpose(0,2,1) needs rank 3.)
  bool Lowerer::interact_released(const InteractMatch &im) const {
    if (im.mode != kInteractFm) return false;
    auto it = vals.find(im.T);
    if (it == vals.end()) return true;
    const Val &t = it->second;
    return t.is_const || t.pv || t.nn || t.q || t.cl || t.padded() || t.half || t.buf < 0 || t.shape.size() != 3;
  }

  void Lowerer::lower_interact(const InteractMatch &im, const NodeDef &anchor) {
    const NodeDef &pn = m.nodes[im.product];
    auto it = vals.find(im.T);
    if (it == vals.end()) unsupported(pn, "input '" + im.T + "' is not produced by any earlier node");
    if (it->second.pv) materialize(im.T, &pn);
    if (it->second.nn) materialize_nearest(im.T);
    const Val t = vals.at(im.T);
    const char *what = im.mode == kInteractDot ? "T . T^T" : "the bi-interaction term";
    if (t.is_const || t.q || t.cl || t.padded() || t.half || t.buf < 0) bad_form(pn, std::string(what) + " of a value that is no plain f32 activation");
    if (t.shape.size() != 3)
      bad_form(pn, std::string(what) + " of " + shape_str(t.shape) + "; T must be a window [N, k, d]" + (t.shape.size() == 2 ? " ([N,F] x [F,N] mixes rows)" : ""));
    if (t.ra != 0)
      bad_form(pn, std::string(what) + " of a time-major value " + shape_str(t.shape) + " (its row axis is axis " + std::to_string(t.ra) + "); T must be rows first, [N, k, d]");
    const int64_t N = t.shape[0], k = t.shape[1], d = t.shape[2];
    if (t.buf > 0 && plan.buf_shape[size_t(t.buf)].size() != 2) {
      // [N, k, d] built by an axis-1 Concat is registered as an [N, C, 1, L] tensor: its rows are flat, and it is a window from here on
      for (const Step &s : plan.steps)
        if (s.out == t.buf && s.kind != StepKind::CopyCols) bad_form(pn, std::string(what) + " of an [N,C,L] tensor a " + s.origin + " step wrote, not a window of a flat table");
      plan.buf_shape[size_t(t.buf)] = {N, k * d};
    }
    auto pack = std::make_shared<InteractPack>();
    pack->mode = im.mode, pack->k = k, pack->d = d;
    Step s;
    s.kind = StepKind::Interact;
    s.in0 = t.buf;
    s.rep = k, s.K = d;
    std::vector<size_t> all = im.nodes;
    all.push_back(size_t(&anchor - m.nodes.data()));
    std::sort(all.begin(), all.end());
    for (size_t i : all) s.origin += (s.origin.empty() ? "" : "+") + node_label(m.nodes[i]);
    std::vector<int64_t> shape;
    if (im.mode == kInteractFm) {
      if (const std::string why = interact_refusal(k, d, 0); !why.empty()) bad_form(pn, why);
      pack->has_h = im.has_h, pack->h = float(im.h), pack->sum_last = im.last_sum != SIZE_MAX, pack->h_after = im.h_after;
      shape = im.keep ? std::vector<int64_t>{N, 1, d} : std::vector<int64_t>{N, d};
      if (pack->sum_last) {
        if (m.nodes[im.last_sum].attr_i("keepdims", 1) != 0) shape.back() = 1;
        else shape.pop_back();
      }
    } else if (im.gather == SIZE_MAX) {
      if (const std::string why = interact_refusal(k, d, 0); !why.empty()) bad_form(pn, why);
      pack->whole = true;
      pack->sel.resize(size_t(k * k));
      std::iota(pack->sel.begin(), pack->sel.end(), int64_t(0));
      shape = {N, k, k};
    } else if (im.advanced) {
      // Transpose(1,2,0) -> [k, k, N]; the views arrive at [k * k, N]; Gather(axis = 0) -> [P, N]; views of rank 2; Transpose(1,0) ->
      // [N, P]; views of rank 2
      const NodeDef &gn = m.nodes[im.gather];
      const std::string &zname = pn.outputs[0];
      int flattened = 0;
      auto target_rank = [&](const InteractView &v, std::vector<int64_t> *tgt) {
        const NodeDef &vn = m.nodes[v.node];
        return vn.op == "Reshape" && vn.inputs.size() == 2 && interact_eval(vn.inputs[1], zname, k, tgt);
      };
      // a Reshape in front of the Gather names [k * k, N] and nothing else: k * k or -1, then the rows (of Shape(Z)) or -1, not both -1
      auto flat_target = [&](const std::vector<int64_t> &tgt) {
        return tgt.size() == 2 && (tgt[0] == k * k || tgt[0] == -1) && (tgt[1] == kInteractDyn || tgt[1] == -1) && !(tgt[0] == -1 && tgt[1] == -1);
      };
      for (const InteractView &v : im.views) {
        const NodeDef &vn = m.nodes[v.node];
        std::vector<int64_t> tgt;
        if (vn.op == "Identity") continue;
        if (vn.op == "Flatten" && v.target[0] == 2 && !flattened) flattened++;
        else if (vn.op == "Reshape" && target_rank(v, &tgt) && flat_target(tgt)) flattened += flattened ? 0 : 1;  // ([k * k, N] stays [k * k, N])
        else bad_form(vn, "between Transpose(1,2,0) of the products and their Gather(axis = 0) only the flattening of [k, k, N] to [k * k, N] is matched");
      }
      if (flattened != 1 || (gn.attr_i("axis", 0) != 0 && gn.attr_i("axis", 0) != -2))
        bad_form(gn, "Gather(axis = " + std::to_string(gn.attr_i("axis", 0)) + ") behind Transpose(1,2,0) of the products; only axis 0 of the flattened [k * k, N] matrix");
      std::vector<int64_t> idx;
      if (!interact_eval(im.index_value, zname, k, &idx) || idx.empty())
        bad_form(gn, "its index list is not a constant (constants, Shape of the products, Gather, Mul, Add, Concat over them are folded)");
      const int64_t P = int64_t(idx.size());
      for (const InteractView &v : im.views_after) {  // [P, N] in front of the Transpose(1,0), [N, P] behind it: a Reshape keeps that
        const NodeDef &vn = m.nodes[v.node];
        std::vector<int64_t> tgt;
        if (vn.op == "Identity") continue;
        auto rows_dim = [](int64_t x) { return x == kInteractDyn || x == -1; };
        auto p_dim = [&](int64_t x) { return x == P || x == -1; };
        const bool ok = vn.op == "Reshape" && target_rank(v, &tgt) && tgt.size() == 2 && !(tgt[0] == -1 && tgt[1] == -1) &&
                        (v.back ? (rows_dim(tgt[0]) || tgt[0] == 0) && p_dim(tgt[1]) : p_dim(tgt[0]) && rows_dim(tgt[1]));
        if (!ok) bad_form(vn, std::string("behind the Gather of the products only a Reshape that keeps ") + (v.back ? "[N, P]" : "[P, N]") + " is matched");
      }
      if (const std::string why = interact_refusal(k, d, int64_t(idx.size())); !why.empty()) bad_form(gn, why);
      for (int64_t ix : idx) {
        if (ix < -k * k || ix >= k * k)
          bad_form(gn, "index " + std::to_string(ix) + " is outside [-" + std::to_string(k * k) + ", " + std::to_string(k * k) + ") of the flattened " + std::to_string(k) + " x " +
                           std::to_string(k) + " products");
        pack->sel.push_back(ix < 0 ? ix + k * k : ix);
      }
      shape = {N, P};
    } else {
      const NodeDef &gn = m.nodes[im.gather];
      // the views between the product and the Gather must arrive at [N, k * k]
      std::vector<int64_t> cur = {N, k, k};
      for (const InteractView &v : im.views) {
        const NodeDef &vn = m.nodes[v.node];
        if (vn.op == "Flatten") {
          if (v.target[0] != 1 && v.target[0] != 1 - int64_t(cur.size())) bad_form(vn, "only axis = 1 keeps the row axis");
          cur = {N, prod(cur, 1)};
        } else if (vn.op == "Reshape") {
          std::vector<int64_t> tgt = v.target;
          int64_t rest = 1;
          int neg = -1;
          for (size_t i = 1; i < tgt.size(); i++) {
            if (tgt[i] == 0 && i < cur.size()) tgt[i] = cur[i];
            if (tgt[i] == -1 && neg < 0) neg = int(i);
            else rest *= tgt[i];
          }
          if (neg >= 0 && rest > 0 && k * k % rest == 0) tgt[size_t(neg)] = k * k / rest;
          if (!(tgt[0] == 0 || tgt[0] == -1 || (N > 0 && tgt[0] == N)) || prod(tgt, 1) != k * k || (tgt[0] == -1 && neg >= 0))
            bad_form(vn, "target shape " + shape_str(v.target) + " does not keep the row axis of " + shape_str(cur));
          tgt[0] = N;
          cur = tgt;
        }
      }
      int64_t axis = gn.attr_i("axis", 0);
      if (axis < 0) axis += int64_t(cur.size());
      if (cur.size() != 2 || axis != 1)
        bad_form(gn, "Gather(axis = " + std::to_string(gn.attr_i("axis", 0)) + ") of the products " + shape_str(cur) + "; only a constant list on axis 1 of the flattened matrix [N, k * k]");
      if (const std::string why = interact_refusal(k, d, int64_t(im.idx.size())); !why.empty()) bad_form(gn, why);
      for (int64_t ix : im.idx) {
        if (ix < -k * k || ix >= k * k)
          bad_form(gn, "index " + std::to_string(ix) + " is outside [-" + std::to_string(k * k) + ", " + std::to_string(k * k) + ") of the flattened " + std::to_string(k) + " x " +
                           std::to_string(k) + " products");
        pack->sel.push_back(ix < 0 ? ix + k * k : ix);
      }
      shape = {N, int64_t(im.idx.size())};
    }
    if (im.out_concat != SIZE_MAX) {
      // the other inputs of the Concat as column ranges of T's row: the columns in front of each in the Concat that built T
      const NodeDef &tc = m.nodes[im.t_concat];
      const NodeDef &sel_node = *graph->producer(im.selection_value);
      const int64_t P = shape[1];
      auto width = [&](const std::string &v) -> int64_t {
        if (auto vi = vals.find(v); vi != vals.end() && !vi->second.is_const && vi->second.ra == 0 && !vi->second.shape.empty()) return prod(vi->second.shape, 1);
        if (auto eg = embed_at.find(im.t_concat); eg != embed_at.end())
          for (const EmbedLookup &L : eg->second.lookups)
            if (L.out == v) return prod(L.shape, 1);
        return -1;
      };
      bool known = true;
      int64_t out = 0;
      for (const auto &in : anchor.inputs) {
        if (in == im.selection_value) {
          pack->sel_out = out;
          out += P;
          continue;
        }
        int64_t off = 0;
        for (const auto &ti : tc.inputs) {
          if (ti == in) break;
          const int64_t w = width(ti);
          known = known && w > 0;
          off += w;
        }
        const int64_t w = width(in);
        known = known && w > 0 && off + w <= k * d;
        pack->passes.push_back({off, w, out});
        out += w;
      }
      if (known) {
        shape = {N, out};
      } else {
        // (a column range that cannot be told at load: the selection alone is the step and the Concat copies, as before)
        pack->passes.clear();
        pack->sel_out = 0;
        if (const std::string why = pack_interact(*pack); !why.empty()) bad_form(sel_node, why);
        s.interact = pack;
        s.M = pack->F;
        s.origin.erase(s.origin.rfind('+'));
        set_act(sel_node, push_step(std::move(s), shape), shape);
        return concat(anchor);
      }
    }
    if (const std::string why = pack_interact(*pack); !why.empty()) bad_form(pn, why);
    s.interact = pack;
    s.M = pack->F;
    if (shape.size() == 3) return emit_window(std::move(s), anchor, shape);
    set_act(anchor, push_step(std::move(s), shape), shape);
  }

  Plan Lowerer::run() {
    graph = std::make_unique<const GraphIndex>(m, m.outputs[out_index].name);
    plan.opset = m.opset;
    const onnx::ValueDef &in = m.inputs[0];
    if (!in.has_shape) throw InferaError::onnx("input '" + in.name + "' has no declared shape");
    // (integer inputs: their values arrive as f32 and are truncated toward zero where a preprocessing region first reads them)
    auto served_type = [](int t) { return t == 0 || t == onnx::kFloat || t == onnx::kInt64 || t == onnx::kInt32; };
    const bool half_input = m.inputs.size() == 1 && in.elem_type == onnx::kFloat16;  // (served as f32 values that are rounded to half first)
    for (const auto &v : m.inputs)
      if (!served_type(v.elem_type) && !half_input)
        throw InferaError::onnx("input '" + v.name + "' is not f32, int64 or int32 (element type " + std::to_string(v.elem_type) + ")");
    if (in.dims.size() < 2) throw InferaError::onnx("input rank " + std::to_string(in.dims.size()) + " has no row axis + feature axis; rank >= 2 is required");
    check_shuffle_extents(in);  // (a DepthToSpace / SpaceToDepth on a symbolic image: refused by the node's name)
    for (size_t i = 1; i < in.dims.size(); i++)
      if (in.dims[i] <= 0) throw InferaError::onnx("only the leading (row/batch) dimension of the input may be symbolic, got " + shape_str(in.dims));
    plan.input_shape = in.dims;
    if (in.dims[0] > 0) plan.fixed_batch = in.dims[0];
    else plan.input_shape[0] = -1;
    if (m.inputs.size() > 1) {
      // Several runtime inputs (the reference feeds input 0 only, engine.rs:139-145, so such a model cannot run
      // there at all): the feature columns of the call are split across the inputs in declaration order.  Every
      // input must be an f32 [rows, k_i] matrix with the same leading dimension.  A rank-1 [rows] int32 / int64 input counts as one
      // column (the length column of padded windows: sequence_lens is rank 1).
      int64_t total = 0;
      for (const auto &v : m.inputs) {
        const bool one_col = v.has_shape && v.dims.size() == 1 && (v.elem_type == onnx::kInt64 || v.elem_type == onnx::kInt32);
        if (!v.has_shape || (v.dims.size() != 2 && !one_col) || (!one_col && v.dims[1] <= 0) || !served_type(v.elem_type) ||
            (v.dims[0] > 0 ? v.dims[0] : -1) != plan.input_shape[0])
          throw InferaError::onnx("multi-input models need f32 [rows, k] inputs with one common leading dimension; input '" + v.name + "' is " +
                                  (v.has_shape ? shape_str(v.dims) : std::string("unshaped")));
        total += input_cols(v);
      }
      plan.input_shape[1] = total;
    }
    {
      Val v;
      v.buf = new_buf(plan.input_shape);
      v.shape = plan.input_shape;
      if (half_input) {  // the C ABI hands over f32: the input is rounded first (an HDense layer that reads it does so on load and drops this step)
        plan.input_declared_type = "float16";
        Step r;
        r.kind = StepKind::RoundHalf;
        r.in0 = v.buf;
        r.origin = "input:" + in.name;
        v.buf = push_step(std::move(r), plan.input_shape);
        v.half = true;
        half_bufs.insert(v.buf);
      }
      if (m.inputs.size() == 1) {
        vals[in.name] = v;
        buf_names[v.buf].push_back(in.name);
      }
    }
    auto int_input = [](const onnx::ValueDef &v) { return v.elem_type == onnx::kInt64 || v.elem_type == onnx::kInt32; };
    const std::vector<char> &live = graph->live;
    for (size_t i = 0; i < m.nodes.size(); i++)
      if (live[i])
        for (const auto &in_name : m.nodes[i].inputs) uses[in_name]++;
    uses[m.outputs[out_index].name]++;
    // The matchers below claim nodes through `region` and `absorbed` and otherwise read the index alone: a later one skips what an
    // earlier one claimed, and none depends on another having run.
    absorbed.assign(m.nodes.size(), 0);
    // preprocessing regions: their graph inputs start as identity columns over the input buffer (integer inputs truncated)
    const std::set<std::string> region_inputs = find_regions();
    find_interactions();
    find_attention_ops();  // (before find_attention, whose tail absorbs the row-mask sub-graphs of every match)
    find_attention();
    check_rotary_ops();
    if (nearest_enabled) find_nearest();
    if (nearest_enabled) find_votes();  // (INFERA_NEAREST=0 has no plan for the vote: Equal stays unsupported, the load is refused as without the matcher)
    find_group_norms();
    find_pixel_shuffles();
    find_embeds();
    find_seq_lens();
    {
      int64_t off = 0;
      for (const auto &v : m.inputs) {
        const int64_t w = m.inputs.size() == 1 ? prod(plan.input_shape, 1) : input_cols(v);
        if (region_inputs.count(v.name)) {
          if (m.inputs.size() == 1 && plan.input_shape.size() != 2 && int_input(v))
            throw InferaError::onnx("integer input '" + v.name + "' must be [rows, k]");
          PrepVal p = prep_identity(0, off, w, int_input(v), false);
          if (int_input(v)) p.origin.push_back("input:" + v.name);
          set_prep(v.name, std::move(p), m.inputs.size() == 1 ? plan.input_shape : v.dims.size() == 1 ? std::vector<int64_t>{plan.input_shape[0]} : std::vector<int64_t>{plan.input_shape[0], w});
        }
        off += w;
      }
    }

    if (m.inputs.size() > 1) {
      Val all;  // the [rows, sum of k] input buffer
      all.buf = 0;
      all.shape = plan.input_shape;
      int64_t off = 0;
      for (const auto &v : m.inputs) {
        if (uses.count(v.name) && uses[v.name] > 0 && !region_inputs.count(v.name)) {
          emit_slice_cols("input:" + v.name, all, off, off + input_cols(v), v.name);
          if (v.dims.size() == 1) vals[v.name].shape = {plan.input_shape[0]};
        }
        off += input_cols(v);
      }
    }
    for (size_t ni = 0; ni < m.nodes.size(); ni++) {
      if (!live[ni]) continue;
      const auto &n = m.nodes[ni];
      if (n.outputs.empty()) throw InferaError::onnx("node " + n.op + " has no outputs");
      if (auto vt = vote_of_topk.find(ni); vt != vote_of_topk.end()) vote_begin(vt->second);  // (takes the k-NN vote behind this TopK, or gives its nodes back)
      if (!vote_inside.empty() && vote_inside[ni]) continue;
      if (region[ni] || n.domain == "ai.onnx.ml") check_row_axis(n, false);
      if (region[ni]) prep_node(n);
      else if (n.domain == "ai.onnx.ml") ml_node(n);
      else if (n.domain == "com.microsoft" && n.op == "CDist") lower_typed(n, [&] { cdist(n); });
      else if (!n.domain.empty() && n.domain != "ai.onnx") {
        if (n.op == "Attention" || n.op == "MultiHeadAttention" || n.op == "SkipLayerNormalization")
          unsupported(n, "unsupported operator form: the contrib fused operator of domain '" + n.domain +
                             "' is not supported; export the standard-domain graph (MatMul / Softmax / LayerNormalization)");
        if (n.op == "RotaryEmbedding")
          unsupported(n, "unsupported operator form: the contrib RotaryEmbedding of domain '" + n.domain + "' is not supported; export the standard-domain RotaryEmbedding (opset 23)");
        unsupported(n, "operator domain '" + n.domain + "'");
      } else if (attn_at.count(ni)) lower_typed(n, [&] { lower_attention(attn_at.at(ni), n); });
      else if (nearest_at.count(ni)) lower_nearest(nearest_at.at(ni));
      else if (vote_at.count(ni) && vote_at.at(ni).np) lower_vote(vote_at.at(ni));
      else if (embed_at.count(ni)) lower_embed(embed_at.at(ni), n);
      else if (interact_at.count(ni)) {
        const InteractMatch &im = interact_at.at(ni);
        if (interact_released(im)) {  // the operators one by one, as without the matcher: their inputs all stand in front of the first of them
          std::vector<size_t> all = im.nodes;
          all.push_back(ni);
          std::sort(all.begin(), all.end());
          for (size_t i : all) lower_typed(m.nodes[i], [&] { lower_node(m.nodes[i]); });
        } else {
          lower_typed(n, [&] { lower_interact(im, n); });
        }
      }
      else if (mmean_at.count(ni)) lower_typed(n, [&] { lower_masked_mean(mmean_at.at(ni), n); });
      else if (absorbed[ni]) continue;
      else if (gn_at.count(ni)) lower_typed(n, [&] { if (!exporter_group_norm(gn_at.at(ni), n)) lower_node(n); });
      else if (shuffle_at.count(ni)) {
        const ShuffleMatch &sm = shuffle_at.at(ni);
        if (!pixel_shuffle_spelling(sm, n))  // the operators one by one, as without the matcher
          for (size_t i : {sm.first, sm.transpose, ni}) lower_typed(m.nodes[i], [&] { lower_node(m.nodes[i]); });
      }
      else lower_typed(n, [&] { lower_node(n); });
    }
    // one output is served: the first (engine.rs:146-149) unless the load call selected another
    const onnx::ValueDef &out = m.outputs[out_index];
    auto it = vals.find(out.name);
    if (it == vals.end()) throw InferaError::onnx("output '" + out.name + "' is never produced");
    if (it->second.pv) materialize(out.name, nullptr);
    if (it->second.nn) materialize_nearest(out.name);
    if (it->second.q) bad_form(*quant_node.at(out.name), "its quantised result is the graph output '" + out.name + "'; end the graph with DequantizeLinear");
    if (it->second.cl) {
      for (const auto &nd : m.nodes)
        if (std::find(nd.outputs.begin(), nd.outputs.end(), out.name) != nd.outputs.end())
          bad_form(nd, "its result " + shape_str(it->second.shape) + " is a channels-last view and the graph output '" + out.name + "'; results are served in [N,C,H,W] order: end the graph with Transpose(0,3,1,2)");
    }
    if (it->second.is_const) throw InferaError::onnx("output '" + out.name + "' is a constant; nothing to run");
    if (it->second.padded()) throw InferaError::onnx("output '" + out.name + "' is a Pad result; padding is only folded into a following Conv");
    if (it->second.ra != 0)
      throw InferaError::onnx("output '" + out.name + "' " + shape_str(it->second.shape) + " is time-major (its row axis is axis " + std::to_string(it->second.ra) +
                              "); results are served rows first: transpose it in the graph (Transpose(1,0,2)) or use layout = 1");
    if (out.elem_type == onnx::kFloat16 && it->second.half) {
      plan.output_declared_type = "float16";  // (half values are f32 values: served exactly)
    } else if (out.elem_type != 0 && out.elem_type != onnx::kFloat) {
      // integer outputs (ArgMax labels, Cast to int) are returned as f32 VALUES: the C ABI carries f32 only
      // (rust.h:28-49; the reference itself rejects non-f32 outputs at engine.rs:150-152)
      const bool int_valued = int_bufs.count(it->second.buf) > 0;
      if (!(int_valued && (out.elem_type == onnx::kInt64 || out.elem_type == onnx::kInt32)))
        throw InferaError::onnx("output '" + out.name + "' is not f32");
      plan.output_declared_type = out.elem_type == onnx::kInt64 ? "int64" : "int32";
    }
    plan.output_name = out.name;
    plan.out_buf = it->second.buf;
    plan.output_shape = it->second.shape;
    if (plan.fixed_batch < 0) plan.output_shape[0] = -1;
    // declared output dims must agree where both are known
    if (out.has_shape) {
      if (out.dims.size() != plan.output_shape.size())
        throw InferaError::onnx("declared output rank " + std::to_string(out.dims.size()) + " differs from inferred " + shape_str(plan.output_shape));
      for (size_t i = 0; i < out.dims.size(); i++)
        if (out.dims[i] > 0 && plan.output_shape[i] > 0 && out.dims[i] != plan.output_shape[i])
          throw InferaError::onnx("declared output shape " + shape_str(out.dims) + " conflicts with inferred " + shape_str(plan.output_shape));
    }
    insert_half_roundings();
    drop_unread_fake_quants();
    return std::move(plan);
  }
  // A FakeQuant whose every reader was a quantised layer that rounds its input itself (two convolutions of a residual block reading one
  // tensor) is read by nothing: its step goes.  (One with a single such reader went when that reader was lowered, sole_tail.)
  void Lowerer::drop_unread_fake_quants() {
    std::set<int> read = {plan.out_buf};
    for (const Step &s : plan.steps)
      for (int b : {s.in0, s.in1, s.in2, s.in3}) read.insert(b);
    plan.steps.erase(std::remove_if(plan.steps.begin(), plan.steps.end(), [&](const Step &s) { return s.kind == StepKind::FakeQuant && !read.count(s.out); }),
                     plan.steps.end());
  }

}  // namespace lowering

Plan lower_model(const onnx::Model &m, const std::string &output_select) { return lowering::Lowerer(m, output_select).run(); }

}  // namespace infera_hip
