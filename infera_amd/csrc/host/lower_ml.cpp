// lower_ml.cpp -- struct Lowerer (lowerer.hpp): the ai.onnx.ml linear heads, tree ensembles, SVM and ZipMap.
// It has no state of its own: it works on the shared state at the head of struct Lowerer (lowerer.hpp);
// which graphs are served and which are refused: INTEGRATION.md section 2.6.
#include <algorithm>

#include "lowerer.hpp"
#include "svm.hpp"
#include "trees.hpp"

namespace infera_hip {

namespace lowering {

// ---- ai.onnx.ml: the classical-ML nodes sklearn exporters write (tract-onnx 0.22 ops/ml is what serves them for
// the reference, engine.rs:49-56).  Each is rewritten into the standard operators above, so a Scaler folds into the
// linear model behind it and a LinearClassifier's scores go through the Dense (+Softmax) kernels; semantics follow
// the ONNX-ML operator specification (tract's sources are not in /root/reference).
NodeDef Lowerer::std_node(const NodeDef &from, const char *op, std::vector<std::string> in, std::string out) {
  NodeDef d;
  d.op = op;
  d.name = from.name.empty() ? from.op : from.op + ":" + from.name;
  d.inputs = std::move(in);
  d.outputs = {std::move(out)};
  return d;
}
void Lowerer::set_i(NodeDef &d, const char *k, int64_t v) {
  onnx::Attribute a;
  a.name = k;
  a.type = 2;
  a.i = v;
  d.attrs[k] = a;
}
bool Lowerer::wanted(const NodeDef &n, size_t i) const {
  if (i >= n.outputs.size() || n.outputs[i].empty()) return false;
  auto it = uses.find(n.outputs[i]);
  return it != uses.end() && it->second > 0;
}
std::vector<float> Lowerer::ml_floats(const NodeDef &n, const char *k, int64_t want, float dflt, bool allow_scalar) {
  const onnx::Attribute *a = n.attr(k);
  std::vector<float> v = a ? a->floats : std::vector<float>{};
  if (v.empty()) return std::vector<float>(size_t(want), dflt);
  if (allow_scalar && v.size() == 1) return std::vector<float>(size_t(want), v[0]);
  if (int64_t(v.size()) != want) unsupported(n, std::string(k) + " holds " + std::to_string(v.size()) + " values, expected " + std::to_string(want));
  return v;
}
// post_transform over raw scores `raw` -> value `out`
void Lowerer::ml_post_transform(const NodeDef &n, const std::string &raw, const std::string &out) {
  const std::string pt = n.attr_s("post_transform", "NONE");
  if (pt == "NONE") lower_node(std_node(n, "Identity", {raw}, out));
  else if (pt == "LOGISTIC") lower_node(std_node(n, "Sigmoid", {raw}, out));
  else if (pt == "SOFTMAX") {
    NodeDef d = std_node(n, "Softmax", {raw}, out);
    set_i(d, "axis", 1);
    lower_node(d);
  } else unsupported(n, "post_transform " + pt);
}
// output 0 of n = a0 + step * index (the label of an evenly spaced class table; not both a0 = 0 and step = 1): a Mul and / or an Add on the
// whole-numbered `index`.  (Tables of int64 labels pass their a0 and step as doubles: float(double(v)) == float(v) for |v| < 2^53.)
void Lowerer::label_from_index(const NodeDef &n, std::string index, double a0, double step) {
  const std::string tmp = n.outputs[0] + "\x01";
  if (step != 1.0) {
    vals[tmp + "step"] = const_f32({float(step)}, {});
    const std::string nxt = a0 == 0.0 ? n.outputs[0] : tmp + "scaled";
    if (nxt != n.outputs[0]) uses[nxt] = 1;
    lower_node(std_node(n, "Mul", {index, tmp + "step"}, nxt));
    index = nxt;
  }
  if (a0 != 0.0) {
    vals[tmp + "first"] = const_f32({float(a0)}, {});
    lower_node(std_node(n, "Add", {index, tmp + "first"}, n.outputs[0]));
  }
}
// ArrayFeatureExtractor: Y = X[..., indices].  Two forms occur in exported pipelines: a constant class table indexed
// by the ArgMax of the scores (label lookup; the table must be evenly spaced, then it is one multiply-add on the
// index), and a contiguous column range picked out of the feature matrix.
void Lowerer::array_feature_extractor(const NodeDef &n) {
  const Val &x = get(n, 0);
  const Val &ix = get(n, 1);
  if (x.is_const && !ix.is_const) {
    if (!int_bufs.count(ix.buf)) unsupported(n, "indices must be whole numbers (an ArgMax output)");
    if (x.shape.size() != 1) unsupported(n, "only a 1-D class table");
    std::vector<double> tab;
    if (x.c->dtype == onnx::kInt64) tab.assign(x.c->i64.begin(), x.c->i64.end());
    else tab.assign(x.c->f32.begin(), x.c->f32.end());
    if (tab.size() < 2) unsupported(n, "class table needs two entries");
    const double a0 = tab[0], step = tab[1] - tab[0];
    for (size_t i = 0; i < tab.size(); i++)
      if (tab[i] != a0 + step * double(i)) unsupported(n, "class table must be evenly spaced (label = a + b * index)");
    if (step == 1.0 && a0 == 0.0) lower_node(std_node(n, "Identity", {n.inputs[1]}, n.outputs[0]));
    else label_from_index(n, n.inputs[1], a0, step);
    return;
  }
  if (!x.is_const && ix.is_const && x.shape.size() == 2 && ix.c->dtype == onnx::kInt64 && !ix.c->i64.empty()) {
    const auto &v = ix.c->i64;
    for (size_t i = 1; i < v.size(); i++)
      if (v[i] != v[0] + int64_t(i)) unsupported(n, "only a contiguous column range");
    if (v[0] < 0 || v[0] + int64_t(v.size()) > x.shape[1]) unsupported(n, "column index out of range");
    const Val src = x;
    emit_slice_cols(node_label(n), src, v[0], v[0] + int64_t(v.size()), n.outputs[0]);
    return;
  }
  unsupported(n, "only (constant table, index activation) or (activation, constant contiguous indices)");
}
// The two-stage head of a tree ensemble / SVM node: kernel step `k` writes its partials [rows, part_cols]; a copy of `r` (the reduce
// step's kind and pack) turns them into a classifier's label (output 0, when read) with `label_mode`, and another into the raw scores
// [rows, score_cols] with `score_mode`, which post_transform turns into the scores output
void Lowerer::ml_head(const NodeDef &n, bool cls, Step k, int64_t part_cols, Step r, int label_mode, int score_mode, int64_t score_cols) {
  const int64_t rows = get_raw(n, 0).shape[0];
  const bool want_label = cls && wanted(n, 0), want_scores = cls ? wanted(n, 1) : true;
  const std::string tmp = n.outputs[0] + "\x01";
  k.out_mode = want_scores ? score_mode : label_mode;
  NodeDef kn = n;
  kn.outputs = {tmp + "partial"};
  r.in0 = emit(std::move(k), kn, {rows, part_cols}).out;
  auto reduce = [&](int mode, const std::string &out, const std::vector<int64_t> &shape) {
    Step s = r;
    s.out_mode = mode;
    NodeDef d = n;
    d.outputs = {out};
    return emit(std::move(s), d, shape).out;
  };
  if (want_label) int_bufs.insert(reduce(label_mode, n.outputs[0], {rows}));
  if (want_scores) {
    const std::string raw = tmp + "raw";
    uses[raw] = 1;
    reduce(score_mode, raw, {rows, score_cols});
    ml_post_transform(n, raw, cls ? n.outputs[1] : n.outputs[0]);
  }
}
// TreeEnsembleRegressor / TreeEnsembleClassifier: a TreeEnsemble step (walk, per-slice partial sums) and a TreeReduce step (slices
// summed in fixed order, AVERAGE, base_values, binary expansion or the label), then post_transform on the scores
void Lowerer::tree_ensemble(const NodeDef &n) {
  std::shared_ptr<const TreePack> tp;
  const Val &x = get(n, 0);
  if (x.is_const || x.shape.size() != 2) unsupported(n, "only [rows, features] activations");
  try {
    tp = std::make_shared<const TreePack>(pack_tree_ensemble(n, x.shape[1]));
  } catch (const TreeError &e) {
    unsupported(n, e.what());
  }
  Step w, r;
  w.kind = StepKind::TreeEnsemble;
  w.in0 = x.buf;
  r.kind = StepKind::TreeReduce;
  w.tree = r.tree = tp;
  // (the partials are f64, as f32 pairs)
  ml_head(n, tp->classifier, std::move(w), 2 * tp->slices * tp->W, std::move(r), tp->binary ? kTreeBinaryLabel : kTreeLabel,
          tp->binary ? kTreeBinaryScores : kTreeScores, tp->E);
}
// SVMRegressor / SVMClassifier: an SvmKernel step (X . S^T on the matrix cores, the kernel function, times the coefficients: per-slice
// partial sums) and an SvmReduce step (slices summed in fixed order, rho, then the value, one-class sign, pairwise decisions, votes and
// label, or Platt + pairwise coupling), then post_transform on the scores
void Lowerer::svm(const NodeDef &n) {
  std::shared_ptr<const SvmPack> sp;
  const Val &x = get(n, 0);
  if (x.is_const || x.shape.size() != 2) unsupported(n, "only [rows, features] activations");
  try {
    sp = std::make_shared<const SvmPack>(pack_svm(n, x.shape[1]));
  } catch (const SvmError &e) {
    unsupported(n, e.what());
  }
  const int64_t C = sp->classes, P = C * (C - 1) / 2;
  const bool cls = sp->classifier;
  const int score_mode = !cls ? (sp->one_class ? kSvmOneClass : kSvmValue) : sp->probabilities ? kSvmProb : kSvmDecision;
  const int64_t score_cols = !cls ? 1 : sp->probabilities ? C : (C == 2 ? 2 : P);
  Step k, r;
  k.kind = StepKind::SvmKernel;
  k.in0 = x.buf;
  r.kind = StepKind::SvmReduce;
  k.svm = r.svm = sp;
  ml_head(n, cls, std::move(k), sp->slices * sp->Q, std::move(r), kSvmLabel, score_mode, score_cols);
}
// ZipMap (probabilities -> a sequence of maps), when its output is the one served: the C ABI carries f32 rows, so the probabilities
// [rows, C] it reads are served, one column per class in classlabels order (get_model_info says so)
void Lowerer::zipmap(const NodeDef &n) {
  const Val &x = get(n, 0);
  if (x.is_const || x.shape.size() != 2) unsupported(n, "only [rows, classes] probabilities");
  size_t labels = 0;
  if (const onnx::Attribute *a = n.attr("classlabels_int64s")) labels = a->ints.size();
  if (const onnx::Attribute *a = n.attr("classlabels_strings")) labels = std::max(labels, a->strings.size());
  if (int64_t(labels) != x.shape[1])
    unsupported(n, "classlabels hold " + std::to_string(labels) + " labels for " + std::to_string(x.shape[1]) + " probability columns");
  const std::vector<int64_t> shape = x.shape;
  set_act(n, x.buf, shape, true);
  if (n.outputs[0] == m.outputs[out_index].name) plan.output_zipmap = true;
}
void Lowerer::ml_node(const NodeDef &n) {
  if (n.op == "ArrayFeatureExtractor") return array_feature_extractor(n);
  if (n.op == "TreeEnsembleRegressor" || n.op == "TreeEnsembleClassifier") return tree_ensemble(n);
  if (n.op == "SVMRegressor" || n.op == "SVMClassifier") return svm(n);
  if (n.op == "ZipMap") return zipmap(n);
  const Val &x = get(n, 0);
  if (x.is_const || x.shape.size() != 2) unsupported(n, "only [rows, features] activations");
  const int64_t F = x.shape[1];
  const std::string tmp = n.outputs[0] + "\x01";
  if (n.op == "Scaler") {
    vals[tmp + "offset"] = const_f32(ml_floats(n, "offset", F, 0.f, true), {F});
    vals[tmp + "scale"] = const_f32(ml_floats(n, "scale", F, 1.f, true), {F});
    uses[tmp + "centered"] = 1;
    lower_node(std_node(n, "Sub", {n.inputs[0], tmp + "offset"}, tmp + "centered"));
    lower_node(std_node(n, "Mul", {tmp + "centered", tmp + "scale"}, n.outputs[0]));
  } else if (n.op == "LinearRegressor" || n.op == "LinearClassifier") {
    const bool cls = n.op == "LinearClassifier";
    std::vector<int64_t> labels;
    if (cls) {
      if (n.attr("classlabels_strings")) unsupported(n, "string class labels cannot be returned as numbers");
      if (auto *p = n.attr_ints("classlabels_ints")) labels = *p;
      if (labels.size() < 2) unsupported(n, "needs at least two classlabels_ints");
    }
    const int64_t E = cls ? int64_t(labels.size()) : n.attr_i("targets", 1);
    if (E < 1) unsupported(n, "targets must be positive");
    vals[tmp + "coef"] = const_f32(ml_floats(n, "coefficients", E * F, 0.f, false), {E, F});
    vals[tmp + "icpt"] = const_f32(ml_floats(n, "intercepts", E, 0.f, false), {E});
    const bool want_label = cls && wanted(n, 0), want_scores = cls ? wanted(n, 1) : true;
    const std::string raw = tmp + "raw";
    uses[raw] = int(want_label) + int(want_scores);
    NodeDef g = std_node(n, "Gemm", {n.inputs[0], tmp + "coef", tmp + "icpt"}, raw);
    set_i(g, "transB", 1);
    lower_node(g);
    if (want_label) {
      // label = classlabels_ints[argmax(raw scores)]; the class table must be an arithmetic progression
      // (0..E-1, 1..E, {-1, 1}, ...), which is then one multiply-add on the index
      const int64_t a0 = labels[0], step = labels[1] - labels[0];
      for (size_t i = 0; i < labels.size(); i++)
        if (labels[i] != a0 + step * int64_t(i)) unsupported(n, "classlabels_ints must be evenly spaced (label = a + b * index)");
      const std::string index = (step == 1 && a0 == 0) ? n.outputs[0] : tmp + "index";
      if (index != n.outputs[0]) uses[index] = 1;
      NodeDef am = std_node(n, "ArgMax", {raw}, index);
      set_i(am, "axis", 1);
      set_i(am, "keepdims", 0);
      lower_node(am);
      if (step != 1 || a0 != 0) label_from_index(n, index, double(a0), double(step));
    }
    if (want_scores) ml_post_transform(n, raw, cls ? n.outputs[1] : n.outputs[0]);
  } else if (n.op == "Normalizer") {
    const std::string norm = n.attr_s("norm", "MAX");
    Step s;
    s.kind = StepKind::Softmax;
    s.in0 = x.buf;
    s.sm_norm = norm == "MAX" ? 1 : norm == "L1" ? 2 : norm == "L2" ? 3 : 0;
    if (!s.sm_norm) unsupported(n, "norm " + norm);
    s.sm_len = F;
    std::vector<int64_t> shape = x.shape;
    emit(std::move(s), n, shape);
  } else {
    unsupported(n, "unsupported operator");
  }
}

}  // namespace lowering

}  // namespace infera_hip
