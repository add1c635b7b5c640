// lower_nearest.cpp -- struct Lowerer (lowerer.hpp): distance models.
// The state, the match structs and the block that explains them stand in lowerer.hpp under "distance models";
// which graphs are served and which are refused: INTEGRATION.md section 2.6.
#include <algorithm>
#include <cmath>

#include "lowerer.hpp"
#include "nearest.hpp"

namespace infera_hip {

namespace lowering {

// a constant f32 tensor known before the walk: an initializer or a Constant node's value
std::shared_ptr<TensorData> Lowerer::const_tensor(const std::string &name) const {
  const std::shared_ptr<TensorData> t = graph->constant(name).t;
  return t && t->dtype == onnx::kFloat ? t : nullptr;
}
// g = -2 X C^T read by one node: the set (and its orientation) and the nodes of the chain
bool Lowerer::match_minus_two_dot(const std::string &g, const std::string &x, NearestMatch *mt) {
  size_t gi = 0;
  const NodeDef *p = graph->producer(g, &gi);
  if (!p || !only_reader(g) || !p->domain.empty()) return false;
  if (p->op == "Gemm") {
    if (p->inputs.size() < 2 || p->inputs[0] != x || p->attr_i("transA", 0) != 0 || p->attr_f("alpha", 1.f) != -2.f) return false;
    auto c = const_tensor(p->inputs[1]);
    if (!c || c->dims.size() != 2) return false;
    if (p->inputs.size() > 2 && !p->inputs[2].empty()) {
      auto z = const_tensor(p->inputs[2]);
      if (!z || std::any_of(z->f32.begin(), z->f32.end(), [](float v) { return v != 0.f; })) return false;
    }
    mt->c = c;
    mt->c_fm = p->attr_i("transB", 0) == 0;
    mt->spelling = "gemm";
    mt->nodes.push_back(gi);
    return true;
  }
  if (p->op != "Mul" || p->inputs.size() != 2) return false;
  for (int side = 0; side < 2; side++) {
    auto k = const_tensor(p->inputs[size_t(1 - side)]);
    if (!k || k->f32.size() != 1 || k->f32[0] != -2.f) continue;
    size_t mi = 0;
    const NodeDef *mm = graph->producer(p->inputs[size_t(side)], &mi);
    if (!mm || mm->op != "MatMul" || !mm->domain.empty() || mm->inputs.size() != 2 || mm->inputs[0] != x || !only_reader(mm->outputs[0])) return false;
    auto c = const_tensor(mm->inputs[1]);
    if (!c || c->dims.size() != 2) return false;
    mt->c = c;
    mt->c_fm = true;
    mt->spelling = "matmul_mul";
    mt->nodes.push_back(mi);
    mt->nodes.push_back(gi);
    return true;
  }
  return false;
}
void Lowerer::find_nearest() {
  for (size_t i = 0; i < m.nodes.size(); i++) {
    const NodeDef &rs = m.nodes[i];
    if (!graph->live[i] || absorbed[i] || region[i] || rs.op != "ReduceSumSquare" || !rs.domain.empty() || rs.inputs.empty() || rs.attr_i("keepdims", 1) == 0) continue;
    std::vector<int64_t> axes;
    if (rs.inputs.size() > 1 && !rs.inputs[1].empty()) {
      auto ci = m.initializers.find(rs.inputs[1]);
      if (ci == m.initializers.end() || ci->second->dtype != onnx::kInt64) continue;
      axes = ci->second->i64;
    } else if (auto *p = rs.attr_ints("axes")) axes = *p;
    if (axes.size() != 1 || (axes[0] != 1 && axes[0] != -1)) continue;
    NearestMatch mt;
    mt.x = rs.inputs[0];
    const NodeDef *a1 = only_reader(rs.outputs[0]);
    if (!a1 || a1->op != "Add" || !a1->domain.empty() || a1->inputs.size() != 2 || a1->inputs[0] == a1->inputs[1]) continue;
    const std::string other = a1->inputs[a1->inputs[0] == rs.outputs[0] ? 1 : 0];
    std::shared_ptr<TensorData> c2;
    mt.nodes.push_back(i);
    mt.nodes.push_back(size_t(a1 - m.nodes.data()));
    if (match_minus_two_dot(other, mt.x, &mt)) {  // (rs + g) + C2
      const NodeDef *a2 = only_reader(a1->outputs[0]);
      if (!a2 || a2->op != "Add" || !a2->domain.empty() || a2->inputs.size() != 2) continue;
      c2 = const_tensor(a2->inputs[a2->inputs[0] == a1->outputs[0] ? 1 : 0]);
      mt.nodes.push_back(size_t(a2 - m.nodes.data()));
      mt.d2 = a2->outputs[0];
    } else {  // rs + (g + C2)
      size_t bi = 0;
      const NodeDef *b = graph->producer(other, &bi);
      if (!b || b->op != "Add" || !b->domain.empty() || b->inputs.size() != 2 || !only_reader(other)) continue;
      int gs = -1;
      for (int side = 0; side < 2 && gs < 0; side++)
        if ((c2 = const_tensor(b->inputs[size_t(1 - side)])) && match_minus_two_dot(b->inputs[size_t(side)], mt.x, &mt)) gs = side;
      if (gs < 0) continue;
      mt.nodes.push_back(bi);
      mt.d2 = a1->outputs[0];
    }
    if (!c2 || !mt.c) continue;
    const int64_t M = mt.c->dims[mt.c_fm ? 1 : 0], F = mt.c->dims[mt.c_fm ? 0 : 1];
    if (M < 1 || F < 1 || int64_t(mt.c->f32.size()) != M * F || int64_t(c2->f32.size()) != M) continue;
    if (!(c2->dims.size() == 1 || (c2->dims.size() == 2 && c2->dims[0] == 1))) continue;
    bool norms = true;  // C2[m] = sum_f C[m, f]^2 within F 2^-23 of it
    for (int64_t j = 0; j < M && norms; j++) {
      double a = 0.0;
      for (int64_t k = 0; k < F; k++) {
        const double v = mt.c->f32[size_t(mt.c_fm ? k * M + j : j * F + k)];
        a += v * v;
      }
      norms = std::fabs(double(c2->f32[size_t(j)]) - a) <= double(F) * std::ldexp(1.0, -23) * a;
    }
    if (!norms) continue;
    std::sort(mt.nodes.begin(), mt.nodes.end());
    bool fresh = true;
    for (size_t q : mt.nodes) fresh = fresh && !absorbed[q] && !region[q] && !attn_at.count(q);
    if (!fresh) continue;
    for (size_t q : mt.nodes) absorbed[q] = 1;
    nearest_at[mt.nodes.back()] = std::move(mt);
  }
}
// the pending value of a recognised set; a form the kernel does not take (a time-major, half or quantised X, another width) returns false
bool Lowerer::bind_nearest(const NodeDef &anchor, const std::string &x_name, const std::string &out, const float *C, int64_t M, int64_t F, const std::string &spelling,
                           bool rooted, const std::string &origin) {
  const Val *xp = find_value(x_name);
  if (!xp) unsupported(anchor, "input '" + x_name + "' is not produced by any earlier node");
  if (xp->pv) materialize(x_name, &anchor);
  if (xp->nn) materialize_nearest(x_name);
  const Val x = *find_value(x_name);
  if (x.is_const || x.q || x.half || x.ra != 0 || x.padded() || x.shape.size() != 2 || x.shape[1] != F) return false;
  auto np = std::make_shared<NearestPending>();
  try {
    np->pack = std::make_shared<const NearestPack>(pack_nearest(C, M, F, spelling));
  } catch (const NearestError &e) {
    unsupported(anchor, e.what());
  }
  np->in_buf = x.buf;
  np->rows = x.shape[0];
  np->rooted = rooted;
  np->origin = origin;
  Val v;
  v.nn = np;
  v.shape = {x.shape[0], M};
  vals[out] = v;
  return true;
}
void Lowerer::lower_nearest(const NearestMatch &mt) {
  const NodeDef &anchor = m.nodes[mt.nodes.back()];
  const int64_t M = mt.c->dims[mt.c_fm ? 1 : 0], F = mt.c->dims[mt.c_fm ? 0 : 1];
  std::vector<float> c(size_t(M * F));
  for (int64_t j = 0; j < M; j++)
    for (int64_t k = 0; k < F; k++) c[size_t(j * F + k)] = mt.c->f32[size_t(mt.c_fm ? k * M + j : j * F + k)];
  if (bind_nearest(anchor, mt.x, mt.d2, c.data(), M, F, mt.spelling, false, node_label(m.nodes[mt.nodes.front()]) + "+...+" + node_label(anchor))) return;
  for (size_t q : mt.nodes) lower_typed(m.nodes[q], [&] { lower_node(m.nodes[q]); });  // not the kernel's form: operator by operator
}
void Lowerer::set_f(NodeDef &d, const char *k, float v) {
  onnx::Attribute a;
  a.name = k;
  a.type = 1;
  a.f = v;
  d.attrs[k] = a;
}
// com.microsoft CDist(X, C, metric): the distances in one node (what skl2onnx writes for neighbour models under optim = 'cdist')
void Lowerer::cdist(const NodeDef &n) {
  const std::string metric = n.attr_s("metric", "sqeuclidean");
  if (metric != "sqeuclidean" && metric != "euclidean") bad_form(n, "metric '" + metric + "' (only sqeuclidean and euclidean)");
  if (n.inputs.size() != 2) bad_form(n, "needs the two inputs X and the reference set");
  const Val &cv = get(n, 1);
  if (!cv.is_const || cv.c->dtype != onnx::kFloat || cv.shape.size() != 2) bad_form(n, "the reference set must be a constant f32 [M, F] matrix");
  const int64_t M = cv.shape[0], F = cv.shape[1];
  const bool rooted = metric == "euclidean";
  const std::shared_ptr<TensorData> ct = cv.c;
  if (int64_t(ct->f32.size()) != M * F || M < 1 || F < 1) bad_form(n, "the reference set " + shape_str(cv.shape) + " does not match its data");
  const Val &x0 = get(n, 0);
  if (x0.is_const || x0.shape.size() != 2 || x0.shape[1] != F) bad_form(n, "X must be a [rows, " + std::to_string(F) + "] activation, got " + shape_str(x0.shape));
  if (nearest_enabled && bind_nearest(n, n.inputs[0], n.outputs[0], ct->f32.data(), M, F, "cdist", rooted, node_label(n))) return;
  try {
    (void)pack_nearest(ct->f32.data(), M, F, "cdist");  // (the caps hold for either lowering)
  } catch (const NearestError &e) {
    unsupported(n, e.what());
  }
  // operator by operator: |x|^2 - 2 x . C^T + |c|^2 [, Sqrt]
  const std::string tmp = n.outputs[0] + "\x01";
  std::vector<float> c2(static_cast<size_t>(M));
  for (int64_t j = 0; j < M; j++) {
    double a = 0.0;
    for (int64_t k = 0; k < F; k++) a += double(ct->f32[size_t(j * F + k)]) * double(ct->f32[size_t(j * F + k)]);
    c2[size_t(j)] = float(a);
  }
  vals[tmp + "c2"] = const_f32(std::move(c2), {M});
  vals[tmp + "axes"] = const_i64({1}, {1});
  for (const char *t : {"rs", "g", "z", "d2"}) uses[tmp + t] = 1;
  NodeDef rs = std_node(n, "ReduceSumSquare", {n.inputs[0], tmp + "axes"}, tmp + "rs");
  set_i(rs, "keepdims", 1);
  lower_node(rs);
  NodeDef g = std_node(n, "Gemm", {n.inputs[0], n.inputs[1]}, tmp + "g");
  set_f(g, "alpha", -2.f);
  set_i(g, "transB", 1);
  lower_node(g);
  lower_node(std_node(n, "Add", {tmp + "rs", tmp + "g"}, tmp + "z"));
  lower_node(std_node(n, "Add", {tmp + "z", tmp + "c2"}, rooted ? tmp + "d2" : n.outputs[0]));
  if (rooted) lower_node(std_node(n, "Sqrt", {tmp + "d2"}, n.outputs[0]));
}
// the [rows, M] matrix of a pending distance value, for a reader that takes it as it is
void Lowerer::materialize_nearest(const std::string &name) {
  Val &v = vals.at(name);
  const std::shared_ptr<NearestPending> np = v.nn;
  Step s;
  s.kind = StepKind::Nearest;
  s.in0 = np->in_buf;
  s.nearest = np->pack;
  s.out_mode = np->rooted ? kNearestMatrixSqrt : kNearestMatrix;
  s.origin = np->origin;
  const std::vector<int64_t> shape = v.shape;
  Val b;
  b.buf = push_step(std::move(s), shape);
  b.shape = shape;
  vals[name] = b;
  buf_names[b.buf].push_back(name);
}
// the best-k lists of a pending distance value (one Nearest step per k)
int Lowerer::nearest_lists(NearestPending &np, int64_t k) {
  auto it = np.part_of_k.find(k);
  if (it != np.part_of_k.end()) return it->second;
  Step s;
  s.kind = StepKind::Nearest;
  s.in0 = np.in_buf;
  s.nearest = np.pack;
  s.M = k;
  s.out_mode = kNearestSelect;
  s.origin = np.origin;
  return np.part_of_k[k] = push_step(std::move(s), {np.rows, np.pack->slices * 2 * nearest_list_width(k)});
}
// ArgMin / TopK / Sqrt / Identity reading a pending distance value: the Nearest step serves them itself.  false: not such a reader (or a form the
// selection does not take -- the matrix is computed and the operator runs on it)
bool Lowerer::nearest_reader(const NodeDef &n) {
  if (n.inputs.empty()) return false;
  auto it = vals.find(n.inputs[0]);
  if (it == vals.end() || !it->second.nn) return false;
  const Val d = it->second;
  NearestPending &np = *d.nn;
  if (n.op == "Identity") {  // the same pending value under another name
    vals[n.outputs[0]] = d;
    return true;
  }
  if (n.op == "Sqrt") {
    if (np.rooted) return false;
    auto r = std::make_shared<NearestPending>(np);
    r->rooted = true;
    r->origin += "+" + node_label(n);
    r->part_of_k.clear();
    Val v;
    v.nn = r;
    v.shape = d.shape;
    vals[n.outputs[0]] = v;
    return true;
  }
  if (n.op == "ArgMin") {
    int64_t axis = n.attr_i("axis", 0);
    if (axis < 0) axis += 2;
    if (axis != 1 || n.attr_i("select_last_index", 0) != 0) return false;
    Step s;
    s.kind = StepKind::NearestReduce;
    s.in0 = nearest_lists(np, 1);
    s.nearest = np.pack;
    s.M = 1;
    s.out_mode = kNearestLabel;
    s.origin = np.origin + "+" + node_label(n);
    std::vector<int64_t> shape = {d.shape[0]};
    if (n.attr_i("keepdims", 1) != 0) shape.push_back(1);
    bind_output(n, 0, std::move(s), shape, true);
    return true;
  }
  // TopK
  int64_t axis = n.attr_i("axis", -1);
  if (axis < 0) axis += 2;
  const int64_t k = topk_k(n);
  if (axis != 1 || n.attr_i("largest", 1) != 0 || k < 1 || k > kNearestMaxK || k > np.pack->M) return false;
  for (size_t o = 0; o < 2; o++) {
    if (!wanted(n, o)) continue;
    Step s;
    s.kind = StepKind::NearestReduce;
    s.in0 = nearest_lists(np, k);
    s.nearest = np.pack;
    s.M = k;
    s.out_mode = o == 1 ? kNearestIndices : np.rooted ? kNearestValuesSqrt : kNearestValues;
    s.origin = np.origin + "+" + node_label(n);
    bind_output(n, o, std::move(s), {d.shape[0], k}, o == 1);
  }
  return true;
}


// ---- the k-NN vote (the block in lowerer.hpp under "distance models") ----
namespace {
bool std_op(const NodeDef *p, const char *op) { return p && p->op == op && GraphIndex::std_dom(*p); }
// the one number of a constant scalar / one-element tensor (f32 or int64)
bool const_number(const GraphIndex::Const &c, double *v) {
  if (!c.t) {
    if (!c.node) return false;
    if (auto *i = c.node->attr("value_int")) return *v = double(i->i), true;
    if (auto *f = c.node->attr("value_float")) return *v = double(f->f), true;
    return false;
  }
  if (c.t->dtype == onnx::kInt64 && c.t->i64.size() == 1) return *v = double(c.t->i64[0]), true;
  if (c.t->dtype == onnx::kFloat && c.t->f32.size() == 1) return *v = double(c.t->f32[0]), true;
  return false;
}
}  // namespace
// a reduction over axis 1 of [rows, k] (axes as a constant input or as the attribute)
bool Lowerer::vote_axis1(const NodeDef &n) const {
  std::vector<int64_t> axes;
  return graph_ints_arg(n, 1, "axes", &axes) && axes.size() == 1 && (axes[0] == 1 || axes[0] == -1);
}
// lab = [Squeeze] [Cast] [Reshape] of ArrayFeatureExtractor(T, Indices) | Gather(T, Indices, axis = 0), Indices the second output of a TopK
bool Lowerer::match_vote_lookup(const std::string &lab, VoteMatch *vm) const {
  std::string cur = lab;
  for (int hops = 0; hops < 4; hops++) {
    size_t pi = 0;
    const NodeDef *p = graph->producer(cur, &pi);
    if (!p || p->inputs.empty()) return false;
    if (std_op(p, "Squeeze") || std_op(p, "Cast") || std_op(p, "Reshape")) {
      if (p->op == "Reshape") vm->reshape = pi;
      vm->nodes.push_back(pi);
      cur = p->inputs[0];
      continue;
    }
    const bool afe = p->op == "ArrayFeatureExtractor" && p->domain == "ai.onnx.ml";
    if (!(afe || (std_op(p, "Gather") && p->attr_i("axis", 0) == 0)) || p->inputs.size() != 2) return false;
    if (!graph->constant(p->inputs[0]).t) return false;
    size_t ti = 0;
    const NodeDef *tk = graph->producer(p->inputs[1], &ti);
    if (!std_op(tk, "TopK") || tk->outputs.size() != 2 || tk->outputs[1] != p->inputs[1] || tk->inputs.empty()) return false;
    vm->table = p->inputs[0];
    vm->lookup = pi;
    vm->topk = ti;
    vm->nodes.push_back(pi);
    return true;
  }
  return false;
}
// wei = Reciprocal(mx) | Div(1, mx), mx = Max(values, eps) in either order, values = the TopK's first output or its Sqrt
bool Lowerer::match_vote_weights(const std::string &wei, VoteMatch *vm) const {
  size_t wi = 0, mi = 0;
  const NodeDef *w = graph->producer(wei, &wi);
  std::string mx;
  if (std_op(w, "Reciprocal") && w->inputs.size() == 1) mx = w->inputs[0];
  else if (std_op(w, "Div") && w->inputs.size() == 2) {
    double one = 0;
    if (!const_number(graph->constant(w->inputs[0]), &one) || one != 1.0) return false;
    mx = w->inputs[1];
  } else return false;
  const NodeDef *c = graph->producer(mx, &mi);
  if (!std_op(c, "Max") || c->inputs.size() != 2) return false;
  const NodeDef &tk = m.nodes[vm->topk];
  for (int side = 0; side < 2; side++) {
    if (!const_tensor(c->inputs[size_t(1 - side)])) continue;
    const std::string &v = c->inputs[size_t(side)];
    size_t si = 0;
    const NodeDef *sq = graph->producer(v, &si);
    if (v != tk.outputs[0] && !(std_op(sq, "Sqrt") && sq->inputs.size() == 1 && sq->inputs[0] == tk.outputs[0])) return false;
    vm->sqrt_values = v != tk.outputs[0];
    // (a Sqrt that something else reads too stays a reader of Values like any other)
    if (vm->sqrt_values && graph->sole_reader(v, false)) vm->nodes.push_back(si);
    vm->eps = c->inputs[size_t(1 - side)];
    vm->clamp = mi;
    vm->weighted = true;
    vm->nodes.push_back(mi);
    vm->nodes.push_back(wi);
    return true;
  }
  return false;
}
// all [rows, C] = the class totals: the branches, their join, the lookup behind them; *wei: the weights' name ("": uniform)
bool Lowerer::match_vote_tally(const std::string &all, VoteMatch *vm, std::string *wei) const {
  size_t ci = 0;
  const NodeDef *cat = graph->producer(all, &ci);
  int64_t unsq_axis = 1;
  if (std_op(cat, "Transpose")) {
    auto *perm = cat->attr_ints("perm");
    if (cat->inputs.size() != 1 || (perm && *perm != std::vector<int64_t>{1, 0})) return false;
    vm->nodes.push_back(ci);
    cat = graph->producer(cat->inputs[0], &ci);
    unsq_axis = 0;
  }
  if (!std_op(cat, "Concat") || cat->inputs.empty() || cat->attr_i("axis", -9) != unsq_axis) return false;
  vm->concat = ci;
  vm->nodes.push_back(ci);
  std::string lab;
  for (size_t b = 0; b < cat->inputs.size(); b++) {
    size_t ri = 0, ui = 0;
    const NodeDef *r = graph->producer(cat->inputs[b], &ri);
    bool unsq = false;
    if (std_op(r, "Unsqueeze")) {
      std::vector<int64_t> axes;
      if (!graph_ints_arg(*r, 1, "axes", &axes) || axes != std::vector<int64_t>{unsq_axis}) return false;
      ui = ri;
      unsq = true;
      vm->nodes.push_back(ui);
      r = graph->producer(r->inputs[0], &ri);
    }
    if (!std_op(r, "ReduceSum") || !vote_axis1(*r) || (r->attr_i("keepdims", 1) == 0) != unsq || (unsq_axis == 0 && !unsq)) return false;
    vm->nodes.push_back(ri);
    size_t xi = 0;
    const NodeDef *x = graph->producer(r->inputs[0], &xi);
    std::string w;
    if (std_op(x, "Mul") && x->inputs.size() == 2) {
      int cs = -1;
      for (int side = 0; side < 2 && cs < 0; side++)
        if (const NodeDef *q = graph->producer(x->inputs[size_t(side)]); std_op(q, "Cast") && !q->inputs.empty() && std_op(graph->producer(q->inputs[0]), "Equal")) cs = side;
      if (cs < 0) return false;
      w = x->inputs[size_t(1 - cs)];
      vm->nodes.push_back(xi);
      x = graph->producer(x->inputs[size_t(cs)], &xi);
    }
    if (b > 0 && w != *wei) return false;
    *wei = w;
    if (!std_op(x, "Cast") || x->attr_i("to", 0) != onnx::kFloat || x->inputs.size() != 1) return false;
    vm->nodes.push_back(xi);
    size_t ei = 0;
    const NodeDef *e = graph->producer(x->inputs[0], &ei);
    if (!std_op(e, "Equal") || e->inputs.size() != 2) return false;
    int ks = -1;
    for (int side = 0; side < 2 && ks < 0; side++)
      if (graph->constant(e->inputs[size_t(side)])) ks = side;
    if (ks < 0) return false;
    if (b > 0 && e->inputs[size_t(1 - ks)] != lab) return false;
    lab = e->inputs[size_t(1 - ks)];
    vm->nodes.push_back(ei);
    vm->equals.push_back(ei);
    vm->equal_consts.push_back(e->inputs[size_t(ks)]);
  }
  return match_vote_lookup(lab, vm) && (wei->empty() || match_vote_weights(*wei, vm));
}
void Lowerer::find_votes() {
  vote_inside.assign(m.nodes.size(), 0);
  for (size_t i = 0; i < m.nodes.size(); i++) {
    const NodeDef &a = m.nodes[i];
    if (!graph->live[i] || absorbed[i] || region[i] || !GraphIndex::std_dom(a) || a.inputs.empty() || a.outputs.empty()) continue;
    VoteMatch vm;
    vm.anchor = i;
    vm.out = a.outputs[0];
    std::string wei;
    bool ok = false;
    if (a.op == "ArgMax") {
      int64_t axis = a.attr_i("axis", 0);
      if ((axis != 1 && axis != -1) || a.attr_i("select_last_index", 0) != 0) continue;
      vm.mode = kVoteLabel;
      vm.out_col = a.attr_i("keepdims", 1) != 0;
      ok = match_vote_tally(a.inputs[0], &vm, &wei);
      // the class values: ArrayFeatureExtractor | Gather of a constant table by the index [-> Reshape / Cast]
      if (ok)
        if (const NodeDef *t = graph->sole_reader(vm.out, false); t && t->inputs.size() == 2 && t->inputs[1] == vm.out && graph->constant(t->inputs[0]).t &&
                                                                   ((t->op == "ArrayFeatureExtractor" && t->domain == "ai.onnx.ml") || (std_op(t, "Gather") && t->attr_i("axis", 0) == 0))) {
          vm.class_lookup = size_t(t - m.nodes.data());
          vm.classes = t->inputs[0];
          vm.nodes.push_back(vm.class_lookup);
          vm.out = t->outputs[0];
          vm.out_col = false;
          for (const NodeDef *q = graph->sole_reader(vm.out, false); q && (std_op(q, "Cast") || std_op(q, "Reshape")) && q->inputs[0] == vm.out; q = graph->sole_reader(vm.out, false)) {
            if (q->op == "Reshape") {
              std::vector<int64_t> shape, dims;
              if (q->inputs.size() != 2 || !graph_const_ints(q->inputs[1], &shape, &dims)) break;
              if (shape == std::vector<int64_t>{-1, 1}) vm.out_col = true;
              else if (shape == std::vector<int64_t>{-1}) vm.out_col = false;
              else break;
            }
            vm.nodes.push_back(size_t(q - m.nodes.data()));
            vm.out = q->outputs[0];
          }
        }
    } else if (a.op == "Div" && a.inputs.size() == 2) {
      size_t ri = 0;
      const NodeDef *r = graph->producer(a.inputs[1], &ri);
      if (!std_op(r, "ReduceSum") || !vote_axis1(*r)) continue;
      if (r->inputs[0] == a.inputs[0]) {  // the probabilities: all / sum(all)
        if (r->attr_i("keepdims", 1) == 0) continue;
        vm.mode = kVoteProba;
        vm.nodes.push_back(ri);
        ok = match_vote_tally(a.inputs[0], &vm, &wei);
      } else {  // the weighted mean: sum(lab * wei) / sum(wei)
        size_t ni = 0, xi = 0;
        const NodeDef *num = graph->producer(a.inputs[0], &ni);
        if (!std_op(num, "ReduceSum") || !vote_axis1(*num) || num->attr_i("keepdims", 1) != r->attr_i("keepdims", 1)) continue;
        const NodeDef *x = graph->producer(num->inputs[0], &xi);
        if (!std_op(x, "Mul") || x->inputs.size() != 2) continue;
        vm.mode = kVoteValue;
        vm.out_col = r->attr_i("keepdims", 1) != 0;
        vm.nodes = {ri, ni, xi};
        wei = r->inputs[0];
        const std::string lab = x->inputs[x->inputs[0] == wei ? 1 : 0];
        ok = (x->inputs[0] == wei || x->inputs[1] == wei) && lab != wei && match_vote_lookup(lab, &vm) && match_vote_weights(wei, &vm);
      }
    } else if (a.op == "ReduceMean") {
      if (!vote_axis1(a)) continue;
      vm.mode = kVoteValue;
      vm.out_col = a.attr_i("keepdims", 1) != 0;
      ok = match_vote_lookup(a.inputs[0], &vm);
    }
    if (!ok) continue;
    if (vm.mode == kVoteValue)  // the closing Reshape([-1, 1])
      if (const NodeDef *q = graph->sole_reader(vm.out, false); std_op(q, "Reshape") && q->inputs.size() == 2 && q->inputs[0] == vm.out) {
        std::vector<int64_t> shape, dims;
        if (graph_const_ints(q->inputs[1], &shape, &dims) && shape == std::vector<int64_t>{-1, 1}) {
          vm.nodes.push_back(size_t(q - m.nodes.data()));
          vm.out = q->outputs[0];
          vm.out_col = true;
        }
      }
    std::sort(vm.nodes.begin(), vm.nodes.end());
    vm.nodes.erase(std::unique(vm.nodes.begin(), vm.nodes.end()), vm.nodes.end());
    // no value inside has a reader outside; the end of the tail is the pattern's result and read by whatever follows
    std::set<size_t> inside(vm.nodes.begin(), vm.nodes.end());
    inside.insert(i);
    bool closed = !vote_of_topk.count(vm.topk) && graph->live[vm.topk] && !absorbed[vm.topk] && !region[vm.topk];
    {  // the TopK reads a recognised distance value (CDist, or the D2 of a find_nearest pattern), directly or through Sqrt / Identity
      std::string d = m.nodes[vm.topk].inputs[0];
      const NodeDef *p = graph->producer(d);
      for (int hops = 0; hops < 4 && (std_op(p, "Sqrt") || std_op(p, "Identity")) && p->inputs.size() == 1; hops++) p = graph->producer(d = p->inputs[0]);
      bool distance = p && p->op == "CDist" && p->domain == "com.microsoft";
      for (const auto &nm : nearest_at) distance = distance || nm.second.d2 == d;
      closed = closed && distance;
    }
    for (size_t q : vm.nodes) {
      closed = closed && graph->live[q] && !absorbed[q] && !region[q] && !vote_inside[q] && !attn_at.count(q) && !nearest_at.count(q);
      for (const std::string &o : m.nodes[q].outputs) {
        if (o == vm.out) continue;
        closed = closed && !graph->graph_outs.count(o);
        if (auto rd = graph->consumers_of.find(o); rd != graph->consumers_of.end())
          for (size_t c : rd->second) closed = closed && inside.count(c);
      }
    }
    if (vm.out != a.outputs[0]) {  // (the anchor's own result lies inside when a tail follows it)
      closed = closed && !graph->graph_outs.count(a.outputs[0]);
      for (size_t c : graph->consumers_of.at(a.outputs[0])) closed = closed && inside.count(c);
    }
    if (!closed) continue;
    for (size_t q : vm.nodes) absorbed[q] = vote_inside[q] = 1;
    vote_of_topk[vm.topk] = i;
    vote_at[i] = std::move(vm);
  }
}
// The walk is at the TopK of a vote pattern.  Its input is a pending distance value the selection serves: the vote is taken, and Values
// / Indices keep the readers outside the pattern (they get their NearestReduce steps from nearest_reader, as without the vote).
// Anything else: the nodes are given back, and every one of them lowers (or is refused) exactly as without the matcher.
void Lowerer::vote_begin(size_t anchor) {
  VoteMatch &vm = vote_at.at(anchor);
  const NodeDef &tk = m.nodes[vm.topk];
  auto it = vals.find(tk.inputs[0]);
  int64_t axis = tk.attr_i("axis", -1);
  if (axis < 0) axis += 2;
  const bool served = it != vals.end() && it->second.nn && axis == 1 && tk.attr_i("largest", 1) == 0 && !(it->second.nn->rooted && vm.sqrt_values);
  if (!served) {
    for (size_t q : vm.nodes) absorbed[q] = vote_inside[q] = 0;
    vote_of_topk.erase(vm.topk);
    vote_at.erase(anchor);
    return;
  }
  vm.np = it->second.nn;
  const int64_t k = topk_k(tk), M = vm.np->pack->M;
  if (k < 1 || k > kNearestMaxK || k > M)
    bad_form(tk, "k = " + std::to_string(k) + " neighbours of a k-NN vote is outside 1 .. " + std::to_string(std::min(kNearestMaxK, M)) + " (min(" + std::to_string(kNearestMaxK) +
                     ", M = " + std::to_string(M) + "))");
  vm.k = k;
  vm.lists = nearest_lists(*vm.np, k);
  std::set<size_t> inside(vm.nodes.begin(), vm.nodes.end());
  for (const std::string &o : tk.outputs) {
    int outside = o == m.outputs[out_index].name ? 1 : 0;
    if (auto rd = graph->consumers_of.find(o); rd != graph->consumers_of.end())
      for (size_t c : rd->second) outside += !inside.count(c);
    uses[o] = outside;
  }
}
// the anchor of a vote that vote_begin took: the load-time checks (each names its node) and the NearestVote step
void Lowerer::lower_vote(const VoteMatch &vm) {
  const NearestPending &np = *vm.np;
  const int64_t M = np.pack->M, k = vm.k;
  const bool cls = vm.mode != kVoteValue;
  auto pack = std::make_shared<VotePack>();
  pack->weighted = vm.weighted;
  pack->rooted = np.rooted || vm.sqrt_values;
  const NodeDef &lk = m.nodes[vm.lookup];
  const std::shared_ptr<TensorData> T = graph->constant(vm.table).t;
  if (T->dims.size() > 2 || (T->dims.size() == 2 && T->dims[1] != 1))
    bad_form(lk, "its table " + shape_str(T->dims) + " holds several targets per reference vector: multi-output neighbours models are not supported (one [M] column only)");
  if (T->dtype != onnx::kInt64 && T->dtype != onnx::kFloat) bad_form(lk, "its table must hold int64 or f32 values");
  if (cls && T->dtype != onnx::kInt64) bad_form(lk, "the table of a k-NN classifier must hold int64 class indices");
  const int64_t n = int64_t(T->dtype == onnx::kInt64 ? T->i64.size() : T->f32.size());
  if (n != M) bad_form(lk, "its table holds " + std::to_string(n) + " entries for the M = " + std::to_string(M) + " reference vectors of the search");
  if (vm.reshape != SIZE_MAX) {
    const NodeDef &rs = m.nodes[vm.reshape];
    std::vector<int64_t> shape, dims;
    const bool known = rs.inputs.size() == 2 && graph_const_ints(rs.inputs[1], &shape, &dims);
    if (!known || !((shape.size() == 2 && shape[1] == k) || (shape.size() == 3 && shape[1] == k && shape[2] == 1)))
      bad_form(rs, "the looked-up neighbours must be reshaped to [rows, k = " + std::to_string(k) + "] or [rows, k, 1]" + (known ? ", got " + shape_str(shape) : std::string()));
  }
  if (vm.weighted) {
    const std::shared_ptr<TensorData> e = const_tensor(vm.eps);
    const float eps = e && e->f32.size() == 1 ? e->f32[0] : 0.f;
    if (!(eps > 0.f) || !std::isfinite(eps))
      bad_form(m.nodes[vm.clamp], "the bound of the distance weights must be one positive finite constant (w = 1 / max(d, eps))" + (e && e->f32.size() == 1 ? ", got " + std::to_string(eps) : std::string()));
    pack->eps = eps;
  }
  int64_t C = 0;
  if (cls) {
    C = int64_t(vm.equals.size());
    const NodeDef &cat = m.nodes[vm.concat];
    if (C < 2) bad_form(cat, "C = " + std::to_string(C) + " class: a vote needs at least 2");
    if (vm.mode == kVoteProba && C > kVoteMaxProbaClasses)
      bad_form(cat, "C = " + std::to_string(C) + " classes is above the cap of " + std::to_string(kVoteMaxProbaClasses) + " for the probabilities of a k-NN vote (the label has no cap)");
    for (int64_t c = 0; c < C; c++) {
      double v = -1;
      if (!const_number(graph->constant(vm.equal_consts[size_t(c)]), &v) || v != double(c))
        bad_form(m.nodes[vm.equals[size_t(c)]], "the class branches must compare with 0 .. " + std::to_string(C - 1) + " in Concat order; branch " + std::to_string(c) + " compares with " +
                                                    (v == std::floor(v) ? std::to_string(int64_t(v)) : std::to_string(v)));
    }
    pack->cls.resize(size_t(M));
    for (int64_t j = 0; j < M; j++) {
      const int64_t v = T->i64[size_t(j)];
      if (v < 0 || v >= C) bad_form(lk, "class index " + std::to_string(v) + " of reference vector " + std::to_string(j) + " is outside 0 .. " + std::to_string(C - 1));
      pack->cls[size_t(j)] = int32_t(v);
    }
    pack->class_value.resize(size_t(C));
    for (int64_t c = 0; c < C; c++) pack->class_value[size_t(c)] = float(c);
    if (vm.class_lookup != SIZE_MAX) {
      const NodeDef &cl = m.nodes[vm.class_lookup];
      const std::shared_ptr<TensorData> V = graph->constant(vm.classes).t;
      if (V->dims.size() != 1 || (V->dtype != onnx::kInt64 && V->dtype != onnx::kFloat)) bad_form(cl, "only a 1-D int64 or f32 class table");
      const int64_t nv = int64_t(V->dtype == onnx::kInt64 ? V->i64.size() : V->f32.size());
      if (nv != C) bad_form(cl, "its class table holds " + std::to_string(nv) + " values for C = " + std::to_string(C) + " classes");
      for (int64_t c = 0; c < C; c++) {
        const double v = V->dtype == onnx::kInt64 ? double(V->i64[size_t(c)]) : double(V->f32[size_t(c)]);
        if (!(std::fabs(v) <= double(kVoteMaxClassValue)))
          bad_form(cl, "class value " + (V->dtype == onnx::kInt64 ? std::to_string(V->i64[size_t(c)]) : std::to_string(v)) + " is beyond 2^24: labels are served as f32 values");
        pack->class_value[size_t(c)] = float(v);
      }
    }
  } else {
    pack->target.resize(size_t(M));
    for (int64_t j = 0; j < M; j++) pack->target[size_t(j)] = T->dtype == onnx::kInt64 ? float(T->i64[size_t(j)]) : T->f32[size_t(j)];
  }
  pack->classes = C;
  Step s;
  s.kind = StepKind::NearestVote;
  s.in0 = vm.lists;
  s.nearest = np.pack;
  s.vote = pack;
  s.M = k;
  s.out_mode = vm.mode;
  s.origin = np.origin + "+" + node_label(m.nodes[vm.topk]) + "+...+" + node_label(m.nodes[vm.anchor]);
  std::vector<int64_t> shape = {np.rows};
  if (vm.mode == kVoteProba) shape.push_back(C);
  else if (vm.out_col) shape.push_back(1);
  Val v;
  v.buf = push_step(std::move(s), shape);
  v.shape = shape;
  vals[vm.out] = v;
  buf_names[v.buf].push_back(vm.out);
  if (vm.mode == kVoteLabel) int_bufs.insert(v.buf);
}

}  // namespace lowering

}  // namespace infera_hip
