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

}  // namespace lowering

}  // namespace infera_hip
