// lower_rotary.cpp -- struct Lowerer (lowerer.hpp): rotary position embeddings.  The opset-23 operator RotaryEmbedding of the standard domain and
// the rotate_half spelling x * cos + cat(-x2, x1) * sin that exporters write by hand both become ONE Rotary step (hip/rotary.hip) with two
// f32 factor tables A, B [T, rd]:  y[j] = fl(fl(x[j] * A[t, j]) + fl(x[partner(j)] * B[t, j])).  A is cos over both members of a pair, B is -sin
// on the first member and +sin on the second, which is the specification's real = c a - s b, imag = s a + c b bit for bit.
// match_rotary recognises either on a head-major value for the two attention front ends (find_attention_ops, find_attention); lower_attention
// emits the steps.  Which forms are served and which are refused: INTEGRATION.md section 2.6 ("Rotary position embeddings").

#include <climits>

#include "lowerer.hpp"

namespace infera_hip {

namespace lowering {

std::shared_ptr<const Lowerer::RotaryMatch> Lowerer::match_rotary(const std::string &v) const {
  size_t vi = 0;
  const NodeDef *p = graph->producer(v, &vi);
  if (!p || !graph->std_dom(*p)) return nullptr;
  auto rm = std::make_shared<RotaryMatch>();
  rm->at = p;
  rm->nodes.push_back(vi);
  if (p->op == "RotaryEmbedding") {
    if (p->inputs.size() < 3 || p->inputs[0].empty()) return nullptr;
    rm->x = p->inputs[0];
    rm->cos = p->inputs[1];
    rm->sin = p->inputs[2];
    if (p->inputs.size() > 3) rm->pos = p->inputs[3];
    return rm;
  }
  // Add(Mul(x, cos), Mul(rh, sin)), operand order free in Add and Mul
  if (p->op != "Add" || p->inputs.size() != 2) return nullptr;
  struct Term {
    std::string act, cst;
    size_t idx = 0;
  } term[2];
  for (int i = 0; i < 2; i++) {
    const NodeDef *mul = graph->producer(p->inputs[size_t(i)], &term[i].idx);
    if (!mul || mul->op != "Mul" || !graph->std_dom(*mul) || mul->inputs.size() != 2 || graph->sole_reader(p->inputs[size_t(i)], false) != p) return nullptr;
    const bool c0 = !graph->row_data.count(mul->inputs[0]), c1 = !graph->row_data.count(mul->inputs[1]);
    if (c0 == c1) return nullptr;
    term[i].act = mul->inputs[c0 ? 1 : 0];
    term[i].cst = mul->inputs[c0 ? 0 : 1];
    if (!const_tensor(term[i].cst)) return nullptr;
    rm->nodes.push_back(term[i].idx);
  }
  // which term reads rh = Concat(Neg(x2), x1)
  auto is_rh = [&](const std::string &a) {
    const NodeDef *c = graph->producer(a);
    return c && c->op == "Concat" && graph->std_dom(*c);
  };
  const int r = is_rh(term[1].act) ? 1 : is_rh(term[0].act) ? 0 : -1;
  if (r < 0 || is_rh(term[1 - r].act)) return nullptr;
  rm->spelling = true;
  rm->x = term[1 - r].act;
  rm->cos = term[1 - r].cst;
  rm->sin = term[r].cst;
  const int64_t d = const_tensor(rm->cos)->dims.empty() ? 0 : const_tensor(rm->cos)->dims.back();
  if (d < 2 || d % 2 != 0) return nullptr;
  size_t ci = 0, ni = 0;
  const NodeDef *cat = graph->producer(term[r].act, &ci);
  const int64_t cat_axis = cat->attr_i("axis", 0);
  if (cat->inputs.size() != 2 || (cat_axis != -1 && cat_axis != 3) || graph->sole_reader(term[r].act, false) != &m.nodes[term[r].idx]) return nullptr;
  const NodeDef *neg = graph->producer(cat->inputs[0], &ni);
  if (!neg || neg->op != "Neg" || !graph->std_dom(*neg) || neg->inputs.size() != 1 || graph->sole_reader(cat->inputs[0], false) != cat) return nullptr;
  const std::string &x2 = neg->inputs[0], &x1 = cat->inputs[1];
  if (graph->sole_reader(x2, false) != neg || graph->sole_reader(x1, false) != cat) return nullptr;
  rm->nodes.push_back(ci);
  rm->nodes.push_back(ni);
  size_t i1 = 0, i2 = 0;
  const NodeDef *h1 = graph->producer(x1, &i1), *h2 = graph->producer(x2, &i2);
  if (!h1 || !h2 || !graph->std_dom(*h1) || !graph->std_dom(*h2) || h1->inputs.empty() || h2->inputs.empty() || h1->inputs[0] != rm->x || h2->inputs[0] != rm->x) return nullptr;
  if (h1 == h2 && h1->op == "Split") {  // one Split into two equal halves: x1 first
    const int64_t axis = h1->attr_i("axis", 0);
    std::vector<int64_t> sizes;
    if (h1->outputs.size() != 2 || h1->outputs[0] != x1 || h1->outputs[1] != x2 || (axis != -1 && axis != 3) || !graph_ints_arg(*h1, 1, "split", &sizes)) return nullptr;
    if (!sizes.empty() && sizes != std::vector<int64_t>{d / 2, d / 2}) return nullptr;
    rm->nodes.push_back(i1);
  } else if (h1 != h2 && h1->op == "Slice" && h2->op == "Slice") {  // the Slices [0, d/2) and [d/2, d) of the last axis
    auto bounds = [&](const NodeDef &s, int64_t b, int64_t e, bool open_end) {
      std::vector<int64_t> st, en, ax, sp;
      if (s.inputs.size() < 4 || !graph_ints_arg(s, 1, "starts", &st) || !graph_ints_arg(s, 2, "ends", &en) || !graph_ints_arg(s, 3, "axes", &ax) ||
          !graph_ints_arg(s, 4, "steps", &sp))
        return false;
      return st == std::vector<int64_t>{b} && (en == std::vector<int64_t>{e} || (open_end && en == std::vector<int64_t>{INT64_MAX})) &&
             (ax == std::vector<int64_t>{-1} || ax == std::vector<int64_t>{3}) && (sp.empty() || sp == std::vector<int64_t>{1});
    };
    if (!bounds(*h1, 0, d / 2, false) || !bounds(*h2, d / 2, d, true)) return nullptr;
    rm->nodes.push_back(i1);
    rm->nodes.push_back(i2);
  } else {
    return nullptr;
  }
  return rm;
}

std::string Lowerer::behind_rotary(const std::string &v, std::shared_ptr<const RotaryMatch> *rot) const {
  const std::shared_ptr<const RotaryMatch> rm = match_rotary(v);
  if (!rm) return v;
  const NodeDef *t = graph->producer(rm->x);
  const std::vector<int64_t> *perm = t && t->op == "Transpose" && graph->std_dom(*t) ? t->attr_ints("perm") : nullptr;
  const NodeDef *r = perm && *perm == std::vector<int64_t>{0, 2, 1, 3} ? graph->producer(t->inputs[0]) : nullptr;
  if (!r || r->op != "Reshape" || r->inputs.size() != 2 || !rotary_reads_alone(*rm)) {
    // the spelling: not absorbed, the front end goes on as without it.  The operator beside num_heads may be the 3-D form: left to the walk
    if (rm->spelling || rm->at->attr_i("num_heads", 0) > 0) return v;
    unsupported(*rm->at, "unsupported operator form: its 4-D X is not the head split Reshape [N,T,h,dh] -> Transpose(0,2,1,3) of a rows-first value, read by this node alone "
                         "(a head-major [N,h,T,dh] tensor such as a graph input is not supported)");
  }
  *rot = rm;
  return rm->x;
}

bool Lowerer::rotary_reads_alone(const RotaryMatch &rm) const {
  auto it = graph->consumers_of.find(rm.x);
  if (it == graph->consumers_of.end() || graph->graph_outs.count(rm.x)) return false;
  // the operator reads x once; the spelling: Mul, and the two Slices or the one Split
  const size_t want = !rm.spelling ? 1 : m.nodes[rm.nodes.back()].op == "Split" ? 2 : 3;
  if (it->second.size() != want) return false;
  for (size_t c : it->second)
    if (std::find(rm.nodes.begin(), rm.nodes.end(), c) == rm.nodes.end()) return false;
  return true;
}

Step Lowerer::rotary_step(const RotaryMatch &rm, int64_t T, int64_t h, int64_t dh) {
  const NodeDef &n = *rm.at;
  if (cur_half) bad_form(n, "a float16 graph: rotary position embeddings are served in float32 only");
  if (T < 1 || T > kAttnMaxT) bad_form(n, "T = " + std::to_string(T) + " is beyond the Rotary kernel's cap of " + std::to_string(kAttnMaxT) + " steps");
  if (dh > kAttnMaxDh) bad_form(n, "dh = " + std::to_string(dh) + " is beyond the Rotary kernel's cap of " + std::to_string(kAttnMaxDh) + " columns per head");
  if (h > kAttnMaxHeads) bad_form(n, "h = " + std::to_string(h) + " is beyond the Rotary kernel's cap of " + std::to_string(kAttnMaxHeads) + " heads");
  auto table = [&](const std::string &name, const char *what) {
    if (graph->row_data.count(name)) bad_form(n, std::string(what) + " '" + name + "' is not a constant (Cos / Sin computed in the graph are not supported; fold the tables)");
    const Val *c = find_value(name);
    if (!c || !c->is_const) bad_form(n, std::string(what) + " '" + name + "' is not a constant");
    if (c->c->dtype != onnx::kFloat || c->c->elem == onnx::kFloat16) bad_form(n, std::string(what) + " must be an f32 constant (a float16 graph is not supported)");
    return c->c;
  };
  Step s;
  s.kind = StepKind::Rotary;
  s.attn_T = T, s.attn_heads = h, s.attn_dh = dh;
  if (rm.spelling) {  // whole factor tables: A = cos, B = -sin | +sin by half
    const auto cs = table(rm.cos, "the cos table"), sn = table(rm.sin, "the sin table");
    for (const auto &t : {cs, sn}) {
      std::vector<int64_t> d = t->dims;
      while (d.size() > 2 && d[0] == 1) d.erase(d.begin());
      if (d != std::vector<int64_t>{T, dh})
        bad_form(n, "the rotate_half tables must be [T, dh] = [" + std::to_string(T) + "," + std::to_string(dh) + "] (or [1,T,dh], [1,1,T,dh]), got " + shape_str(t->dims));
    }
    if (dh % 2 != 0) bad_form(n, "dh = " + std::to_string(dh) + " is odd");
    s.rot_rd = dh;
    s.scale = cs->f32;
    s.shift = sn->f32;
    for (int64_t t = 0; t < T; t++)
      for (int64_t j = 0; j < dh / 2; j++) s.shift[size_t(t * dh + j)] = -s.shift[size_t(t * dh + j)];
    return s;
  }
  if (m.opset < 23) bad_form(n, "RotaryEmbedding belongs to the standard domain from opset 23 on; the model declares opset " + std::to_string(m.opset));
  if (const int64_t nh = n.attr_i("num_heads", 0); nh > 0 && nh != h)
    bad_form(n, "num_heads = " + std::to_string(nh) + " disagrees with the " + std::to_string(h) + " heads of the head split in front of it");
  const int64_t inter = n.attr_i("interleaved", 0);
  if (inter != 0 && inter != 1) bad_form(n, "interleaved = " + std::to_string(inter) + "; only 0 or 1");
  const int64_t rd_attr = n.attr_i("rotary_embedding_dim", 0), rd = rd_attr == 0 ? dh : rd_attr;
  if (rd < 2 || rd % 2 != 0 || rd > dh)
    bad_form(n, "rotary_embedding_dim = " + std::to_string(rd) + " must be even and at most the head size " + std::to_string(dh) + " (an odd or wider rotated width has no pairs)");
  const auto cs = table(rm.cos, "cos_cache"), sn = table(rm.sin, "sin_cache");
  std::vector<int64_t> pos;  // the cache row of each step
  int64_t P = 0;
  if (!rm.pos.empty()) {
    if (graph->row_data.count(rm.pos)) bad_form(n, "position_ids '" + rm.pos + "' depend on the row (they are computed from a graph input); per-row positions are not supported yet");
    const Val *pv = find_value(rm.pos);
    if (!pv || !pv->is_const || pv->c->dtype != onnx::kInt64) bad_form(n, "position_ids '" + rm.pos + "' must be a constant int64 tensor");
    if (pv->shape != std::vector<int64_t>{1, T} && pv->shape != std::vector<int64_t>{T})
      bad_form(n, "position_ids must be [1, T] or [T] with T = " + std::to_string(T) + ", got " + shape_str(pv->shape) + " (per-row positions are not supported yet)");
    pos = pv->c->i64;
    for (const auto &t : {cs, sn})
      if (t->dims.size() != 2) bad_form(n, "with position_ids the caches must be [P, rd/2], got " + shape_str(t->dims));
    P = cs->dims[0];
    s.rot_const_pos = true;
  } else {
    for (const auto &t : {cs, sn}) {
      if (t->dims.size() != 3) bad_form(n, "without position_ids the caches must be [1, T, rd/2], got " + shape_str(t->dims));
      if (t->dims[0] != 1)
        bad_form(n, "the caches have a leading extent of " + std::to_string(t->dims[0]) + "; the row count is symbolic, so only [1, T, rd/2] (one table for every row) is served");
      if (t->dims[1] != T) bad_form(n, "the caches hold " + std::to_string(t->dims[1]) + " steps, the window T = " + std::to_string(T));
    }
    P = T;
    for (int64_t t = 0; t < T; t++) pos.push_back(t);
  }
  for (const auto &t : {cs, sn})
    if (t->dims.back() != rd / 2 || (s.rot_const_pos && t->dims[0] != P))
      bad_form(n, "the caches must be " + std::string(s.rot_const_pos ? "[P, " : "[1, T, ") + std::to_string(rd / 2) + "] (rd/2 columns, equal shapes), got " + shape_str(t->dims));
  for (int64_t t = 0; t < T; t++)
    if (pos[size_t(t)] < 0 || pos[size_t(t)] >= P)
      bad_form(n, "position " + std::to_string(pos[size_t(t)]) + " (step " + std::to_string(t) + ") lies outside the caches' [0, " + std::to_string(P) + ")");
  s.rot_rd = rd;
  s.rot_interleaved = inter == 1;
  s.scale.resize(size_t(T * rd));
  s.shift.resize(size_t(T * rd));
  const int64_t half = rd / 2;
  for (int64_t t = 0; t < T; t++)
    for (int64_t i = 0; i < half; i++) {
      const float c = cs->f32[size_t(pos[size_t(t)] * half + i)], sv = sn->f32[size_t(pos[size_t(t)] * half + i)];
      const int64_t a = inter ? 2 * i : i, b = inter ? 2 * i + 1 : i + half;  // the pair's first and second member
      s.scale[size_t(t * rd + a)] = s.scale[size_t(t * rd + b)] = c;
      s.shift[size_t(t * rd + a)] = -sv;
      s.shift[size_t(t * rd + b)] = sv;
    }
  return s;
}

// A head-major RotaryEmbedding that no attention front end absorbed is refused before the walk, which would stop at the Transpose in front of
// it: the refusal names the operator and says which half of the served form is missing
void Lowerer::check_rotary_ops() {
  for (size_t ni = 0; ni < m.nodes.size(); ni++) {
    const NodeDef &n = m.nodes[ni];
    if (!graph->live[ni] || absorbed[ni] || n.op != "RotaryEmbedding" || !graph->std_dom(n) || n.inputs.empty()) continue;
    const NodeDef *t = graph->producer(n.inputs[0]);
    const std::vector<int64_t> *perm = t && t->op == "Transpose" ? t->attr_ints("perm") : nullptr;
    if (perm && perm->size() == 4) {
      const NodeDef *r = *perm == std::vector<int64_t>{0, 2, 1, 3} ? graph->producer(t->inputs[0]) : nullptr;
      if (r && r->op == "Reshape" && graph->sole_reader(n.inputs[0], false) == &n)
        bad_form(n, "its 4-D result is read by something other than an attention operand (Q, K or V of Attention, or of the MatMul / Softmax pattern)");
      bad_form(n, "its 4-D X is not the head split Reshape [N,T,h,dh] -> Transpose(0,2,1,3) of a rows-first value, read by this node alone");
    }
    for (const auto &in : m.inputs)
      if (in.name == n.inputs[0] && in.dims.size() == 4)
        bad_form(n, "its 4-D X is not the head split Reshape [N,T,h,dh] -> Transpose(0,2,1,3) of a rows-first value (a head-major graph input is not supported)");
  }
}

void Lowerer::rotary_embedding(const NodeDef &n) {
  if (n.inputs.size() < 3) bad_form(n, "X, cos_cache and sin_cache are required");
  const Val a = get(n, 0);
  if (a.is_const) bad_form(n, "X is a constant; only activations");
  if (a.shape.size() == 4) bad_form(n, "its 4-D X is not the head split Reshape [N,T,h,dh] -> Transpose(0,2,1,3) of a rows-first value");
  if (a.shape.size() != 3 || a.ra != 0 || a.padded()) bad_form(n, "X must be a rows-first [N, T, h*dh] window, got " + shape_str(a.shape) + (a.ra ? " (time-major)" : ""));
  const int64_t T = a.shape[1], E = a.shape[2], h = n.attr_i("num_heads", 0);
  if (h < 1) bad_form(n, "a 3-D X needs num_heads");
  if (E % h != 0) bad_form(n, "E = " + std::to_string(E) + " is not divisible by num_heads = " + std::to_string(h));
  RotaryMatch rm;
  rm.at = &n;
  rm.cos = n.inputs[1];
  rm.sin = n.inputs[2];
  if (n.inputs.size() > 3) rm.pos = n.inputs[3];
  Step s = rotary_step(rm, T, h, E / h);
  s.in0 = a.buf;
  s.attn_ld[0] = E;
  emit_window(std::move(s), n, a.shape);
}

}  // namespace lowering

}  // namespace infera_hip
