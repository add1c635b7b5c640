// lower_embed.cpp -- struct Lowerer (lowerer.hpp): embedding lookups.
// The state, the match structs and the block that explains them stand in lowerer.hpp under "embedding lookups";
// which graphs are served and which are refused: INTEGRATION.md section 2.6 ("Embedding lookups").

#include "embed.hpp"
#include "lowerer.hpp"

namespace infera_hip {

namespace lowering {

// an integer constant known before the walk: an initializer or a Constant node
bool Lowerer::graph_const_ints(const std::string &name, std::vector<int64_t> *v, std::vector<int64_t> *dims) const {
  const GraphIndex::Const c = graph->constant(name);
  const TensorData *t = c.t.get();
  if (!t) {
    if (!c.node) return false;
    if (auto *i = c.node->attr("value_int")) { *v = {i->i}; dims->clear(); return true; }
    else if (auto *is = c.node->attr_ints("value_ints")) { *v = *is; *dims = {int64_t(is->size())}; return true; }
    else return false;
  }
  if (t->dtype != onnx::kInt64) return false;
  *v = t->i64;
  *dims = t->dims;
  return true;
}
// the integer list input `i` (or, in older opsets, attribute `attr`) of n; false: not constant
bool Lowerer::graph_ints_arg(const NodeDef &n, size_t i, const char *attr, std::vector<int64_t> *v) const {
  v->clear();
  std::vector<int64_t> dims;
  if (has_input(n, i)) return graph_const_ints(n.inputs[i], v, &dims);
  if (auto *p = n.attr_ints(attr)) *v = *p;
  return true;
}
// `v` as columns of the input buffer; "" or why it is none
std::string Lowerer::embed_cols(const std::string &v, EmbedCols *c, int depth) const {
  int64_t off = 0;
  for (const auto &in : m.inputs) {
    const int64_t w = m.inputs.size() == 1 ? (in.dims.size() == 2 ? in.dims[1] : 0) : input_cols(in);
    if (in.name == v) {
      const bool one_col = m.inputs.size() > 1 && in.dims.size() == 1;  // (a rank-1 integer input: run())
      if (in.dims.size() != 2 && !one_col) return "indices of rank " + std::to_string(in.dims.size()) + " (graph input '" + v + "'); only [N] and [N, k]";
      c->src0 = off, c->k = w, c->rank2 = !one_col;
      c->int_input = in.elem_type == onnx::kInt64 || in.elem_type == onnx::kInt32;
      return "";
    }
    off += w;
  }
  auto pi = graph->producer_of.find(v);
  if (pi == graph->producer_of.end()) return "indices that are not computed from a graph input";
  const NodeDef &p = m.nodes[pi->second];
  const std::string by = "indices computed by " + p.op + (p.name.empty() ? "" : " '" + p.name + "'") +
                         "; only columns of a graph input, picked by Gather(axis = 1) / Slice / Squeeze, Cast to an integer type, plus a constant integer offset";
  if (depth > 64 || (!p.domain.empty() && p.domain != "ai.onnx") || p.inputs.empty()) return by;
  auto narrow = [&](int64_t b, int64_t n) {
    c->src0 += b;
    if (!c->off.empty()) c->off = std::vector<int64_t>(c->off.begin() + b, c->off.begin() + b + n);
    c->k = n;
  };
  std::string why;
  if (p.op == "Cast" || p.op == "Identity") {
    const int64_t to = p.attr_i("to", onnx::kFloat);
    const bool to_int = p.op == "Cast" && (to == onnx::kInt64 || to == onnx::kInt32);
    if (p.op == "Cast" && !to_int && to != onnx::kFloat && to != onnx::kDouble) return by;
    if (!(why = embed_cols(p.inputs[0], c, depth + 1)).empty()) return why;
    c->truncated = c->truncated || to_int;
  } else if (p.op == "Flatten") {  // [N, k] stays [N, k]
    const int64_t axis = p.attr_i("axis", 1);
    if (!(why = embed_cols(p.inputs[0], c, depth + 1)).empty()) return why;
    if (!c->rank2 || (axis != 1 && axis != -1)) return by;
  } else if (p.op == "Gather") {
    std::vector<int64_t> iv, idims;
    if (p.inputs.size() != 2 || !graph_const_ints(p.inputs[1], &iv, &idims) || idims.size() > 1 || iv.empty()) return by;
    if (!(why = embed_cols(p.inputs[0], c, depth + 1)).empty()) return why;
    int64_t axis = p.attr_i("axis", 0);
    if (!c->rank2 || (axis != 1 && axis != -1)) return by;
    for (auto &i : iv)
      if (i < 0) i += c->k;
    for (size_t i = 1; i < iv.size(); i++)
      if (iv[i] != iv[0] + int64_t(i)) return "index columns picked out of order; only a contiguous column range";
    if (iv[0] < 0 || iv[0] + int64_t(iv.size()) > c->k) return "an index column out of range";
    narrow(iv[0], int64_t(iv.size()));
    if (idims.empty()) c->rank2 = false;
  } else if (p.op == "Slice") {
    std::vector<int64_t> st, en, ax, sp;
    if (!graph_ints_arg(p, 1, "starts", &st) || !graph_ints_arg(p, 2, "ends", &en) || !graph_ints_arg(p, 3, "axes", &ax) || !graph_ints_arg(p, 4, "steps", &sp)) return by;
    if (!(why = embed_cols(p.inputs[0], c, depth + 1)).empty()) return why;
    if (!c->rank2 || st.size() != 1 || en.size() != 1 || ax.size() != 1 || (ax[0] != 1 && ax[0] != -1) || (!sp.empty() && sp[0] != 1)) return by;
    int64_t b = st[0] < 0 ? st[0] + c->k : st[0], e = en[0] < 0 ? en[0] + c->k : en[0];
    b = std::clamp<int64_t>(b, 0, c->k);
    e = std::clamp<int64_t>(e, b, c->k);
    if (e == b) return "an empty column range";
    narrow(b, e - b);
  } else if (p.op == "Squeeze" || p.op == "Unsqueeze") {
    std::vector<int64_t> ax;
    if (!graph_ints_arg(p, 1, "axes", &ax)) return by;
    if (!(why = embed_cols(p.inputs[0], c, depth + 1)).empty()) return why;
    const bool sq = p.op == "Squeeze";
    if (c->rank2 != sq || c->k != 1 || ax.size() > 1 || (ax.empty() && !sq) || (!ax.empty() && ax[0] != 1 && ax[0] != -1)) return by;
    c->rank2 = !sq;
  } else if (p.op == "Add") {
    std::vector<int64_t> ov, odims;
    if (p.inputs.size() != 2) return by;
    const bool left = graph_const_ints(p.inputs[0], &ov, &odims);
    if (!left && !graph_const_ints(p.inputs[1], &ov, &odims)) return by;
    if (!(why = embed_cols(p.inputs[left ? 1 : 0], c, depth + 1)).empty()) return why;
    const bool shape_ok = odims.empty() || odims.size() == 1 || (odims.size() == 2 && odims[0] == 1);
    if (!shape_ok || ov.empty() || (ov.size() != 1 && (!c->rank2 || int64_t(ov.size()) != c->k)))
      return "an offset tensor " + shape_str(odims) + " added to " + std::to_string(c->k) + " index column" + (c->k == 1 ? "" : "s") + "; only a scalar, [k] or [1, k]";
    if (c->off.empty()) c->off.assign(size_t(c->k), 0);
    for (int64_t j = 0; j < c->k; j++) {
      int64_t &o = c->off[size_t(j)];
      if (__builtin_add_overflow(o, ov[ov.size() == 1 ? 0 : size_t(j)], &o) || o > kEmbedMaxV || o < -kEmbedMaxV)
        return "an index offset beyond 2^24 (indices arrive as f32 values)";
    }
  } else {
    return by;
  }
  c->chain.push_back(pi->second);
  return "";
}

void Lowerer::find_embeds() {
  const size_t N = m.nodes.size();
  std::vector<EmbedLookup> found;
  for (size_t i = 0; i < N; i++) {
    const NodeDef &n = m.nodes[i];
    if (!graph->live[i] || absorbed[i] || n.op != "Gather" || !graph->std_dom(n) || n.inputs.size() != 2 || n.outputs.empty() || !graph->row_data.count(n.inputs[1])) continue;
    const std::shared_ptr<TensorData> t = graph->constant(n.inputs[0]).t;
    if (!t) continue;  // (data that is no plain constant: Lowerer::gather says what it serves)
    // from here on the node is an embedding lookup, served or refused in its own words
    static const std::map<int, const char *> type_names = {{onnx::kFloat16, "float16"}, {onnx::kDouble, "float64"}, {onnx::kInt64, "int64"}, {onnx::kInt32, "int32"},
                                                           {onnx::kInt8, "int8"}, {onnx::kUint8, "uint8"}};
    const int elem = t->elem ? t->elem : t->dtype;
    if (t->dtype != onnx::kFloat || elem != onnx::kFloat || t->q_data)
      bad_form(n, std::string("a table of type ") + (type_names.count(elem) ? type_names.at(elem) : "other than f32") +
                      "; only f32 tables are looked up (float16, integer and quantised tables are not)");
    if (const std::string why = embed_table_refusal(t->dims); !why.empty()) bad_form(n, why);
    int64_t axis = n.attr_i("axis", 0);
    if (axis < 0) axis += int64_t(t->dims.size());
    if (axis != 0) bad_form(n, "axis = " + std::to_string(n.attr_i("axis", 0)) + " of a constant table; a lookup takes whole rows (axis = 0)");
    EmbedLookup L;
    L.gather = i;
    L.table = t;
    L.V = t->dims[0];
    L.d = t->dims.size() == 2 ? t->dims[1] : 1;
    if (t->f32.size() != size_t(L.V) * size_t(L.d)) bad_form(n, "a table whose data disagrees with its dims " + shape_str(t->dims));
    if (plan.input_declared_type == "float16") bad_form(n, "indices taken from a float16 graph input");
    if (const std::string why = embed_cols(n.inputs[1], &L.ix); !why.empty()) bad_form(n, why);
    L.out = n.outputs[0];
    L.shape = {plan.input_shape[0]};
    if (L.ix.rank2) L.shape.push_back(L.ix.k);
    if (t->dims.size() == 2) L.shape.push_back(L.d);
    // [N, k, d] -> [N, k * d] by the Flatten / Reshape that alone reads it
    if (L.shape.size() == 3)
      if (const NodeDef *r = only_reader(L.out); r && graph->std_dom(*r) && !r->outputs.empty() && r->inputs[0] == L.out) {
        bool flat = r->op == "Flatten" && r->attr_i("axis", 1) == 1;
        std::vector<int64_t> tgt, tdims;
        if (r->op == "Reshape" && r->inputs.size() == 2 && graph_const_ints(r->inputs[1], &tgt, &tdims) && tgt.size() == 2)
          flat = (tgt[0] == 0 || tgt[0] == -1 || (tgt[0] > 0 && tgt[0] == L.shape[0])) && (tgt[1] == L.ix.k * L.d || (tgt[1] == -1 && tgt[0] != -1));
        if (flat) {
          L.tail.push_back(size_t(r - m.nodes.data()));
          L.out = r->outputs[0];
          L.shape = {L.shape[0], L.ix.k * L.d};
        }
      }
    // [N] (a rank-1 table by one index column) -> [N, 1] by the Unsqueeze(axis 1) that alone reads it: what a Concat wants
    if (L.shape.size() == 1)
      if (const NodeDef *r = only_reader(L.out); r && graph->std_dom(*r) && r->op == "Unsqueeze" && !r->outputs.empty() && r->inputs[0] == L.out) {
        std::vector<int64_t> ax;
        if (graph_ints_arg(*r, 1, "axes", &ax) && ax.size() == 1 && (ax[0] == 1 || ax[0] == -1)) {
          L.tail.push_back(size_t(r - m.nodes.data()));
          L.out = r->outputs[0];
          L.shape = {L.shape[0], 1};
        }
      }
    found.push_back(std::move(L));
  }
  if (found.empty()) return;
  // A feature-axis Concat that reads lookups is one step: its lookups and the numeric columns of a graph input among its inputs are pieces,
  // and an input that another step computes (a Scaler on the numeric columns, a Relu of a lookup) is a gap that one CopyCols behind the
  // step fills.  A lookup is looked up again by every such Concat that reads it -- that costs nothing -- and is a step of its own only
  // where something else reads it too.
  const std::set<std::string> &graph_outs = graph->graph_outs;
  std::set<size_t> concats;
  for (size_t li = 0; li < found.size(); li++) {
    if (found[li].shape.size() != 2) continue;
    auto it = graph->consumers_of.find(found[li].out);
    if (it == graph->consumers_of.end()) continue;
    for (size_t c : it->second) {
      const NodeDef &r = m.nodes[c];
      if (r.op == "Concat" && graph->std_dom(r) && !r.outputs.empty() && !absorbed[c] && (r.attr_i("axis", 1) == 1 || r.attr_i("axis", 1) == -1)) concats.insert(c);
    }
  }
  for (size_t ci : concats) {
    const NodeDef &cn = m.nodes[ci];
    EmbedGroup g;
    std::map<size_t, int> slot;  // lookup -> its place in g.lookups
    for (size_t i = 0; i < cn.inputs.size(); i++) {
      const std::string &in = cn.inputs[i];
      size_t li = SIZE_MAX;
      for (size_t q = 0; q < found.size(); q++)
        if (found[q].shape.size() == 2 && found[q].out == in) li = q;
      if (li != SIZE_MAX) {
        if (!slot.count(li)) {
          slot[li] = int(g.lookups.size());
          g.lookups.push_back(found[li]);
        }
        g.parts.push_back({slot[li], EmbedCols()});
        continue;
      }
      EmbedCols c;
      if (embed_cols(in, &c).empty() && c.rank2 && c.off.empty() && !c.truncated && !c.int_input) {
        g.parts.push_back({-1, std::move(c)});
      } else {
        EmbedCols gap;
        gap.src0 = int64_t(i);  // (a gap: the Concat's input i, whatever computes it)
        g.parts.push_back({-2, std::move(gap)});
      }
    }
    embed_at[ci] = std::move(g);
  }
  for (size_t li = 0; li < found.size(); li++) {
    bool own = graph_outs.count(found[li].out) > 0;
    auto it = graph->consumers_of.find(found[li].out);
    if (it == graph->consumers_of.end() || it->second.empty()) own = true;
    else
      for (size_t c : it->second) own = own || !concats.count(c);
    if (!own) continue;
    EmbedGroup g;
    g.lookups.push_back(found[li]);
    g.parts.push_back({0, EmbedCols()});
    embed_at[found[li].tail.empty() ? found[li].gather : found[li].tail.back()] = std::move(g);
  }
  // the nodes each step stands for: its lookups and their tails, its Concat, and every node of an index / column chain that nothing
  // outside the steps reads (a chain node with another reader is lowered as before, for that reader)
  std::vector<int> owner(N, -1);  // node -> anchor
  std::set<size_t> chain_nodes;
  for (auto &ag : embed_at) {
    for (const EmbedLookup &L : ag.second.lookups) {
      const size_t last = L.tail.empty() ? L.gather : L.tail.back();
      const int who = embed_at.count(last) ? int(last) : int(ag.first);  // (a lookup that is also a step of its own is lowered there)
      owner[L.gather] = who;
      for (size_t t : L.tail) owner[t] = who;
      chain_nodes.insert(L.ix.chain.begin(), L.ix.chain.end());
    }
    owner[ag.first] = int(ag.first);
    for (const auto &p : ag.second.parts) chain_nodes.insert(p.second.chain.begin(), p.second.chain.end());
  }
  std::vector<char> gone(N, 0);
  for (size_t i = N; i-- > 0;) {
    if (!chain_nodes.count(i) || owner[i] >= 0) continue;
    bool all = true;
    for (const auto &o : m.nodes[i].outputs) {
      all = all && !graph_outs.count(o);
      if (auto it = graph->consumers_of.find(o); it != graph->consumers_of.end())
        for (size_t c : it->second) all = all && (owner[c] >= 0 || gone[c]);
    }
    gone[i] = all;
  }
  for (auto &ag : embed_at) {
    std::set<size_t> nodes;
    for (const EmbedLookup &L : ag.second.lookups) {
      nodes.insert(L.gather);
      nodes.insert(L.tail.begin(), L.tail.end());
      for (size_t c : L.ix.chain)
        if (gone[c]) nodes.insert(c);
    }
    for (const auto &p : ag.second.parts)
      for (size_t c : p.second.chain)
        if (gone[c]) nodes.insert(c);
    nodes.insert(ag.first);
    ag.second.nodes.assign(nodes.begin(), nodes.end());
  }
  // the steps read the input buffer itself: what their nodes read counts no longer (a graph input nothing else reads gets no SliceCols)
  for (size_t i = 0; i < N; i++) {
    if (owner[i] < 0 && !gone[i]) continue;
    std::set<size_t> kept;  // (a gap's value is still read: by the CopyCols that fills it)
    if (auto ag = embed_at.find(i); ag != embed_at.end())
      for (const auto &part : ag->second.parts)
        if (part.first == -2) kept.insert(size_t(part.second.src0));
    for (size_t k = 0; k < m.nodes[i].inputs.size(); k++)
      if (!kept.count(k)) uses[m.nodes[i].inputs[k]]--;
    region[i] = 0;
    if (owner[i] != int(i)) absorbed[i] = 1;
  }
}

void Lowerer::lower_embed(const EmbedGroup &g, const NodeDef &anchor) {
  auto pack = std::make_shared<EmbedPack>();
  pack->W = plan.buf_per_row[0];
  std::map<const TensorData *, int> table_id;
  int64_t out = 0;
  struct Gap { int buf; int64_t out; size_t input; };
  std::vector<Gap> gaps;  // the Concat inputs other steps compute: their buffer, first output column and place among the inputs
  for (const auto &part : g.parts) {
    if (part.first == -2) {
      const Val &v = get(anchor, size_t(part.second.src0));
      if (v.is_const) unsupported(anchor, "mixing constants and activations");
      if (v.shape.size() != 2 || v.ra != 0 || v.shape[0] != plan.input_shape[0] || v.shape[1] <= 0 || v.half)
        unsupported(anchor, "shape mismatch " + shape_str(v.shape) + " beside embedding lookups [rows, d]");
      EmbedPiece q;
      q.table = -2, q.d = v.shape[1], q.out = out;
      gaps.push_back({v.buf, out, size_t(part.second.src0)});
      out += q.d;
      pack->pieces.push_back(q);
      continue;
    }
    if (part.first < 0) {
      EmbedPiece q;
      q.src = part.second.src0, q.d = part.second.k, q.out = out;
      out += q.d;
      pack->pieces.push_back(q);
      continue;
    }
    const EmbedLookup &L = g.lookups[size_t(part.first)];
    const NodeDef &gn = m.nodes[L.gather];
    if (!table_id.count(L.table.get())) {
      table_id[L.table.get()] = int(pack->tables.size());
      pack->tables.push_back(std::shared_ptr<const std::vector<float>>(L.table, &L.table->f32));
      embed_elems += L.V * L.d;  // (every step packs and uploads its own copy, so a table counts once per step that reads it)
      if (embed_elems > kEmbedMaxTableElems)
        bad_form(gn, "the model's Embed steps hold more than 2^27 table elements (" + std::to_string(embed_elems) + "); 512 MiB is the cap");
    }
    if (!embed_node_id.count(L.gather)) {
      plan.prep_strict_nodes.push_back({"node '" + (gn.name.empty() ? gn.op : gn.name) + "' (" + gn.op + ")",
                                        ": an index is out of range for a table of " + std::to_string(L.V) + " rows"});
      embed_node_id[L.gather] = int(plan.prep_strict_nodes.size());
    }
    for (int64_t j = 0; j < L.ix.k; j++) {
      EmbedPiece q;
      q.table = table_id[L.table.get()];
      q.src = L.ix.src0 + j, q.V = L.V, q.d = L.d, q.out = out;
      q.offset = L.ix.off.empty() ? 0 : L.ix.off[size_t(j)];
      q.node = embed_node_id[L.gather];
      out += q.d;
      pack->pieces.push_back(q);
    }
  }
  const NodeDef &first = m.nodes[g.lookups[0].gather];
  if (const std::string why = pack_embed(*pack); !why.empty()) bad_form(first, why);
  Step s;
  s.kind = StepKind::Embed;
  s.in0 = 0;
  s.K = pack->W, s.M = pack->F;
  for (size_t i : g.nodes) s.origin += (s.origin.empty() ? "" : "+") + node_label(m.nodes[i]);
  std::vector<int64_t> shape = anchor.op == "Concat" ? std::vector<int64_t>{plan.input_shape[0], pack->F} : g.lookups[0].shape;
  if (shape.size() == 3) {
    pack->win_k = shape[1], pack->win_d = shape[2];
    s.rep = shape[1];
    s.embed = pack;
    return emit_window(std::move(s), anchor, shape);
  }
  s.embed = pack;
  const int out_buf = push_step(std::move(s), shape);
  for (const Gap &gp : gaps) {  // the computed inputs, each into its columns
    Step c;
    c.kind = StepKind::CopyCols;
    c.in0 = gp.buf;
    c.out = out_buf;
    c.col_off = gp.out;
    c.origin = node_label(anchor) + "[" + std::to_string(gp.input) + "]";
    plan.steps.push_back(std::move(c));
    producer[out_buf] = int(plan.steps.size()) - 1;
  }
  set_act(anchor, out_buf, shape);
}

}  // namespace lowering

}  // namespace infera_hip
