// lower_prep.cpp -- struct Lowerer (lowerer.hpp): ai.onnx.ml preprocessing regions.
// The state, the match structs and the block that explains them stand in lowerer.hpp under "ai.onnx.ml preprocessing regions";
// which graphs are served and which are refused: INTEGRATION.md section 2.6.
#include <algorithm>
#include <cmath>
#include <functional>
#include <numeric>

#include "lowerer.hpp"
#include "prep.hpp"

namespace infera_hip {

namespace lowering {

bool Lowerer::prep_encoder(const std::string &op) {
  return op == "Imputer" || op == "Binarizer" || op == "OneHotEncoder" || op == "LabelEncoder" || op == "FeatureVectorizer";
}
// marks `region`; returns the graph inputs that start inside a region
std::set<std::string> Lowerer::find_regions() {
  const size_t N = m.nodes.size(), M = m.inputs.size();
  const std::map<std::string, size_t> &prod_of = graph->producer_of;
  std::map<std::string, size_t> input_of;
  for (size_t j = 0; j < M; j++) input_of[m.inputs[j].name] = j;
  const std::set<std::string> &act = graph->row_data;  // names that hold row data
  std::vector<char> elig(N, 0), trig(N + M, 0);
  std::vector<size_t> uf(N + M);
  std::iota(uf.begin(), uf.end(), size_t(0));
  std::function<size_t(size_t)> find = [&](size_t a) { return uf[a] == a ? a : uf[a] = find(uf[a]); };
  auto from_region = [&](const std::string &v) {  // a graph input or an eligible node's output
    auto p = prod_of.find(v);
    return input_of.count(v) || (p != prod_of.end() && elig[p->second]);
  };
  for (size_t i = 0; i < N; i++) {
    if (!graph->live[i]) continue;
    const NodeDef &n = m.nodes[i];
    bool any_act = false;
    for (const auto &in : n.inputs) any_act = any_act || act.count(in);
    if (!any_act) continue;
    const bool ml = n.domain == "ai.onnx.ml", std_dom = graph->std_dom(n);
    const bool data_act = !n.inputs.empty() && act.count(n.inputs[0]);
    bool e = false, t = false;
    if (ml && n.op == "ArrayFeatureExtractor") {
      e = data_act && n.inputs.size() == 2 && bool(graph->constant(n.inputs[1]));
      if (e) {  // non-contiguous constant indices: nothing else serves them
        auto ci = m.initializers.find(n.inputs[1]);
        if (ci != m.initializers.end() && ci->second->dtype == onnx::kInt64) {
          const auto &v = ci->second->i64;
          for (size_t k = 1; k < v.size(); k++) t = t || v[k] != v[0] + int64_t(k);
        } else {
          t = true;  // (a Constant node's list: checked when lowered)
        }
      }
    } else if (ml && (prep_encoder(n.op) || n.op == "Scaler")) {
      e = data_act;
      t = e && n.op != "Scaler";
    } else if (std_dom && (n.op == "Cast" || n.op == "Reshape" || n.op == "Flatten" || n.op == "Squeeze" || n.op == "Identity")) {
      e = data_act;
    } else if (std_dom && n.op == "Concat") {
      e = true;
      for (const auto &in : n.inputs) e = e && act.count(in) && from_region(in);
    }
    if (!e) continue;
    elig[i] = 1;
    if (t) trig[i] = 1;
    for (const auto &in : n.inputs) {
      if (!act.count(in)) continue;
      auto ij = input_of.find(in);
      auto p = prod_of.find(in);
      if (ij != input_of.end()) uf[find(i)] = find(N + ij->second);
      else if (p != prod_of.end() && elig[p->second]) uf[find(i)] = find(p->second);
    }
  }
  for (size_t j = 0; j < M; j++)
    if (m.inputs[j].elem_type == onnx::kInt64 || m.inputs[j].elem_type == onnx::kInt32) trig[N + j] = 1;
  std::vector<char> hot(N + M, 0);
  for (size_t a = 0; a < N + M; a++)
    if (trig[a]) hot[find(a)] = 1;
  region.assign(N, 0);
  for (size_t i = 0; i < N; i++) region[i] = elig[i] && hot[find(i)];
  std::set<std::string> ins;
  for (size_t j = 0; j < M; j++)
    if (hot[find(N + j)]) ins.insert(m.inputs[j].name);
  return ins;
}

// identity columns over buffer `buf` (a region value's source); is_int: whole numbers already
PrepVal Lowerer::prep_identity(int buf, int64_t off, int64_t width, bool trunc, bool is_int) {
  PrepVal p;
  p.src = buf;
  for (int64_t j = 0; j < width; j++) {
    PrepCol c;
    c.src = off + j;
    c.trunc = trunc;
    c.is_int = is_int || trunc;
    p.cols.push_back(c);
  }
  return p;
}
void Lowerer::set_prep(const std::string &name, PrepVal p, std::vector<int64_t> shape) {
  if (int64_t(p.cols.size()) > kPrepMaxOut)
    throw InferaError::onnx("value '" + name + "' has " + std::to_string(p.cols.size()) + " columns; a preprocessing step writes at most " +
                            std::to_string(kPrepMaxOut));
  Val v;
  v.pv = std::make_shared<const PrepVal>(std::move(p));
  v.shape = std::move(shape);
  vals[name] = v;
}
// input i of a region node as columns: a region value as it is, an activation as identity columns over its buffer.  Columns that
// already went past `stage` (an Imputer behind a Scaler, ...) are materialised first, and the program starts again on that buffer.
PrepVal Lowerer::prep_in(const NodeDef &n, size_t i, int stage) {
  const Val *v = &get_raw(n, i);
  if (v->is_const) unsupported(n, "expected row data, got a constant");
  if (v->pv) {
    bool clash = false;
    for (const PrepCol &c : v->pv->cols) clash = clash || c.stage() >= stage;
    if (!clash) return *v->pv;
    v = &get(n, i);
  }
  if (v->padded()) unsupported(n, "the output of a Pad node can only feed a Conv");
  PrepVal p = prep_identity(v->buf, 0, plan.buf_per_row[size_t(v->buf)], false, int_bufs.count(v->buf) > 0);
  return p;
}
// the region value `name` becomes a buffer: the source itself, a SliceCols, or one Prep step
void Lowerer::materialize(const std::string &name, const NodeDef *at) {
  Val &v = vals[name];
  const std::shared_ptr<const PrepVal> keep = v.pv;
  const PrepVal &p = *keep;
  const std::vector<int64_t> shape = v.shape;
  const int64_t F = int64_t(p.cols.size()), src_w = plan.buf_per_row[size_t(p.src)];
  bool plain = true, contiguous = true;
  for (int64_t j = 0; j < F; j++) {
    plain = plain && p.cols[size_t(j)].plain();
    contiguous = contiguous && p.cols[size_t(j)].src == p.cols[0].src + j;
  }
  Val r;
  r.shape = shape;
  if (plain && contiguous && p.cols[0].src == 0 && F == src_w) {  // the source as it is
    r.buf = p.src;
    v = r;
    buf_names[r.buf].push_back(name);
    alias_edges[r.buf]++;
    return;
  }
  Step s;
  s.in0 = p.src;
  if (plain && contiguous) {
    s.kind = StepKind::SliceCols;
    s.col_off = p.cols[0].src;
    s.K = F;
  } else {
    try {
      s.prep = std::make_shared<const PrepPack>(pack_prep(p.cols, prep_tables, src_w));
    } catch (const PrepError &e) {
      if (at) unsupported(*at, std::string("preprocessing step: ") + e.what());
      throw InferaError::onnx("output '" + name + "': preprocessing step: " + e.what());
    }
    s.kind = StepKind::Prep;
  }
  for (const auto &o : p.origin) s.origin += (s.origin.empty() ? "" : "+") + o;
  if (s.origin.empty()) s.origin = "input:" + name;  // (only a graph input's columns as they are absorb no node)
  r.buf = push_step(std::move(s), {shape[0], F});
  bool all_int = true;
  for (const PrepCol &c : p.cols) all_int = all_int && c.is_int;
  if (all_int) int_bufs.insert(r.buf);
  v = r;
  buf_names[r.buf].push_back(name);
}

std::vector<int64_t> Lowerer::afe_indices(const NodeDef &n) {
  const Val &ix = get_raw(n, 1);
  if (!ix.is_const || ix.c->dtype != onnx::kInt64 || ix.c->i64.empty()) unsupported(n, "indices must be a constant int64 list");
  return ix.c->i64;
}
// the inputs of n as they are (stage 5: nothing is materialised), their columns side by side in *out; false: an input reads another
// source than input 0
bool Lowerer::prep_side_by_side(const NodeDef &n, PrepVal *out) {
  *out = prep_in(n, 0, 5);
  for (size_t i = 1; i < n.inputs.size(); i++) {
    const PrepVal q = prep_in(n, i, 5);
    if (q.src != out->src) return false;
    out->append(q);
  }
  out->add_origin(node_label(n));
  return true;
}
// columns of region values with one source side by side (Concat / FeatureVectorizer); false: the sources differ
bool Lowerer::prep_concat(const NodeDef &n, std::vector<int64_t> out_shape) {
  PrepVal out;
  for (size_t i = 0; i < n.inputs.size(); i++) {
    const Val &v = get_raw(n, i);
    if (v.is_const || !v.pv) return false;
    if (i && v.pv->src != out.src) return false;
    if (!i) out.src = v.pv->src;
  }
  for (size_t i = 0; i < n.inputs.size(); i++) out.append(*get_raw(n, i).pv);
  out.add_origin(node_label(n));
  out_shape[1] = int64_t(out.cols.size()) / std::max<int64_t>(1, prod(out_shape, 2));
  set_prep(n.outputs[0], std::move(out), out_shape);
  return true;
}
void Lowerer::prep_node(const NodeDef &n) {
  const std::string &op = n.op;
  if (op == "Identity" || op == "Reshape" || op == "Flatten" || op == "Squeeze") return reshape_like(n);
  if (op == "Cast") {
    const Val &a = get_raw(n, 0);
    const int64_t to = n.attr_i("to", onnx::kFloat);
    if (!a.pv || !(to == onnx::kInt64 || to == onnx::kInt32)) return cast(n);  // (to float: an alias)
    PrepVal p = *a.pv;
    bool clash = false;  // a column that is not whole yet and went past the truncation stage: materialised first
    for (const PrepCol &c : p.cols) clash = clash || (!c.is_int && c.stage() >= 1);
    if (clash) p = prep_in(n, 0, 1);
    for (PrepCol &c : p.cols)
      if (!c.is_int) c.trunc = true, c.is_int = true;
    p.add_origin(node_label(n));
    return set_prep(n.outputs[0], std::move(p), a.shape);
  }
  if (op == "Concat") {
    const Val &first = get_raw(n, 0);
    const int64_t rank = int64_t(first.shape.size());
    int64_t axis = n.attr_i("axis", 1);
    if (axis < 0) axis += rank;
    bool flat = axis >= 1 && axis < rank;  // a flat concatenation of rows: every axis between the row axis and `axis` has extent 1
    std::vector<int64_t> out_shape = first.shape;
    for (size_t i = 0; i < n.inputs.size() && flat; i++) {
      const Val &v = get_raw(n, i);
      flat = !v.is_const && int64_t(v.shape.size()) == rank;
      for (int64_t d = 1; d < rank && flat; d++) flat = d == axis || v.shape[size_t(d)] == first.shape[size_t(d)];
      for (int64_t d = 1; d < axis && flat; d++) flat = v.shape[size_t(d)] == 1;
    }
    if (flat && axis != 1) {  // [N, 1, a] ++ [N, 1, b] -> [N, 1, a + b]
      int64_t total = 0;
      for (size_t i = 0; i < n.inputs.size(); i++) total += get_raw(n, i).shape[size_t(axis)];
      out_shape[size_t(axis)] = total;
      PrepVal p;
      if (!prep_side_by_side(n, &p)) unsupported(n, "a preprocessing Concat over the last axis reads one source");
      return set_prep(n.outputs[0], std::move(p), out_shape);
    }
    if (axis == 1 && flat && prep_concat(n, out_shape)) return;
    return concat(n);
  }
  if (op == "FeatureVectorizer") {
    const std::vector<int64_t> *dims = n.attr_ints("inputdimensions");
    if (!dims || dims->size() != n.inputs.size())
      unsupported(n, "inputdimensions must hold one entry per input (" + std::to_string(n.inputs.size()) + ")");
    int64_t total = 0;
    for (size_t i = 0; i < n.inputs.size(); i++) {
      const Val &v = get_raw(n, i);
      if (v.is_const || v.shape.empty()) unsupported(n, "inputs must be row data");
      const int64_t w = prod(v.shape, 1);
      if ((*dims)[i] != w)
        unsupported(n, "inputdimensions[" + std::to_string(i) + "] = " + std::to_string((*dims)[i]) + " but input '" + n.inputs[i] + "' has " +
                           std::to_string(w) + " columns");
      total += w;
    }
    const std::vector<int64_t> out_shape = {get_raw(n, 0).shape[0], total};
    // (each input as [rows, width]; the sources differ: materialised and copied side by side)
    const Val &v0 = get_raw(n, 0);
    bool one_src = v0.pv != nullptr;
    for (size_t i = 1; i < n.inputs.size() && one_src; i++) {
      const Val &v = get_raw(n, i);
      one_src = v.pv && v.pv->src == v0.pv->src;
    }
    PrepVal cat;
    if (one_src && prep_side_by_side(n, &cat)) return set_prep(n.outputs[0], std::move(cat), out_shape);
    std::vector<std::string> flat;
    for (size_t i = 0; i < n.inputs.size(); i++) {
      const Val &v = get(n, i);
      const std::string f = n.outputs[0] + "\x01" + std::to_string(i);
      Val a = v;
      a.shape = {v.shape[0], prod(v.shape, 1)};
      vals[f] = a;
      uses[f] = 1;
      flat.push_back(f);
    }
    NodeDef c = std_node(n, "Concat", flat, n.outputs[0]);
    set_i(c, "axis", 1);
    return concat(c);
  }
  // the per-column nodes: rows of [N, F] (LabelEncoder: any shape)
  const Val &x = get_raw(n, 0);
  const std::vector<int64_t> xshape = x.shape;
  if (x.is_const) unsupported(n, "expected row data, got a constant");
  if (op != "LabelEncoder" && xshape.size() != 2) unsupported(n, "only [rows, features] inputs");
  const int64_t F = prod(xshape, 1);
  PrepVal p;
  std::vector<int64_t> out_shape = xshape;
  if (op == "ArrayFeatureExtractor") {
    const std::vector<int64_t> ix = afe_indices(n);
    const PrepVal in = prep_in(n, 0, 5);
    p.src = in.src;
    p.origin = in.origin;
    for (int64_t k : ix) {
      if (k < 0) unsupported(n, "negative column index " + std::to_string(k));
      if (k >= F) unsupported(n, "column index " + std::to_string(k) + " out of range for " + std::to_string(F) + " columns");
      p.cols.push_back(in.cols[size_t(k)]);
    }
    out_shape = {xshape[0], int64_t(ix.size())};
  } else if (op == "Imputer") {
    ImputerSpec sp;
    try {
      sp = parse_imputer(n, F);
    } catch (const PrepError &e) {
      unsupported(n, e.what());
    }
    p = prep_in(n, 0, 2);
    for (int64_t j = 0; j < F; j++) {
      PrepCol &c = p.cols[size_t(j)];
      c.impute = true;
      c.imp_nan = std::isnan(sp.replaced);
      c.repl = sp.replaced;
      c.imp = sp.imputed[size_t(j)];
      c.is_int = c.is_int && std::nearbyint(c.imp) == c.imp;
    }
  } else if (op == "Scaler") {
    const std::vector<float> off = ml_floats(n, "offset", F, 0.f, true), sc = ml_floats(n, "scale", F, 1.f, true);
    p = prep_in(n, 0, 3);
    for (int64_t j = 0; j < F; j++) {
      PrepCol &c = p.cols[size_t(j)];
      c.affine = true;
      c.off = off[size_t(j)];
      c.scale = sc[size_t(j)];
      c.is_int = false;
    }
  } else if (op == "Binarizer") {
    const float thr = parse_binarizer(n);
    p = prep_in(n, 0, 4);
    for (PrepCol &c : p.cols) c.kind = kPrepBin, c.c = thr, c.is_int = true;
  } else if (op == "OneHotEncoder") {
    OneHotSpec sp;
    try {
      sp = parse_onehot(n);
    } catch (const PrepError &e) {
      unsupported(n, e.what());
    }
    const int64_t C = int64_t(sp.cats.size());
    prep_cats += C;
    if (prep_cats > kPrepMaxCats) unsupported(n, "more than " + std::to_string(kPrepMaxCats) + " one-hot categories in all");
    if (F * C > kPrepMaxOut)
      unsupported(n, std::to_string(F) + " x " + std::to_string(C) + " one-hot columns; a preprocessing step writes at most " + std::to_string(kPrepMaxOut));
    int table = -1, strict = 0;
    if (!sp.zeros) {
      prep_tables.push_back(std::make_shared<PrepTable>(onehot_table(sp.cats)));
      table = int(prep_tables.size()) - 1;
      plan.prep_strict_nodes.push_back({"node '" + (n.name.empty() ? n.op : n.name) + "' (" + n.op + ")", ": a value is not in cats_int64s (zeros = 0)"});
      strict = int(std::min<size_t>(plan.prep_strict_nodes.size(), size_t(kPrepMaxStrictIds)));
    }
    const PrepVal in = prep_in(n, 0, 4);
    p.src = in.src;
    p.origin = in.origin;
    for (const PrepCol &base : in.cols)
      for (int64_t k = 0; k < C; k++) {
        PrepCol c = base;
        c.kind = kPrepOneHot;
        c.c = sp.cats[size_t(k)];
        c.is_int = true;
        if (k == 0) c.table = table, c.strict = strict;
        p.cols.push_back(c);
      }
    out_shape = {xshape[0], F, C};
  } else if (op == "LabelEncoder") {
    bool int_values = false;
    PrepTable t;
    try {
      t = parse_label_encoder(n, &int_values);
    } catch (const PrepError &e) {
      unsupported(n, e.what());
    }
    prep_keys += int64_t(t.keys.size()) + (t.has_nan ? 1 : 0);
    if (prep_keys > kPrepMaxKeys) unsupported(n, "more than " + std::to_string(kPrepMaxKeys) + " LabelEncoder keys in all");
    const float dflt = t.dflt;
    prep_tables.push_back(std::make_shared<PrepTable>(std::move(t)));
    p = prep_in(n, 0, 4);
    for (PrepCol &c : p.cols) c.kind = kPrepLookup, c.c = dflt, c.table = int(prep_tables.size()) - 1, c.is_int = int_values;
  } else {
    unsupported(n, "unsupported operator");
  }
  p.add_origin(node_label(n));
  set_prep(n.outputs[0], std::move(p), out_shape);
}

}  // namespace lowering

}  // namespace infera_hip
