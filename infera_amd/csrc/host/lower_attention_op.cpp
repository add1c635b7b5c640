// lower_attention_op.cpp -- struct Lowerer (lowerer.hpp): the opset-23 operators Attention and RMSNormalization of the standard domain.
// find_attention_ops fills the AttnMatch of lowerer.hpp ("self-attention") for every Attention node, anchored where the step is emitted;
// lower_attention (lowering.cpp) validates shapes and constants and emits ONE Attention step, as for the pattern form.
// Which forms are served and which are refused: INTEGRATION.md section 2.6 ("The Attention operator", "RMSNormalization").

#include <cmath>

#include "lowerer.hpp"

namespace infera_hip {

namespace lowering {

void Lowerer::find_attention_ops() {
  const std::vector<int64_t> split_perm{0, 2, 1, 3};
  auto perm_of = [&](const NodeDef &t) {
    std::vector<int64_t> p;
    if (auto *q = t.attr_ints("perm")) p = *q;
    return p;
  };
  auto idx = [&](const NodeDef *n) { return size_t(n - m.nodes.data()); };
  for (size_t ni = 0; ni < m.nodes.size(); ni++) {
    const NodeDef &n = m.nodes[ni];
    if (!graph->live[ni] || n.op != "Attention" || !graph->std_dom(n) || absorbed[ni]) continue;
    auto given = [&](size_t i) { return i < n.inputs.size() && !n.inputs[i].empty(); };
    auto consumed = [&](size_t o) {
      if (o >= n.outputs.size() || n.outputs[o].empty()) return false;
      auto it = graph->consumers_of.find(n.outputs[o]);
      return graph->graph_outs.count(n.outputs[o]) > 0 || (it != graph->consumers_of.end() && !it->second.empty());
    };
    if (!given(0) || !given(1) || !given(2)) bad_form(n, "Q, K and V are required");
    if (given(4) || given(5)) bad_form(n, "past_key / past_value (a KV cache) is not supported");
    if (given(6)) bad_form(n, "nonpad_kv_seqlen is not supported; pass the padding as a bool attn_mask [N,1,1,Tk]");
    static const char *outs[] = {"Y", "present_key", "present_value", "qk_matmul_output"};
    for (size_t o = 1; o < 4; o++)
      if (consumed(o)) bad_form(n, std::string("output ") + outs[o] + " is consumed; only Y is served");
    if (n.attr_f("softcap", 0.f) != 0.f) bad_form(n, "softcap = " + std::to_string(n.attr_f("softcap", 0.f)) + " is not supported (only 0)");
    if (const int64_t sp = n.attr_i("softmax_precision", 0); sp != 0 && sp != onnx::kFloat)
      bad_form(n, "softmax_precision = " + std::to_string(sp) + "; only float (1)");
    for (size_t i = 0; i < 3; i++)
      if (!graph->row_data.count(n.inputs[i])) bad_form(n, std::string("operand ") + "QKV"[i] + " is a constant; only activations");

    AttnMatch am;
    am.qk = am.op = &n;
    am.nodes.push_back(ni);
    // an operand behind its head split: Reshape [N,T,h,dh] -> Transpose(0,2,1,3), each read by the next alone
    auto head_split = [&](const std::string &operand, AttnSide &side) {
      if (graph->sole_reader(operand, true) != &n) return false;
      // (a rotary embedding on the head-major value, lower_rotary.cpp: the split is looked for behind it, and its readers are the embedding's)
      std::shared_ptr<const RotaryMatch> rot;
      const std::string v = behind_rotary(operand, &rot);
      const NodeDef *t = graph->producer(v);
      if (!t || t->op != "Transpose" || !graph->std_dom(*t) || perm_of(*t) != split_perm) return false;
      const NodeDef *r = graph->producer(t->inputs[0]);
      if (!r || r->op != "Reshape" || !graph->std_dom(*r) || r->inputs.size() != 2 || graph->sole_reader(t->inputs[0], false) != t) return false;
      if (rot) am.nodes.insert(am.nodes.end(), rot->nodes.begin(), rot->nodes.end());
      side.rot = rot;
      am.nodes.push_back(idx(t));
      am.nodes.push_back(idx(r));
      side.src = r->inputs[0];
      side.shape = r->inputs[1];
      return true;
    };
    int split = 0;
    bool is_split[3];
    for (int i = 0; i < 3; i++) {
      // (Q = K = V of one value: one split read three times by this node)
      bool seen = false;
      for (int j = 0; j < i; j++)
        if (n.inputs[size_t(j)] == n.inputs[size_t(i)]) am.side[i] = am.side[j], is_split[i] = is_split[j], seen = true;
      if (!seen) is_split[i] = head_split(n.inputs[size_t(i)], am.side[i]);
      split += is_split[i];
    }
    if (split == 0 && n.attr("q_num_heads") && n.attr("kv_num_heads")) {
      am.form3 = true;
      for (int i = 0; i < 3; i++) am.side[i].src = n.inputs[size_t(i)];
    } else if (split != 3) {
      for (int i = 0; i < 3; i++)
        if (!is_split[i])
          bad_form(n, std::string("operand ") + "QKV"[i] + " '" + n.inputs[size_t(i)] + "' is neither an [N,T,h*dh] value beside q_num_heads / kv_num_heads nor the head split Reshape [N,T,h,dh] -> "
                          "Transpose(0,2,1,3) of one, read by this node alone (a head-major [N,h,T,dh] tensor such as a graph input is not supported)");
    }
    // a Split / Slice cut of a packed projection on the last axis, as in the pattern form
    for (AttnSide &side : am.side) {
      const NodeDef *c = graph->producer(side.src);
      if (!c || (c->op != "Split" && c->op != "Slice") || !graph->std_dom(*c)) continue;
      int64_t axis = -100;
      if (c->op == "Split") axis = c->attr_i("axis", 0);
      else if (std::vector<int64_t> ax; c->inputs.size() >= 4 && graph_ints_arg(*c, 3, "axes", &ax) && ax.size() == 1) axis = ax[0];
      if (axis != 2 && axis != -1) continue;
      side.cut = c;
      side.cut_out = size_t(std::find(c->outputs.begin(), c->outputs.end(), side.src) - c->outputs.begin());
      am.nodes.push_back(idx(c));
      side.src = c->inputs[0];
    }
    size_t anchor = ni;
    if (!am.form3) {  // Y [N,h,Tq,dh] goes back to rows first and nowhere else
      const NodeDef *t = graph->sole_reader(n.outputs[0], false);
      const NodeDef *r = t && t->op == "Transpose" && perm_of(*t) == split_perm ? graph->sole_reader(t->outputs[0], false) : nullptr;
      if (!r || r->op != "Reshape" || r->inputs.size() != 2 || r->inputs[0] != t->outputs[0]) {
        std::string who = graph->graph_outs.count(n.outputs[0]) ? "the graph output" : "several nodes";
        if (t) who = "'" + node_label(r ? *r : *t) + "'";
        bad_form(n, "Y is read as [N,h,T,dh] by " + who + "; only Transpose(0,2,1,3) -> Reshape [N,Tq,hq*dh]");
      }
      am.nodes.push_back(idx(t));
      anchor = idx(r);
    }
    if (given(3) && graph->row_data.count(n.inputs[3])) {  // a row's own key mask: bool [N,1,1,Tk], true = kept
      std::string v = n.inputs[3];
      const NodeDef *p = nullptr;
      for (int hop = 0; hop < 32; hop++) {
        p = graph->producer(v);
        if (!p || p->inputs.empty() || (p->op != "Unsqueeze" && p->op != "Reshape" && p->op != "Expand")) break;
        v = p->inputs[0];
      }
      const bool is_bool = p && (p->op == "Equal" || p->op == "Not" || (p->op == "Cast" && p->attr_i("to", onnx::kFloat) == onnx::kBool));
      if (!is_bool && (!p || p->op == "Cast"))
        bad_form(n, "attn_mask '" + n.inputs[3] + "' is a float (or integer) mask that depends on the row; only a bool mask [N,1,1,Tk] (Cast(to = BOOL), Not(Equal(ids, pad)))");
      auto rm = std::make_shared<RowMask>();
      if (const std::string why = trace_row_mask(n.inputs[3], rm.get()); !why.empty()) bad_form(n, why);
      if (rm->state == 1)
        bad_form(n, "attn_mask is true at the keys that EQUAL the compare value, and the operator keeps the keys where it is true; write Not(Equal(...))");
      rm->at = &n;
      rm->mode = kRowMaskReplace;
      rm->fill = -INFINITY;
      am.rm = std::move(rm);
    } else if (given(3)) {
      am.mask = n.inputs[3];
    }
    for (size_t i : am.nodes) absorbed[i] = 1;
    attn_at[anchor] = std::move(am);
  }
}

void Lowerer::rms_norm(const NodeDef &n) {
  const Val a = get(n, 0);
  const int64_t rank = int64_t(a.shape.size());
  if (a.is_const || rank < 2 || rank > 3) unsupported(n, "unsupported operator form: the input must be a [rows, E] or [rows, T, E] activation");
  int64_t axis = n.attr_i("axis", -1);
  if (axis < 0) axis += rank;
  if (axis != rank - 1)
    unsupported(n, "unsupported operator form: only normalisation over the last axis (axis = -1) is supported, got axis " + std::to_string(n.attr_i("axis", -1)) + " of " +
                       shape_str(a.shape));
  if (n.attr_i("stash_type", onnx::kFloat) != onnx::kFloat) unsupported(n, "unsupported operator form: stash_type = " + std::to_string(n.attr_i("stash_type", 1)) + "; only float (1)");
  if (!has_input(n, 1)) unsupported(n, "unsupported operator form: scale is required");
  const int64_t E = a.shape[size_t(rank - 1)];
  if (E < 1 || E > kLnMaxE) unsupported(n, "unsupported operator form: E = " + std::to_string(E) + " is beyond the RmsNorm kernel's cap of " + std::to_string(kLnMaxE));
  const Val &g = get(n, 1);
  if (!g.is_const) unsupported(n, "unsupported operator form: scale is not a constant");
  Step s;
  s.kind = StepKind::RmsNorm;
  s.in0 = a.buf;
  s.K = E;
  s.rep = prod(a.shape, 1) / E;
  s.scale = cf32(n, g);
  if (int64_t(s.scale.size()) != E || g.shape.size() > 1) unsupported(n, "unsupported operator form: scale must be a vector of E = " + std::to_string(E) + " elements, got " + shape_str(g.shape));
  s.ln_eps = n.attr_f("epsilon", 1e-5f);
  if (!(s.ln_eps >= 0.f) || !std::isfinite(s.ln_eps)) unsupported(n, "unsupported operator form: epsilon must be a finite number >= 0");
  if (rank == 3) emit_window(std::move(s), n, a.shape);
  else emit(std::move(s), n, a.shape);
}

}  // namespace lowering

}  // namespace infera_hip
