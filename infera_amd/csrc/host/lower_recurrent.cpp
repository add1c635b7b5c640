// lower_recurrent.cpp -- struct Lowerer (lowerer.hpp): LSTM / GRU / RNN and their per-row sequence lengths.
// The state, the match structs and the block that explains them stand in lowerer.hpp under "per-row sequence lengths";
// which graphs are served and which are refused: INTEGRATION.md section 2.6 ("Padded windows").
#include <algorithm>

#include "lowerer.hpp"
#include "recurrent.hpp"

namespace infera_hip {

namespace lowering {

void Lowerer::find_seq_lens() {
  std::set<size_t> chain;
  for (size_t i = 0; i < m.nodes.size(); i++) {
    const NodeDef &n = m.nodes[i];
    if (!graph->live[i] || !graph->std_dom(n) || (n.op != "LSTM" && n.op != "GRU" && n.op != "RNN") || !has_input(n, 4) || !graph->row_data.count(n.inputs[4])) continue;
    RowMask r;
    if (const std::string why = trace_row_mask(n.inputs[4], &r, true); !why.empty()) bad_form(n, why);
    if (r.k != 1 || r.shape != std::vector<int64_t>{-1})
      bad_form(n, "sequence_lens traced to " + std::to_string(r.k) + " column" + (r.k == 1 ? "" : "s") + " of a graph input as " + shape_str(r.shape) +
                      "; only one length per row, [N]");
    if (!r.is_int) bad_form(n, "sequence_lens read from a float graph input without a Cast to an integer type");
    if (plan.input_declared_type == "float16") bad_form(n, "sequence_lens taken from a float16 graph input");
    if (r.src0 < 0 || r.src0 >= plan.buf_per_row[0]) bad_form(n, "the sequence_lens column lies outside the input");
    plan.prep_strict_nodes.push_back({"node '" + (n.name.empty() ? n.op : n.name) + "' (" + n.op + ")", ": sequence_lens outside 0…T"});
    seq_lens_at[i] = {r.src0, r.is_int, int(plan.prep_strict_nodes.size())};
    chain.insert(r.nodes.begin(), r.nodes.end());
  }
  // what a tracing node computes is read by recurrent layers as sequence_lens and by nothing else
  const std::string &served = m.outputs[out_index].name;
  for (size_t i : chain)
    for (const auto &o : m.nodes[i].outputs) {
      bool ok = o != served;
      if (auto it = graph->consumers_of.find(o); it != graph->consumers_of.end())
        for (size_t c : it->second) {
          const NodeDef &r = m.nodes[c];
          const bool as_lens = seq_lens_at.count(c) && std::count(r.inputs.begin(), r.inputs.end(), o) == 1 && r.inputs[4] == o;
          ok = ok && (chain.count(c) || as_lens);
        }
      if (!ok) bad_form(m.nodes[i], "this node of a sequence_lens sub-graph also feeds nodes outside the recurrent layers' sequence_lens");
    }
  for (size_t i : chain) {
    absorbed[i] = 1;
    region[i] = 0;
    for (const auto &in : m.nodes[i].inputs)
      if (!in.empty()) uses[in]--;
  }
  for (const auto &kv : seq_lens_at) uses[m.nodes[kv.first].inputs[4]]--;
}

// LSTM / GRU / RNN: one Recurrent step per output that is read.  X is [T, rows, F] (layout 0: time-major, row-axis tag 1) or
// [rows, T, F] (layout 1); the step writes Y as [rows, T, D, H] and the last states as [rows, D, H], and the values carry ONNX's shapes
// with the row-axis tag that makes them so
void Lowerer::recurrent(const NodeDef &n) {
  if (n.inputs.size() < 3 || n.inputs[0].empty() || n.inputs[1].empty() || n.inputs[2].empty())
    unsupported(n, "unsupported operator form: needs the three inputs X, W, R");
  const Val x = get(n, 0);
  const int64_t layout = n.attr_i("layout", 0) == 1 ? 1 : 0;
  if (x.is_const || x.shape.size() != 3 || x.ra != 1 - layout)
    unsupported(n, std::string("unsupported operator form: X must be ") + (layout ? "[rows, T, F] (layout 1)" : "[T, rows, F] (layout 0: a Transpose(1,0,2) of the rows-first input)") +
                       ", got " + shape_str(x.shape) + " with the row axis at " + std::to_string(x.ra));
  auto arg = [&](size_t i) {
    RnnInput r;
    if (!has_input(n, i)) return r;
    r.present = true;
    const Val &v = get(n, i);
    if (v.is_const) r.c = v.c.get();
    return r;
  };
  const bool lstm = n.op == "LSTM";
  auto sl = seq_lens_at.find(size_t(&n - m.nodes.data()));  // (traced: the value itself was never produced)
  const bool lens = sl != seq_lens_at.end();
  std::shared_ptr<const RnnPack> rp;
  try {
    rp = std::make_shared<const RnnPack>(pack_recurrent(n, x.shape[size_t(layout)], x.shape[2], arg(1), arg(2), arg(3), lens ? RnnInput{} : arg(4), arg(5),
                                                        lstm ? arg(6) : RnnInput{}, lstm ? arg(7) : RnnInput{}));
  } catch (const RnnError &e) {
    unsupported(n, e.what());
  }
  const int64_t N = x.shape[size_t(x.ra)], T = rp->T, D = rp->D, H = rp->H;
  for (size_t o = 0; o < (lstm ? 3u : 2u); o++) {
    if (!wanted(n, o)) continue;
    Step s;
    s.kind = StepKind::Recurrent;
    s.in0 = x.buf;
    s.rnn = rp;
    s.out_mode = o == 0 ? kRnnY : o == 1 ? kRnnYh : kRnnYc;
    if (lens) {
      s.in3 = 0;
      s.rm_off = sl->second.col;
      s.rm_int = sl->second.is_int;
      s.rnn_node = sl->second.node;
    }
    s.origin = node_label(n);
    Val v;
    v.buf = push_step(std::move(s), {N, o == 0 ? T * D * H : D * H});
    if (o == 0) v.shape = layout ? std::vector<int64_t>{N, T, D, H} : std::vector<int64_t>{T, D, N, H};
    else v.shape = layout ? std::vector<int64_t>{N, D, H} : std::vector<int64_t>{D, N, H};
    v.ra = layout ? 0 : (o == 0 ? 2 : 1);
    vals[n.outputs[o]] = v;
    buf_names[v.buf].push_back(n.outputs[o]);
  }
}

}  // namespace lowering

}  // namespace infera_hip
