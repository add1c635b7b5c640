// lower_shuffle.cpp -- struct Lowerer (lowerer.hpp): the sub-pixel layers.  The operators DepthToSpace (DCR, CRD) and SpaceToDepth and the four
// Reshape -> Transpose -> Reshape spellings exporters write for them (nn.PixelShuffle below opset 11, F.pixel_unshuffle everywhere, the
// specification's own definition of the two operators) all become ONE PixelShuffle step (host/pixelshuffle.hpp, hip/pixelshuffle.hip).
//   form                    first Reshape target         Transpose perm
//   DepthToSpace DCR        [N, b, b, C', H, W]          (0,3,4,1,5,2)
//   DepthToSpace CRD        [N, C', b, b, H, W]          (0,1,4,2,5,3)
//   SpaceToDepth            [N, C, H/b, b, W/b, b]       (0,3,5,1,2,4)
//   pixel_unshuffle         [N, C, H/b, b, W/b, b]       (0,1,3,5,2,4)
// find_pixel_shuffles claims the three nodes by structure before the walk (operators, the perm, sole readers), anchored at the last Reshape,
// where both targets are constants (or folded Shape sub-graphs) by the time the walk arrives; pixel_shuffle_spelling checks them against the
// input's shape.  Whatever is not exactly one of the four is lowered node by node as without the matcher, and refused where it was before.

#include "lowerer.hpp"
#include "pixelshuffle.hpp"

namespace infera_hip {

namespace lowering {

namespace {

struct Spelling {
  std::vector<int64_t> perm;
  bool to_space, channel_major;
};
const Spelling kSpellings[] = {
    {{0, 3, 4, 1, 5, 2}, true, false},
    {{0, 1, 4, 2, 5, 3}, true, true},
    {{0, 3, 5, 1, 2, 4}, false, false},
    {{0, 1, 3, 5, 2, 4}, false, true},
};

// A Reshape target against the shape `in` it is applied to: 0 copies the extent at its own index, one -1 is inferred; the leading entry must
// denote the row axis (0, -1 or the fixed batch).  false: it does not resolve
bool resolve_target(std::vector<int64_t> tgt, const std::vector<int64_t> &in, std::vector<int64_t> *out) {
  if (tgt.empty() || in.empty()) return false;
  if (!(tgt[0] == 0 || tgt[0] == -1 || (tgt[0] > 0 && tgt[0] == in[0]))) return false;
  int64_t per_row = 1, rest = 1;
  for (size_t i = 1; i < in.size(); i++) per_row *= in[i];
  int neg = -1;
  for (size_t i = 1; i < tgt.size(); i++) {
    if (tgt[i] == 0) {
      if (i >= in.size()) return false;
      tgt[i] = in[i];
    }
    if (tgt[i] == -1) {
      if (neg >= 0) return false;
      neg = int(i);
      continue;
    }
    if (tgt[i] < 1 || tgt[i] > per_row) return false;
    rest *= tgt[i];
    if (rest > per_row) return false;
  }
  if (neg >= 0) {
    if (per_row % rest) return false;
    tgt[size_t(neg)] = per_row / rest;
    rest = per_row;
  }
  if (rest != per_row) return false;
  tgt[0] = in[0];
  *out = std::move(tgt);
  return true;
}

}  // namespace

void Lowerer::find_pixel_shuffles() {
  for (size_t i = 0; i < m.nodes.size(); i++) {
    const NodeDef &r = m.nodes[i];
    if (!graph->live[i] || absorbed[i] || region[i] || r.op != "Reshape" || !graph->std_dom(r) || r.inputs.size() != 2 || r.outputs.empty()) continue;
    const NodeDef *t = graph->sole_reader(r.outputs[0], false);
    if (!t || t->op != "Transpose" || !graph->std_dom(*t) || t->inputs.size() != 1 || t->outputs.empty()) continue;
    const auto *perm = t->attr_ints("perm");
    int form = -1;
    for (int k = 0; perm && k < 4; k++)
      if (*perm == kSpellings[k].perm) form = k;
    if (form < 0) continue;
    const NodeDef *l = graph->sole_reader(t->outputs[0], false);
    if (!l || l->op != "Reshape" || !graph->std_dom(*l) || l->inputs.size() != 2 || l->inputs[0] != t->outputs[0] || l->outputs.empty()) continue;
    const size_t ti = size_t(t - m.nodes.data()), li = size_t(l - m.nodes.data());
    if (absorbed[ti] || absorbed[li] || region[ti] || region[li] || ti <= i || li <= ti) continue;
    shuffle_at[li] = ShuffleMatch{i, ti, form};
    absorbed[i] = absorbed[ti] = 1;
  }
}

void Lowerer::check_shuffle_extents(const onnx::ValueDef &in) const {
  if (in.dims.size() != 4 || (in.dims[1] > 0 && in.dims[2] > 0 && in.dims[3] > 0)) return;
  auto it = graph->consumers_of.find(in.name);
  if (it == graph->consumers_of.end()) return;
  for (size_t i : it->second) {
    const NodeDef &n = m.nodes[i];
    if ((n.op == "DepthToSpace" || n.op == "SpaceToDepth") && graph->std_dom(n) && !n.inputs.empty() && n.inputs[0] == in.name)
      unsupported(n, "unsupported operator form: symbolic spatial extents: the input " + shape_str(in.dims) + " must have constant C, H and W");
  }
}

bool Lowerer::pixel_shuffle_spelling(const ShuffleMatch &sm, const NodeDef &last) {
  const NodeDef &first = m.nodes[sm.first], &tr = m.nodes[sm.transpose];
  const Spelling &sp = kSpellings[sm.form];
  const Val *xp = find_value(first.inputs[0]);
  if (!xp || xp->is_const || xp->pv || xp->q || xp->cl || xp->ra != 0 || xp->padded() || xp->buf < 0 || xp->shape.size() != 4) return false;
  const Val x = *xp;
  const int64_t C = x.shape[1], H = x.shape[2], W = x.shape[3];
  if (C < 1 || H < 1 || W < 1) return false;
  const Val *t1 = find_value(first.inputs[1]), *t2 = find_value(last.inputs[1]);
  if (!t1 || !t2 || !t1->is_const || !t2->is_const || t1->c->dtype != onnx::kInt64 || t2->c->dtype != onnx::kInt64 || t1->c->i64.size() != 6 || t2->c->i64.size() != 4)
    return false;
  std::vector<int64_t> d, tshape(6), out;
  if (!resolve_target(t1->c->i64, x.shape, &d)) return false;
  int64_t b;
  std::vector<int64_t> want;
  if (sp.to_space) {  // [N, b, b, C', H, W] or [N, C', b, b, H, W]
    const int64_t b0 = sp.channel_major ? d[2] : d[1], b1 = sp.channel_major ? d[3] : d[2], Cs = sp.channel_major ? d[1] : d[3];
    if (b0 != b1 || d[4] != H || d[5] != W || Cs * b0 * b0 != C) return false;
    b = b0;
    want = {x.shape[0], Cs, H * b, W * b};
  } else {  // [N, C, H/b, b, W/b, b]
    if (d[3] != d[5] || d[1] != C || d[2] * d[3] != H || d[4] * d[5] != W) return false;
    b = d[3];
    want = {x.shape[0], C * b * b, H / b, W / b};
  }
  for (size_t k = 0; k < 6; k++) tshape[k] = d[size_t(sp.perm[k])];
  if (!resolve_target(t2->c->i64, tshape, &out) || out != want) return false;
  pixel_shuffle_step(tr, last, x, b, sp.to_space, sp.channel_major, node_label(first) + "+" + node_label(tr) + "+" + node_label(last));
  if (x.half) mark_half(last.outputs[0]);
  return true;
}

// DepthToSpace (opsets 1, 11: mode, 13) and SpaceToDepth on an [N,C,H,W] activation
void Lowerer::depth_space(const NodeDef &n) {
  const bool to_space = n.op == "DepthToSpace";
  const Val a = get(n, 0);
  if (a.is_const) bad_form(n, "its input is a constant; only an activation is shuffled");
  if (a.shape.size() != 4) bad_form(n, "the input must be an [N,C,H,W] activation, got " + shape_str(a.shape));
  const int64_t b = n.attr_i("blocksize", 0);
  if (b < 1) bad_form(n, "blocksize = " + std::to_string(b) + " (it must be at least 1)");
  const std::string mode = to_space ? n.attr_s("mode", "DCR") : "DCR";
  if (mode != "DCR" && mode != "CRD") bad_form(n, "mode " + mode + " (only DCR and CRD)");
  pixel_shuffle_step(n, n, a, b, to_space, mode == "CRD", node_label(n));
}

void Lowerer::pixel_shuffle_step(const NodeDef &at, const NodeDef &out_node, const Val &a, int64_t b, bool to_space, bool channel_major, const std::string &origin) {
  const int64_t C = a.shape[1], H = a.shape[2], W = a.shape[3];
  if (C < 1 || H < 1 || W < 1) bad_form(at, "symbolic spatial extents: the input " + shape_str(a.shape) + " must have constant C, H and W");
  if (to_space ? (b > C || C % (b * b) != 0) : false)
    bad_form(at, "C = " + std::to_string(C) + " is not divisible by blocksize^2 = " + std::to_string(b) + "^2");
  if (!to_space && (H % b != 0 || W % b != 0))
    bad_form(at, "H x W = " + std::to_string(H) + " x " + std::to_string(W) + " is not divisible by blocksize = " + std::to_string(b));
  if (C > kPixelShuffleMaxC || (!to_space && b * b > kPixelShuffleMaxC / C))
    bad_form(at, "more than " + std::to_string(kPixelShuffleMaxC) + " channels (" + std::to_string(C) + " in, blocksize " + std::to_string(b) + ") are beyond the PixelShuffle kernel's cap");
  const int64_t OC = to_space ? C / (b * b) : C * b * b, OH = to_space ? H * b : H / b, OW = to_space ? W * b : W / b;
  if (H > kPixelShuffleMaxS / W || OH > kPixelShuffleMaxS / OW)
    bad_form(at, "a plane of more than 2^20 pixels (" + std::to_string(H) + " x " + std::to_string(W) + " -> " + std::to_string(OH) + " x " + std::to_string(OW) +
                     ") is beyond the PixelShuffle kernel's cap");
  if (b == 1) {  // the identity: the value keeps its buffer
    Val v = a;
    vals[out_node.outputs[0]] = v;
    buf_names[v.buf].push_back(out_node.outputs[0]);
    alias_edges[v.buf]++;
    return;
  }
  Step s;
  s.kind = StepKind::PixelShuffle;
  s.in0 = a.buf;
  s.ps_block = b;
  s.ps_to_space = to_space;
  s.ps_channel_major = channel_major;
  s.C = C, s.H = H, s.Wd = W, s.Mo = OC, s.OH = OH, s.OW = OW;
  s.origin = origin;
  const std::vector<int64_t> shape = {a.shape[0], OC, OH, OW};
  const bool whole = int_bufs.count(a.buf) > 0;
  const int out = push_step(std::move(s), shape);
  set_act(out_node, out, shape);
  if (whole) int_bufs.insert(out);
}

}  // namespace lowering

}  // namespace infera_hip
