// lower_deformconv.cpp -- struct Lowerer (lowerer.hpp): DeformConv (opsets 19, 22; torchvision.ops.deform_conv2d) on [N,C,H,W] activations
// (INTEGRATION.md 2.6 "Deformable convolutions").  One DeformConv2d step per node: in0 = X, in1 = the offsets, in2 = the mask (-1: DCNv1).
// The weights and the bias are constants; X, the offsets and the mask are activations -- inputs of the call reshaped in the graph, or tensors a
// step wrote (the offset and mask convolutions of a DCN block).  A BatchNormalization behind the node folds into it and the fusable activations
// go into its epilogue, as for Conv (batchnorm(), apply_unary()).  The kernel and the layouts are the scheduler's decision (hip/schedule.cpp).

#include "deformconv.hpp"
#include "lowerer.hpp"

namespace infera_hip {

namespace lowering {

void Lowerer::check_deform_extents() const {
  for (size_t i = 0; i < m.nodes.size(); i++) {
    const NodeDef &n = m.nodes[i];
    if (!graph->live[i] || n.op != "DeformConv" || !graph->std_dom(n) || n.inputs.empty()) continue;
    for (const auto &in : m.inputs)
      if (in.name == n.inputs[0] && in.has_shape && in.dims.size() == 4 && (in.dims[1] <= 0 || in.dims[2] <= 0 || in.dims[3] <= 0))
        unsupported(n, "unsupported operator form: symbolic spatial extents: the input '" + in.name + "' " + shape_str(in.dims) + " must have constant extents behind the batch axis");
  }
}

void Lowerer::deform_conv(const NodeDef &n) {
  const Val x = get(n, 0);
  const Val w = get(n, 1);
  const Val off = get(n, 2);
  const bool has_mask = has_input(n, 4);
  if (cur_half || x.half || (w.is_const && w.c->elem == onnx::kFloat16)) bad_form(n, "a float16 deformable convolution is not served; export the model in float32");
  if (!w.is_const || w.c->dtype != onnx::kFloat) bad_form(n, "W must be a constant f32 tensor [M,C/group,kh,kw]");
  if (w.c->q_data) bad_form(n, "a quantised (QuantizeLinear / DequantizeLinear) deformable convolution is not served");
  if (x.is_const) bad_form(n, "its input X is a constant; only an activation is convolved");
  if (off.is_const) bad_form(n, "its offset is a constant; only an activation [N,og*kh*kw*2,OH,OW] is served");
  if (x.shape.size() != 4 || w.shape.size() != 4 || off.shape.size() != 4)
    bad_form(n, "only rank 4 is served: X " + shape_str(x.shape) + ", W " + shape_str(w.shape) + ", offset " + shape_str(off.shape));
  auto plain = [](const Val &v) { return !v.cl && v.ra == 0 && !v.padded() && v.buf >= 0; };
  if (!plain(x) || !plain(off)) bad_form(n, "X and offset must be plain [N,C,H,W] activations (no channels-last view, no pending Pad)");

  Step s;
  s.kind = StepKind::DeformConv2d;
  s.in0 = x.buf, s.in1 = off.buf;
  s.C = x.shape[1], s.H = x.shape[2], s.Wd = x.shape[3];
  s.Mo = w.shape[0], s.kh = w.shape[2], s.kw = w.shape[3];
  if (s.C < 1 || s.H < 1 || s.Wd < 1) bad_form(n, "symbolic spatial extents: the input " + shape_str(x.shape) + " must have constant C, H and W");
  if (auto *ks = n.attr_ints("kernel_shape"))
    if (ks->size() != 2 || (*ks)[0] != s.kh || (*ks)[1] != s.kw) bad_form(n, "kernel_shape differs from the kernel " + shape_str(w.shape));
  if (s.kh > kDeformMaxKernel || s.kw > kDeformMaxKernel) bad_form(n, "a kernel extent above " + std::to_string(kDeformMaxKernel) + " (" + shape_str(w.shape) + ")");
  s.groups = n.attr_i("group", 1);
  s.offset_groups = n.attr_i("offset_group", 1);
  if (s.groups < 1 || s.Mo < 1 || w.shape[1] < 1 || s.C % s.groups || s.Mo % s.groups || s.C != w.shape[1] * s.groups)
    bad_form(n, "group = " + std::to_string(s.groups) + " does not divide C = " + std::to_string(s.C) + " and M = " + std::to_string(s.Mo) + " into the kernel " + shape_str(w.shape));
  if (s.offset_groups < 1 || s.C % s.offset_groups) bad_form(n, "offset_group = " + std::to_string(s.offset_groups) + " does not divide C = " + std::to_string(s.C));

  // strides, pads, dilations: untrusted input, as in spatial3d -- extents >= 1, pads >= 0, everything <= 2^20
  int64_t st[2] = {1, 1}, dl[2] = {1, 1}, pads[4] = {0, 0, 0, 0};
  auto ints = [&](const char *name, int64_t *dst, size_t count) {
    if (auto *p = n.attr_ints(name)) {
      if (p->size() != count) bad_form(n, std::string(name) + " must have " + std::to_string(count) + " entries on an [N,C,H,W] input, got " + std::to_string(p->size()));
      for (size_t i = 0; i < count; i++) dst[i] = (*p)[i];
    }
  };
  ints("strides", st, 2);
  ints("dilations", dl, 2);
  ints("pads", pads, 4);
  const int64_t lim = int64_t(1) << 20, in[2] = {s.H, s.Wd}, k[2] = {s.kh, s.kw};
  int64_t out[2];
  for (size_t i = 0; i < 2; i++) {
    if (st[i] < 1) bad_form(n, "strides must be >= 1");
    if (dl[i] < 1) bad_form(n, "dilations must be >= 1");
    if (k[i] < 1) bad_form(n, "kernel extents must be >= 1");
    if (pads[i] < 0 || pads[i + 2] < 0) bad_form(n, "negative pads");
    if (st[i] > lim || dl[i] > lim || pads[i] > lim || pads[i + 2] > lim || in[i] > lim) bad_form(n, "spatial attribute out of range");
    const int64_t num = in[i] + pads[i] + pads[i + 2] - (dl[i] * (k[i] - 1) + 1);
    if (num < 0) bad_form(n, "empty spatial output");
    out[i] = num / st[i] + 1;
  }
  s.sh = st[0], s.sw = st[1], s.dh = dl[0], s.dw = dl[1];
  s.pt = pads[0], s.pl = pads[1], s.pb = pads[2], s.pr = pads[3];
  s.OH = out[0], s.OW = out[1];

  const int64_t taps = s.kh * s.kw;
  auto operand = [&](const Val &v, const char *what, int64_t per_tap) {
    const int64_t want = s.offset_groups * taps * per_tap;
    if (v.shape[2] < 1 || v.shape[3] < 1) bad_form(n, std::string("symbolic spatial extents: the ") + what + " " + shape_str(v.shape) + " must have constant OH and OW");
    if (v.shape[1] != want || v.shape[2] != s.OH || v.shape[3] != s.OW || v.shape[0] != x.shape[0])
      bad_form(n, std::string("its ") + what + " " + shape_str(v.shape) + " disagrees with [N," + std::to_string(want) + "," + std::to_string(s.OH) + "," + std::to_string(s.OW) + "] (offset_group * kh * kw" +
                      (per_tap == 2 ? " * 2" : "") + " channels on the output's extents)");
  };
  operand(off, "offset", 2);
  if (has_mask) {
    const Val mk = get(n, 4);
    if (mk.is_const) bad_form(n, "its mask is a constant; only an activation [N,og*kh*kw,OH,OW] is served");
    if (mk.shape.size() != 4) bad_form(n, "only rank 4 is served: mask " + shape_str(mk.shape));
    if (!plain(mk)) bad_form(n, "the mask must be a plain [N,C,H,W] activation");
    operand(mk, "mask", 1);
    s.in2 = mk.buf;
  }
  const int64_t lim31 = int64_t(1) << 31;
  if (s.C * s.H * s.Wd >= lim31 || s.Mo * s.OH * s.OW >= lim31 || s.offset_groups * taps * 2 * s.OH * s.OW >= lim31)
    bad_form(n, "C*H*W, M*OH*OW or the offset tensor is 2^31 elements or more per image");
  s.K = (s.C / s.groups) * taps;
  s.M = s.Mo;
  s.W = w.c->f32;
  if (has_input(n, 3)) {
    const Val &b = get(n, 3);
    if (!b.is_const || b.c->dtype != onnx::kFloat) bad_form(n, "B must be a constant f32 tensor");
    s.bias = b.c->f32;
    if (int64_t(s.bias.size()) != s.Mo) bad_form(n, "the bias has " + std::to_string(s.bias.size()) + " entries for M = " + std::to_string(s.Mo) + " output channels");
  }
  emit(std::move(s), n, {x.shape[0], s.Mo, s.OH, s.OW});
}

}  // namespace lowering

}  // namespace infera_hip
