// lower_conv3d.cpp -- struct Lowerer (lowerer.hpp): Conv, MaxPool and AveragePool on rank-5 activations [N,C,D,H,W] (INTEGRATION.md 2.6
// "3-D convolutions").  conv() and pool() hand a rank-5 activation over; ranks 3 and 4 never come here.  A rank-5 value lies in its buffer in
// plain NCDHW element order and is registered with its own rank-5 shape: the scheduler's layout pass sees no [N,C,H,W] tensor in it, so the
// elementwise, residual and global-pool steps read it as the flat row it is, and a plan that holds one of these steps stays out of the
// channel-quad layout (hip/schedule.cpp).  The kernel that serves a Conv3d step is decided here from its geometry (host/conv3d.hpp).

#include "lowerer.hpp"

namespace infera_hip {

namespace lowering {

// strides, dilations, pads, auto_pad and ceil_mode of a 3-D node into `s` (kd, kh, kw, D, H, Wd are set): the checks of spatial(), on three axes
void Lowerer::spatial3d(const NodeDef &n, Step &s) {
  int64_t st[3] = {1, 1, 1}, dl[3] = {1, 1, 1}, p0[3] = {0, 0, 0}, p1[3] = {0, 0, 0};
  const int64_t in[3] = {s.D, s.H, s.Wd}, k[3] = {s.kd, s.kh, s.kw};
  auto three = [&](const char *name, int64_t *dst) {
    if (auto *p = n.attr_ints(name)) {
      if (p->size() != 3) bad_form(n, std::string(name) + " must have 3 entries on an [N,C,D,H,W] input, got " + std::to_string(p->size()));
      for (size_t i = 0; i < 3; i++) dst[i] = (*p)[i];
    }
  };
  three("strides", st);
  three("dilations", dl);
  if (auto *p = n.attr_ints("pads")) {
    if (p->size() != 6) bad_form(n, "pads must have 6 entries on an [N,C,D,H,W] input, got " + std::to_string(p->size()));
    for (size_t i = 0; i < 3; i++) p0[i] = (*p)[i], p1[i] = (*p)[i + 3];
  }
  // A model file is untrusted input (spatial()): nothing below may divide by zero, index backwards or leave int64
  const int64_t lim = int64_t(1) << 20;
  for (size_t i = 0; i < 3; i++) {
    if (st[i] < 1) bad_form(n, "strides must be >= 1");
    if (dl[i] < 1) bad_form(n, "dilations must be >= 1");
    if (k[i] < 1) bad_form(n, "kernel extents must be >= 1");
    if (p0[i] < 0 || p1[i] < 0) bad_form(n, "negative pads");
    if (st[i] > lim || dl[i] > lim || k[i] > lim || p0[i] > lim || p1[i] > lim || in[i] > lim) bad_form(n, "spatial attribute out of range");
  }
  const std::string ap = n.attr_s("auto_pad", "NOTSET");
  if (ap == "VALID") {
    for (size_t i = 0; i < 3; i++) p0[i] = p1[i] = 0;
  } else if (ap == "SAME_UPPER" || ap == "SAME_LOWER") {
    for (size_t i = 0; i < 3; i++) {
      const int64_t o = (in[i] + st[i] - 1) / st[i], p = std::max<int64_t>(0, (o - 1) * st[i] + (k[i] - 1) * dl[i] + 1 - in[i]);
      p0[i] = ap == "SAME_UPPER" ? p / 2 : p - p / 2;
      p1[i] = p - p0[i];
    }
  } else if (ap != "NOTSET") bad_form(n, "auto_pad " + ap);
  const bool ceil_mode = n.attr_i("ceil_mode", 0) != 0;
  int64_t out[3];
  for (size_t i = 0; i < 3; i++) {
    const int64_t num = in[i] + p0[i] + p1[i] - (dl[i] * (k[i] - 1) + 1);
    if (num < 0) bad_form(n, "empty spatial output");
    out[i] = (ceil_mode ? (num + st[i] - 1) / st[i] : num / st[i]) + 1;
    if (ceil_mode && (out[i] - 1) * st[i] >= in[i] + p0[i]) out[i]--;  // (a last window that starts beyond the input and its leading pad is dropped)
    if (out[i] <= 0) bad_form(n, "empty spatial output");
  }
  s.sd = st[0], s.sh = st[1], s.sw = st[2];
  s.dd = dl[0], s.dh = dl[1], s.dw = dl[2];
  s.pf = p0[0], s.pt = p0[1], s.pl = p0[2];
  s.pk = p1[0], s.pb = p1[1], s.pr = p1[2];
  s.OD = out[0], s.OH = out[1], s.OW = out[2];
}

void Lowerer::conv3d(const NodeDef &n) {
  const Val &a = get(n, 0);
  const Val &w = get(n, 1);
  if (cur_half || a.half || (w.is_const && w.c->elem == onnx::kFloat16)) bad_form(n, "a float16 convolution on an [N,C,D,H,W] input is not supported; export the model in float32");
  if (!w.is_const) bad_form(n, "the weights of a convolution on an [N,C,D,H,W] input must be a constant [M,C/g,kd,kh,kw] tensor");
  if (w.shape.size() != 5) bad_form(n, "the kernel " + shape_str(w.shape) + " does not have the rank of the input " + shape_str(a.shape));
  if (w.c->q_data) bad_form(n, "a quantised (QuantizeLinear / DequantizeLinear) convolution on an [N,C,D,H,W] input is not supported");
  if (auto *ks = n.attr_ints("kernel_shape"))
    if (ks->size() != 3 || (*ks)[0] != w.shape[2] || (*ks)[1] != w.shape[3] || (*ks)[2] != w.shape[4]) bad_form(n, "kernel_shape differs from the kernel " + shape_str(w.shape));
  Step s;
  s.kind = StepKind::Conv3d;
  s.in0 = a.buf;
  s.C = a.shape[1], s.D = a.shape[2], s.H = a.shape[3], s.Wd = a.shape[4];
  s.Mo = w.shape[0], s.kd = w.shape[2], s.kh = w.shape[3], s.kw = w.shape[4];
  s.groups = n.attr_i("group", 1);
  if (s.groups < 1 || s.Mo < 1 || w.shape[1] < 1 || s.C != w.shape[1] * s.groups || s.Mo % s.groups) bad_form(n, "channel/group mismatch");
  if (s.kd > kConv3dMaxKernel || s.kh > kConv3dMaxKernel || s.kw > kConv3dMaxKernel)
    bad_form(n, "a kernel extent above " + std::to_string(kConv3dMaxKernel) + " (" + shape_str(w.shape) + ")");
  spatial3d(n, s);
  const int64_t lim31 = int64_t(1) << 31;
  if (prod(a.shape, 1) >= lim31 || s.Mo * s.OD * s.OH * s.OW >= lim31) bad_form(n, "C*D*H*W or M*OD*OH*OW is 2^31 or more per image");
  s.K = (s.C / s.groups) * s.kd * s.kh * s.kw;
  s.M = s.Mo;
  s.W = cf32(n, w);
  if (has_input(n, 2)) {
    const Val &b = get(n, 2);
    if (!b.is_const || b.c->dtype != onnx::kFloat) bad_form(n, "B must be a constant f32 tensor");
    s.bias = b.c->f32;
    if (int64_t(s.bias.size()) != s.Mo) bad_form(n, "the bias has " + std::to_string(s.bias.size()) + " entries for M = " + std::to_string(s.Mo) + " output channels");
  }
  const ScheduleKnobs knobs = ScheduleKnobs::read();
  s.out_mode = knobs.conv3d_mfma ? conv3d_exec(conv3d_geom(s), knobs.conv3d_stage) : kConv3dGeneric;
  emit(std::move(s), n, {a.shape[0], s.Mo, s.OD, s.OH, s.OW});
}

void Lowerer::pool3d(const NodeDef &n, bool is_max) {
  const Val &a = get(n, 0);
  if (cur_half || a.half) bad_form(n, "float16 pooling on an [N,C,D,H,W] input is not supported; export the model in float32");
  auto *ks = n.attr_ints("kernel_shape");
  if (!ks || ks->size() != 3) bad_form(n, "kernel_shape must have 3 entries on an [N,C,D,H,W] input");
  if (n.outputs.size() > 1 && !n.outputs[1].empty() && uses.count(n.outputs[1]) && uses[n.outputs[1]] > 0) bad_form(n, "the Indices output is not served");
  Step s;
  s.kind = StepKind::Pool3d;
  s.in0 = a.buf;
  s.is_max = is_max;
  s.count_pad = n.attr_i("count_include_pad", 0) != 0;
  if (!is_max && s.count_pad && n.attr_i("ceil_mode", 0) != 0) bad_form(n, "ceil_mode=1 with count_include_pad=1");
  s.C = s.Mo = a.shape[1], s.D = a.shape[2], s.H = a.shape[3], s.Wd = a.shape[4];
  s.kd = (*ks)[0], s.kh = (*ks)[1], s.kw = (*ks)[2];
  if (s.kd > kConv3dMaxKernel || s.kh > kConv3dMaxKernel || s.kw > kConv3dMaxKernel) bad_form(n, "a kernel extent above " + std::to_string(kConv3dMaxKernel));
  spatial3d(n, s);
  if (prod(a.shape, 1) >= (int64_t(1) << 31)) bad_form(n, "C*D*H*W is 2^31 or more per image");
  emit(std::move(s), n, {a.shape[0], s.C, s.OD, s.OH, s.OW});
}

}  // namespace lowering

}  // namespace infera_hip
