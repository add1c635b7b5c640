// lower_spectrum.cpp -- the ONNX DFT and STFT operators on real signals as one Spectrum step (INTEGRATION.md 2.6 "Spectral front ends",
// host/spectrum.hpp, hip/spectrum.hip).  The magnitude and the layout nodes that alone read the transform are absorbed into the step.
#include "lowerer.hpp"
#include "spectrum.hpp"

namespace infera_hip {

namespace lowering {

namespace {

// the one integer of a constant input; refusals name the input
int64_t one_int(Lowerer &lw, const NodeDef &n, size_t i, const char *what) {
  const Val &v = lw.get(n, i);
  if (!v.is_const) lw.bad_form(n, std::string(what) + " is not a constant");
  if (v.c->dtype != onnx::kInt64 || v.c->i64.size() != 1) lw.bad_form(n, std::string(what) + " must be one constant integer");
  return v.c->i64[0];
}

}  // namespace

// The nodes behind the transform `n` that the step stands for: [Transpose(0,2,1,3)] -> the magnitude (ReduceSumSquare | ReduceL2 | Pow(., 2) ->
// ReduceSum [-> Sqrt], over the last axis) -> [Transpose(0,2,1 [,3])], each the only reader of the one before.  Sets the pack's mode and
// layout, marks the nodes absorbed and returns the last of them (n itself: none); *keep: the magnitude kept its trailing axis
const NodeDef *Lowerer::spectrum_tail(const NodeDef &n, bool stft, SpectrumPack &p, bool *keep) {
  const NodeDef *last = &n;
  std::vector<const NodeDef *> taken;
  auto reader = [&](const NodeDef *of) { return graph->sole_reader(of->outputs[0], false); };
  auto transpose_of = [&](const NodeDef *t, size_t rank) {
    if (!t || t->op != "Transpose" || !GraphIndex::std_dom(*t)) return false;
    const std::vector<int64_t> *perm = t->attr_ints("perm");
    const std::vector<int64_t> want = rank == 4 ? std::vector<int64_t>{0, 2, 1, 3} : std::vector<int64_t>{0, 2, 1};
    return perm && *perm == want;
  };
  auto last_axis = [&](const NodeDef &r, int64_t rank) {
    std::vector<int64_t> axes;
    return graph_ints_arg(r, 1, "axes", &axes) && axes.size() == 1 && (axes[0] == -1 || axes[0] == rank - 1) && r.attr_i("noop_with_empty_axes", 0) == 0;
  };
  const int64_t rank = stft ? 4 : (p.C > 1 || p.rank4 ? 4 : 3);
  const NodeDef *r = reader(last);
  if (stft && transpose_of(r, 4)) p.bins_major = true, taken.push_back(r), last = r, r = reader(last);
  *keep = false;
  if (r && GraphIndex::std_dom(*r) && (r->op == "ReduceSumSquare" || r->op == "ReduceL2") && last_axis(*r, rank)) {
    p.mode = r->op == "ReduceL2" ? kSpectrumMagnitude : kSpectrumPower;
    *keep = r->attr_i("keepdims", 1) != 0;
    taken.push_back(r), last = r;
  } else if (r && GraphIndex::std_dom(*r) && r->op == "Pow" && r->inputs.size() == 2 && r->inputs[0] == last->outputs[0]) {
    double e = 0;
    size_t cnt = 0;
    const NodeDef *sum = reader(r);
    if (graph_const_scalar(r->inputs[1], &e, &cnt) && cnt == 1 && e == 2.0 && sum && GraphIndex::std_dom(*sum) && sum->op == "ReduceSum" && last_axis(*sum, rank)) {
      p.mode = kSpectrumPower;
      *keep = sum->attr_i("keepdims", 1) != 0;
      taken.push_back(r), taken.push_back(sum), last = sum;
      if (const NodeDef *sq = reader(sum); sq && GraphIndex::std_dom(*sq) && sq->op == "Sqrt") p.mode = kSpectrumMagnitude, taken.push_back(sq), last = sq;
    }
  }
  if (stft && !p.bins_major && p.mode != kSpectrumComplex)
    if (const NodeDef *t = reader(last); transpose_of(t, *keep ? 4 : 3)) p.bins_major = true, taken.push_back(t), last = t;
  for (const NodeDef *t : taken) {
    size_t idx = 0;
    graph->producer(t->outputs[0], &idx);
    absorbed[idx] = 1;
  }
  return last;
}

// ONE Spectrum step over the signals of `a`, bound to the last absorbed node's output
void Lowerer::spectrum_step(const NodeDef &n, const Val &a, SpectrumPack p, const std::vector<int64_t> &lead) {
  bool keep = false;
  const NodeDef *last = spectrum_tail(n, p.stft, p, &keep);
  const std::string why = spectrum_refusal(p.stft, p.n, p.C, p.frames, p.bins, p.mode == kSpectrumComplex);
  if (!why.empty()) bad_form(n, why);
  pack_spectrum(p);
  std::vector<int64_t> shape = lead;  // [N (, C)]
  if (p.stft) shape.push_back(p.bins_major ? p.bins : p.frames), shape.push_back(p.bins_major ? p.frames : p.bins);
  else shape.push_back(p.bins);
  if (p.mode == kSpectrumComplex) shape.push_back(2);
  else if (keep) shape.push_back(1);
  Step s;
  s.kind = StepKind::Spectrum;
  s.in0 = a.buf;
  s.out_mode = p.mode;
  s.origin = node_label(n) + (last != &n ? "+...+" + node_label(*last) : "");
  s.spectrum = std::make_shared<const SpectrumPack>(std::move(p));
  set_act(*last, push_step(std::move(s), flat_shape(shape)), shape);
}

void Lowerer::spectrum_input(const NodeDef &n, const Val &a, const char *what) {
  if (a.is_const) bad_form(n, std::string(what) + " is a constant; only activations");
  if (a.ra != 0) bad_form(n, std::string(what) + " " + shape_str(a.shape) + " is time-major (its row axis is axis " + std::to_string(a.ra) + "); only rows-first signals");
  if (a.half || cur_half) bad_form(n, "float16 operands are not supported; cast the signal to float in front of it");
  if (a.q) bad_form(n, "quantised operands are not supported");
  if (a.cl || a.pv || a.nn || a.buf < 0) bad_form(n, std::string(what) + " is not a rows-first f32 activation");
}

void Lowerer::dft(const NodeDef &n) {
  const Val a = get(n, 0);
  spectrum_input(n, a, "the input");
  if (n.attr_i("inverse", 0) != 0) bad_form(n, "inverse = 1 (the inverse transform is not supported)");
  const int64_t rank = int64_t(a.shape.size());
  if (rank != 3 && rank != 4) bad_form(n, "the input must be a real [N, L, 1] or [N, C, L, 1] signal, got " + shape_str(a.shape));
  if (a.shape.back() == 2) bad_form(n, "a complex input (last axis 2) is not supported; only real signals");
  if (a.shape.back() != 1) bad_form(n, "the input must be a real [N, L, 1] or [N, C, L, 1] signal, got " + shape_str(a.shape));
  int64_t axis = plan.opset >= 20 ? -2 : 1;
  if (has_input(n, 2)) axis = one_int(*this, n, 2, "axis");
  else if (n.attr("axis")) axis = n.attr_i("axis", axis);
  if (axis < 0) axis += rank;
  if (axis != rank - 2) bad_form(n, "axis = " + std::to_string(axis) + " of " + shape_str(a.shape) + "; only the second to last axis is transformed");
  SpectrumPack p;
  p.stft = false;
  p.rank4 = rank == 4;
  p.C = rank == 4 ? a.shape[1] : 1;
  p.L = a.shape[size_t(rank - 2)];
  p.n = has_input(n, 1) ? one_int(*this, n, 1, "dft_length") : p.L;
  p.onesided = n.attr_i("onesided", 0) != 0;
  p.hop = p.n, p.frames = 1;
  p.bins = p.onesided ? p.n / 2 + 1 : p.n;
  spectrum_step(n, a, std::move(p), rank == 4 ? std::vector<int64_t>{a.shape[0], a.shape[1]} : std::vector<int64_t>{a.shape[0]});
}

bool Lowerer::pad_signal(const NodeDef &n) {
  const Val a = get(n, 0);
  const int64_t rank = int64_t(a.shape.size());
  if (a.is_const || rank == 4) return false;
  const std::string only = "only the time axis of a rows-first f32 signal [N, L], [N, 1, L] or [1, N, L] in front of an STFT (and [N,C,H,W] in front of a Conv)";
  if (a.half || cur_half) bad_form(n, "float16 operands are not supported; cast the signal to float in front of it");
  if (a.q) bad_form(n, "quantised operands are not supported");
  if (a.cl || a.pv || a.nn || a.buf < 0 || a.padded()) bad_form(n, "its data is not a rows-first f32 activation; " + only);
  const bool lead1 = rank == 3 && a.ra == 1 && a.shape[0] == 1;  // [1, N, L]
  if (!(rank == 2 && a.ra == 0) && !(rank == 3 && a.ra == 0 && a.shape[1] == 1) && !lead1) bad_form(n, "its data is " + shape_str(a.shape) + " (row axis " + std::to_string(a.ra) + "); " + only);
  const int64_t L = a.shape.back();
  const std::string mode = n.attr_s("mode", "constant");
  if (mode != "constant" && mode != "reflect") bad_form(n, "mode = \"" + mode + "\" (only reflect and constant zero padding are absorbed into an STFT)");
  std::vector<int64_t> pads, axes;
  if (has_input(n, 1)) {
    if (!graph_ints_arg(n, 1, "pads", &pads)) bad_form(n, "pads is not a constant");
  } else if (auto *pp = n.attr_ints("pads")) pads = *pp;
  if (has_input(n, 3) && !graph_ints_arg(n, 3, "axes", &axes)) bad_form(n, "axes is not a constant");
  if (axes.empty())
    for (int64_t i = 0; i < rank; i++) axes.push_back(i);
  if (pads.size() != 2 * axes.size()) bad_form(n, "pads must hold " + std::to_string(2 * axes.size()) + " entries, got " + std::to_string(pads.size()));
  int64_t left = 0, right = 0;
  for (size_t i = 0; i < axes.size(); i++) {
    const int64_t ax = axes[i] < 0 ? axes[i] + rank : axes[i], lo = pads[i], hi = pads[i + axes.size()];
    if (lo < 0 || hi < 0) bad_form(n, "negative pads (cropping)");
    if (ax == rank - 1) left += lo, right += hi;
    else if (lo || hi) bad_form(n, "pads on axis " + std::to_string(ax) + " of " + shape_str(a.shape) + "; only the time axis (the last) is padded");
  }
  double value = double(n.attr_f("value", 0.f));
  size_t cnt = 1;
  if (has_input(n, 2) && (!graph_const_scalar(n.inputs[2], &value, &cnt) || cnt != 1)) bad_form(n, "constant_value is not one constant");
  if (mode == "constant" && value != 0.0) bad_form(n, "a constant_value of " + std::to_string(value) + " (only zero padding is absorbed into an STFT)");
  if (mode == "reflect" && (left >= L || right >= L)) bad_form(n, "reflect pads (" + std::to_string(left) + ", " + std::to_string(right) + ") reach beyond a signal of L = " + std::to_string(L) + " samples (at most L - 1)");
  // the readers up to the STFT: the shape holds only the rows (-1), the padded length and 1s, so these nodes move nothing
  std::vector<int64_t> shape(size_t(rank), 1);
  shape[size_t(a.ra)] = -1, shape.back() = L + left + right;
  std::vector<const NodeDef *> chain;
  const NodeDef *r = graph->sole_reader(n.outputs[0], false);
  for (; r && GraphIndex::std_dom(*r) && (r->op == "Reshape" || r->op == "Squeeze" || r->op == "Unsqueeze"); r = graph->sole_reader(r->outputs[0], false)) {
    if (r->inputs.empty() || r->inputs[0] != (chain.empty() ? n : *chain.back()).outputs[0]) break;  // (it reads the signal as a shape operand)
    std::vector<int64_t> arg, out;
    if (!graph_ints_arg(*r, 1, r->op == "Reshape" ? "shape" : "axes", &arg)) bad_form(n, "its reader '" + r->name + "' (" + r->op + ") has no constant " + (r->op == "Reshape" ? "shape" : "axes"));
    const int64_t cur = int64_t(shape.size());
    if (r->op == "Reshape") {
      // the entries that are not 1 must be the rows (-1, 0 or the fixed batch) and then the padded length
      std::vector<int64_t> big;
      for (int64_t v : arg)
        if (v != 1) big.push_back(v);
      const int64_t rows = a.shape[size_t(a.ra)];
      if (big.size() != 2 || (big[0] != -1 && big[0] != 0 && big[0] != rows) || big[1] != L + left + right)
        bad_form(n, "its reader '" + r->name + "' reshapes the padded signal to " + shape_str(arg) + "; only [rows, L'] with axes of extent 1 around them");
      bool seen = false;
      for (int64_t v : arg) out.push_back(v == 1 ? 1 : seen ? v : (seen = true, -1));
    } else if (r->op == "Squeeze") {
      for (int64_t i = 0; i < cur; i++) {
        bool drop = arg.empty() && shape[size_t(i)] == 1;
        for (int64_t ax : arg) drop = drop || (ax < 0 ? ax + cur : ax) == i;
        if (drop && shape[size_t(i)] != 1) bad_form(n, "its reader '" + r->name + "' squeezes an axis of the padded signal that is not 1");
        if (!drop) out.push_back(shape[size_t(i)]);
      }
    } else {
      const int64_t nr = cur + int64_t(arg.size());
      size_t src = 0;
      for (int64_t i = 0; i < nr; i++) {
        bool ins = false;
        for (int64_t ax : arg) ins = ins || (ax < 0 ? ax + nr : ax) == i;
        if (!ins && src >= shape.size()) bad_form(n, "its reader '" + r->name + "' has axes out of range");
        out.push_back(ins ? 1 : shape[src++]);
      }
    }
    shape = out;
    chain.push_back(r);
  }
  if (!r || !GraphIndex::std_dom(*r) || r->op != "STFT" || r->inputs.empty() || r->inputs[0] != (chain.empty() ? n : *chain.back()).outputs[0])
    bad_form(n, "the output of a Pad node can only feed a Conv, or -- the time axis of a signal -- one STFT through Reshape / Squeeze / Unsqueeze nodes" +
                    (r ? "; it reaches '" + r->name + "' (" + r->op + ")" : std::string("; it has several readers or is a model output")));
  const bool r2 = shape == std::vector<int64_t>{-1, L + left + right}, r3 = shape == std::vector<int64_t>{-1, L + left + right, 1};
  if (!r2 && !r3) bad_form(n, "the padded signal reaches '" + r->name + "' (STFT) as " + shape_str(shape) + " (-1: the rows); only [N, L'] or [N, L', 1]");
  for (const NodeDef *c : chain) {
    size_t idx = 0;
    graph->producer(c->outputs[0], &idx);
    absorbed[idx] = 1;
  }
  TimePad tp;
  tp.src = a, tp.left = left, tp.right = right, tp.mode = mode == "reflect" ? kSpectrumPadReflect : kSpectrumPadConstant;
  shape[0] = a.shape[size_t(a.ra)];
  tp.shape = shape;
  time_pads[r->inputs[0]] = tp;
  return true;
}

void Lowerer::stft(const NodeDef &n) {
  if (n.inputs.size() < 2) bad_form(n, "signal and frame_step are required");
  const auto tp = time_pads.find(n.inputs[0]);
  Val a = tp != time_pads.end() ? tp->second.src : get(n, 0);
  SpectrumPack p;
  if (tp != time_pads.end()) {  // (pad_signal has checked the operand; the shape is the padded signal's as this node reads it)
    p.pad_left = tp->second.left, p.pad_right = tp->second.right, p.pad_mode = tp->second.mode;
    a.shape = tp->second.shape, a.ra = 0;
  }
  spectrum_input(n, a, "the signal");
  if (a.shape.size() == 2) a.shape.push_back(1);  // (torch's exporter passes the rank-2 [N, L] signal)
  if (a.shape.size() != 3) bad_form(n, "the signal must be a real [N, L, 1] value, got " + shape_str(a.shape));
  if (a.shape[2] == 2) bad_form(n, "a complex signal (last axis 2) is not supported; only real signals");
  if (a.shape[2] != 1) bad_form(n, "the signal must be a real [N, L, 1] value, got " + shape_str(a.shape));
  p.stft = true;
  p.L = a.shape[1] - p.pad_left - p.pad_right;
  p.hop = one_int(*this, n, 1, "frame_step");
  if (p.hop < 1) bad_form(n, "frame_step = " + std::to_string(p.hop) + " must be at least 1");
  if (has_input(n, 2)) {
    const Val &w = get(n, 2);
    if (!w.is_const) bad_form(n, "window is not a constant");
    if (w.c->dtype != onnx::kFloat || w.c->elem == onnx::kFloat16) bad_form(n, "window must be a constant f32 [n] tensor (float16 operands are not supported)");
    if (w.shape.size() != 1) bad_form(n, "window must be a constant f32 [n] tensor, got " + shape_str(w.shape));
    p.window = w.c->f32;
    p.n = int64_t(p.window.size());
  }
  if (has_input(n, 3)) {
    const int64_t fl = one_int(*this, n, 3, "frame_length");
    if (!p.window.empty() && fl != p.n) bad_form(n, "the window has " + std::to_string(p.n) + " values, frame_length is " + std::to_string(fl));
    p.n = fl;
  }
  if (p.n == 0) bad_form(n, "neither window nor frame_length is given");
  p.onesided = n.attr_i("onesided", 1) != 0;
  p.bins = p.onesided ? p.n / 2 + 1 : p.n;
  const std::string why = spectrum_refusal(true, p.n, 1, 1, p.bins, true);  // (the length first: L < n below speaks of a served length)
  if (!why.empty()) bad_form(n, why);
  if (p.padded() < p.n) bad_form(n, "the signal has L = " + std::to_string(p.padded()) + " samples, fewer than a frame of " + std::to_string(p.n) + " (no frame)");
  p.frames = (p.padded() - p.n) / p.hop + 1;
  spectrum_step(n, a, std::move(p), {a.shape[0]});
}

}  // namespace lowering

}  // namespace infera_hip
