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
  const std::string why = spectrum_refusal(p.n, p.C, p.frames, p.bins, p.mode == kSpectrumComplex);
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

void Lowerer::stft(const NodeDef &n) {
  if (n.inputs.size() < 2) bad_form(n, "signal and frame_step are required");
  const Val a = get(n, 0);
  spectrum_input(n, a, "the signal");
  if (a.shape.size() != 3) bad_form(n, "the signal must be a real [N, L, 1] value, got " + shape_str(a.shape));
  if (a.shape[2] == 2) bad_form(n, "a complex signal (last axis 2) is not supported; only real signals");
  if (a.shape[2] != 1) bad_form(n, "the signal must be a real [N, L, 1] value, got " + shape_str(a.shape));
  SpectrumPack p;
  p.stft = true;
  p.L = a.shape[1];
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
  const std::string why = spectrum_refusal(p.n, 1, 1, p.bins, true);  // (the length first: L < n below speaks of a served length)
  if (!why.empty()) bad_form(n, why);
  if (p.L < p.n) bad_form(n, "the signal has L = " + std::to_string(p.L) + " samples, fewer than a frame of " + std::to_string(p.n) + " (no frame)");
  p.frames = (p.L - p.n) / p.hop + 1;
  spectrum_step(n, a, std::move(p), {a.shape[0]});
}

}  // namespace lowering

}  // namespace infera_hip
