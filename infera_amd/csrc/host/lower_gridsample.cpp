// lower_gridsample.cpp -- struct Lowerer (lowerer.hpp): GridSample (opsets 16, 20, 22) and AffineGrid (opset 20) on [N,C,H,W] activations
// (INTEGRATION.md 2.6 "Grid sampling").  One GridSample step per node, whatever its coordinates come from (host/gridsample.hpp):
//   grid     input 1 is an [N,Ho,Wo,2] activation -- a second graph input, or a step's result.  The step reads its buffer as the flat row it is.
//   planar   input 1 is the channels-last view (Val::cl) of an [N,2,Ho,Wo] tensor a step wrote: a flow field.  The Transpose moved nothing and
//            the step reads the two planes.
//   affine   input 1 is the result of an AffineGrid that nothing else reads: the AffineGrid emits nothing (affine_pending), the step reads the
//            six numbers of each image and the grid is never written.
// An AffineGrid with any other reader becomes an AffineGrid step that writes the grid into a flat buffer, and its readers take the grid form.
// The step reads and writes whichever layout the scheduler gives X and Y; the grid, the flow field and theta are never channel-quad tensors.

#include "gridsample.hpp"
#include "lowerer.hpp"

namespace infera_hip {

namespace lowering {

void Lowerer::check_grid_extents() const {
  auto input_named = [&](const std::string &v) -> const onnx::ValueDef * {
    for (const auto &in : m.inputs)
      if (in.name == v && in.has_shape && in.dims.size() == 4) return &in;
    return nullptr;
  };
  for (size_t i = 0; i < m.nodes.size(); i++) {
    const NodeDef &n = m.nodes[i];
    if (!graph->live[i] || n.op != "GridSample" || !graph->std_dom(n) || n.inputs.size() != 2) continue;
    const onnx::ValueDef *x = input_named(n.inputs[0]), *g = input_named(n.inputs[1]);
    for (const onnx::ValueDef *in : {x, g})
      if (in && (in->dims[1] <= 0 || in->dims[2] <= 0 || in->dims[3] <= 0))
        unsupported(n, "unsupported operator form: symbolic spatial extents: the input '" + in->name + "' " + shape_str(in->dims) + " must have constant extents behind the batch axis");
    // (inside the walk every activation has the model's batch; two inputs of the graph are the one place where the extents can differ)
    if (x && g && x->dims[0] > 0 && g->dims[0] > 0 && x->dims[0] != g->dims[0])
      unsupported(n, "unsupported operator form: its grid's N disagrees: grid " + shape_str(g->dims) + " against X " + shape_str(x->dims));
  }
}

// AffineGrid(theta [N,2,3], size): nothing is emitted where one GridSample alone reads the grid (it computes the coordinates itself)
void Lowerer::affine_grid(const NodeDef &n) {
  const Val th = get(n, 0);
  const Val &sz = get(n, 1);
  if (!sz.is_const || sz.c->dtype != onnx::kInt64) bad_form(n, "its size is not a constant (only a constant [N,C,H,W] size is served)");
  if (sz.c->i64.size() == 5) bad_form(n, "a 3-D size " + shape_str(sz.c->i64) + " (volumetric grids are not served)");
  if (sz.c->i64.size() != 4) bad_form(n, "size must have four entries [N,C,H,W], got " + std::to_string(sz.c->i64.size()));
  if (th.is_const) bad_form(n, "theta is a constant; only an activation [N,2,3] is served");
  const bool flat6 = th.shape.size() == 2 && th.shape[1] == 6, mat = th.shape.size() == 3 && th.shape[1] == 2 && th.shape[2] == 3;
  if (th.cl || th.ra != 0 || th.padded() || th.buf < 0 || !(flat6 || mat)) bad_form(n, "theta must be an [N,2,3] (or [N,6]) activation, got " + shape_str(th.shape));
  const int64_t OH = sz.c->i64[2], OW = sz.c->i64[3];
  if (OH < 1 || OW < 1) bad_form(n, "symbolic spatial extents: the size " + shape_str(sz.c->i64) + " must have constant H and W");
  if (OH > kGridSampleMaxPlane / OW || OH * OW >= kGridSampleMaxPlane) bad_form(n, "a grid of " + std::to_string(OH) + " x " + std::to_string(OW) + " positions (2^31 or more)");
  AffinePending ap{th, OH, OW, n.attr_i("align_corners", 0) != 0, node_label(n)};
  const NodeDef *r = graph->sole_reader(n.outputs[0], false);
  // (a reader with the other align_corners convention is served too: the grid is written by this node's rule and read by the reader's)
  if (r && r->op == "GridSample" && graph->std_dom(*r) && r->inputs.size() == 2 && r->inputs[1] == n.outputs[0] && r->inputs[0] != n.outputs[0] &&
      (r->attr_i("align_corners", 0) != 0) == ap.align) {
    affine_pending[n.outputs[0]] = std::move(ap);
    return;
  }
  Step s;
  s.kind = StepKind::AffineGrid;
  s.in0 = th.buf;
  s.OH = OH, s.OW = OW;
  s.gs_align = ap.align;
  s.origin = ap.origin;
  // (the buffer is registered as the flat row it is: a grid is no [N,C,H,W] image to the layout rules; the value carries the 4-D shape)
  const std::vector<int64_t> shape = {th.shape[0], OH, OW, 2};
  set_act(n, push_step(std::move(s), flat_shape(shape)), shape);
}

void Lowerer::grid_sample(const NodeDef &n) {
  const std::string mode = n.attr_s("mode", m.opset >= 20 ? "linear" : "bilinear");
  if (mode == "cubic" || mode == "bicubic") bad_form(n, "mode " + mode + " (only linear / bilinear and nearest are served)");
  if (mode != "linear" && mode != "bilinear" && mode != "nearest") bad_form(n, "mode " + mode);
  const std::string padding = n.attr_s("padding_mode", "zeros");
  if (padding != "zeros" && padding != "border" && padding != "reflection") bad_form(n, "padding_mode " + padding);
  const Val x = get(n, 0);
  if (x.is_const) bad_form(n, "its input X is a constant; only an activation is sampled");
  if (x.shape.size() == 5) bad_form(n, "a 5-D input " + shape_str(x.shape) + " (volumetric sampling is not served)");
  if (x.cl) bad_form(n, "its input X '" + n.inputs[0] + "' is a channels-last view; only the grid is read through one");
  if (x.shape.size() != 4 || x.padded() || x.buf < 0) bad_form(n, "the input X must be an [N,C,H,W] activation, got " + shape_str(x.shape));
  const int64_t C = x.shape[1], H = x.shape[2], W = x.shape[3];
  if (C < 1 || H < 1 || W < 1) bad_form(n, "symbolic spatial extents: the input " + shape_str(x.shape) + " must have constant C, H and W");
  if (H > kGridSampleMaxExtent || W > kGridSampleMaxExtent)
    bad_form(n, "an extent above 2^24 (" + std::to_string(H) + " x " + std::to_string(W) + "): its pixel coordinates are no f32 values");
  if (H * W >= kGridSampleMaxPlane) bad_form(n, "a plane of " + std::to_string(H) + " x " + std::to_string(W) + " pixels (2^31 or more)");

  Step s;
  s.kind = StepKind::GridSample;
  s.in0 = x.buf;
  s.gs_mode = mode == "nearest" ? kGridNearest : kGridBilinear;
  s.gs_pad = padding == "border" ? kGridBorder : padding == "reflection" ? kGridReflection : kGridZeros;
  s.gs_align = n.attr_i("align_corners", 0) != 0;
  s.origin = node_label(n);
  int64_t OH = 0, OW = 0;
  if (!has_input(n, 1)) unsupported(n, "missing input 1");
  if (auto ap = affine_pending.find(n.inputs[1]); ap != affine_pending.end()) {
    const AffinePending &a = ap->second;
    if (a.theta.shape[0] != x.shape[0]) bad_form(n, "its grid's N disagrees: theta " + shape_str(a.theta.shape) + " against X " + shape_str(x.shape));
    s.gs_coords = kGridCoordsAffine;
    s.in1 = a.theta.buf;
    s.origin = a.origin + "+" + s.origin;
    OH = a.OH, OW = a.OW;
  } else {
    const Val g = get(n, 1);
    if (g.is_const) bad_form(n, "its grid is a constant; only an activation [N,Ho,Wo,2] is served");
    if (g.shape.size() == 5) bad_form(n, "a 5-D grid " + shape_str(g.shape) + " (volumetric sampling is not served)");
    if (g.shape.size() != 4 || g.ra != 0 || g.padded() || g.buf < 0) bad_form(n, "the grid must be an [N,Ho,Wo,2] activation, got " + shape_str(g.shape));
    if (g.shape[0] != x.shape[0]) bad_form(n, "its grid's N disagrees: grid " + shape_str(g.shape) + " against X " + shape_str(x.shape));
    if (g.shape[3] != 2) bad_form(n, "its grid's last extent is " + std::to_string(g.shape[3]) + ", not 2: grid " + shape_str(g.shape));
    OH = g.shape[1], OW = g.shape[2];
    s.gs_coords = g.cl ? kGridCoordsPlanar : kGridCoordsGrid;
    s.in1 = g.buf;
  }
  if (OH < 1 || OW < 1) bad_form(n, "symbolic spatial extents: the grid must have constant Ho and Wo");
  if (OH > kGridSampleMaxPlane / OW || OH * OW >= kGridSampleMaxPlane) bad_form(n, "a grid of " + std::to_string(OH) + " x " + std::to_string(OW) + " positions (2^31 or more)");
  s.C = C, s.H = H, s.Wd = W, s.Mo = C, s.OH = OH, s.OW = OW;
  const std::vector<int64_t> shape = {x.shape[0], C, OH, OW};
  set_act(n, push_step(std::move(s), shape), shape);
}

}  // namespace lowering

}  // namespace infera_hip
