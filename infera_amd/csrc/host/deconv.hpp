// deconv.hpp -- what the lowering precomputes for the steps that make a tensor spatially larger:
//   ConvTranspose2d: the stride-phase decomposition.  Output pixel (oh, ow) belongs to phase (ph, pw) = ((oh + pt) mod sh, (ow + pl) mod sw);
//     only taps with ky * dh == ph (mod sh), kx * dw == pw (mod sw) reach it, from input pixel ih = (oh + pt - ky * dh) / sh (likewise iw): each
//     phase is an ordinary stride-1 convolution of the input with a sub-filter, and no multiply is spent on an inserted zero.  The lists are
//     separable (a phase's taps are the product of its row list and its column list, ascending in (ky, kx)) and fixed at load.
//   Resize2d: the per-output-row and per-output-column source tables of the ONNX coordinate formulas, computed in f64.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace infera_hip {

struct Step;

// One axis of a transposed convolution, phase by phase
struct ConvTAxisPhase {
  int out0 = 0;    // first output coordinate of the phase
  int count = 0;   // output coordinates of the phase: out0, out0 + s, ...
  std::vector<int> tap;  // the taps that reach it, ascending
  std::vector<int> q;    // per tap: input coordinate = (index inside the phase) + q   (may leave the image: the kernels mask)
};
std::vector<ConvTAxisPhase> convt_axis_phases(int64_t out, int64_t k, int64_t s, int64_t d, int64_t pad_begin);

constexpr int64_t kConvTMaxKernel = 64;  // kernel extent per axis the device tables are laid out for

struct DeconvPack {
  // ---- ConvTranspose2d ----
  std::vector<ConvTAxisPhase> hphase, wphase;  // [sh], [sw]
  int64_t out_pad_h = 0, out_pad_w = 0;        // the output_padding attribute (diagnostics; OH / OW already include it)
  // the axis tables as the kernels read them: per row phase [out0, count, taps, (ky, q) x kh], then per column phase the same with kw
  std::vector<int32_t> tab;
  int h_stride = 0, w_stride = 0;  // ints per phase record
  int64_t max_phase_pixels = 0;    // of one image
  // ---- Resize2d ----
  bool linear = false;
  std::string coord_mode, nearest_mode;
  // nearest: idx[o] = source index.  linear: idx[2o], idx[2o + 1] = i0, i1 and wgt[2o], wgt[2o + 1] = 1 - w, w (each rounded once to f32 from the f64 value)
  std::vector<int32_t> row_idx, col_idx;
  std::vector<float> row_wgt, col_wgt;
};

// fills DeconvPack::hphase / wphase / tab from the step's geometry fields
void convt_build_phases(const Step &s, DeconvPack &p);
// one axis of a Resize: `scale` as the operator specification defines it (the `scales` entry, or out / in when `sizes` is given)
void resize_axis_table(int64_t in, int64_t out, double scale, bool linear, const std::string &coord_mode, const std::string &nearest_mode,
                       std::vector<int32_t> &idx, std::vector<float> &wgt);

}  // namespace infera_hip
