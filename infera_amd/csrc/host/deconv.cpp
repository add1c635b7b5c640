// deconv.cpp -- phase tap lists of transposed convolutions and source tables of Resize (host/deconv.hpp).
#include "deconv.hpp"

#include <algorithm>
#include <cmath>

#include "plan.hpp"

namespace infera_hip {

std::vector<ConvTAxisPhase> convt_axis_phases(int64_t out, int64_t k, int64_t s, int64_t d, int64_t pad_begin) {
  std::vector<ConvTAxisPhase> phases(static_cast<size_t>(s));
  for (int64_t ph = 0; ph < s; ph++) {
    ConvTAxisPhase &a = phases[size_t(ph)];
    const int64_t out0 = ((ph - pad_begin) % s + s) % s;  // the first o >= 0 with (o + pad_begin) mod s == ph
    a.out0 = int(out0);
    a.count = out0 < out ? int((out - out0 + s - 1) / s) : 0;
    for (int64_t t = 0; t < k; t++)
      if ((t * d) % s == ph) {
        a.tap.push_back(int(t));
        a.q.push_back(int((out0 + pad_begin - t * d) / s));  // (exact: both terms are == ph mod s)
      }
  }
  return phases;
}

void convt_build_phases(const Step &s, DeconvPack &p) {
  p.hphase = convt_axis_phases(s.OH, s.kh, s.sh, s.dh, s.pt);
  p.wphase = convt_axis_phases(s.OW, s.kw, s.sw, s.dw, s.pl);
  p.h_stride = 3 + 2 * int(s.kh);
  p.w_stride = 3 + 2 * int(s.kw);
  p.tab.assign(size_t(s.sh) * p.h_stride + size_t(s.sw) * p.w_stride, 0);
  auto put = [&](const std::vector<ConvTAxisPhase> &ph, size_t base, int stride) {
    for (size_t i = 0; i < ph.size(); i++) {
      int32_t *r = p.tab.data() + base + i * size_t(stride);
      r[0] = ph[i].out0, r[1] = ph[i].count, r[2] = int(ph[i].tap.size());
      for (size_t t = 0; t < ph[i].tap.size(); t++) r[3 + 2 * t] = ph[i].tap[t], r[4 + 2 * t] = ph[i].q[t];
    }
  };
  put(p.hphase, 0, p.h_stride);
  put(p.wphase, size_t(s.sh) * p.h_stride, p.w_stride);
  p.max_phase_pixels = 0;
  for (const auto &a : p.hphase)
    for (const auto &b : p.wphase) p.max_phase_pixels = std::max<int64_t>(p.max_phase_pixels, int64_t(a.count) * b.count);
}

void resize_axis_table(int64_t in, int64_t out, double scale, bool linear, const std::string &coord_mode, const std::string &nearest_mode,
                       std::vector<int32_t> &idx, std::vector<float> &wgt) {
  idx.clear();
  wgt.clear();
  for (int64_t o = 0; o < out; o++) {
    double x;  // the source coordinate of output coordinate o (Resize, coordinate_transformation_mode)
    if (coord_mode == "half_pixel") x = (double(o) + 0.5) / scale - 0.5;
    else if (coord_mode == "pytorch_half_pixel") x = out > 1 ? (double(o) + 0.5) / scale - 0.5 : 0.0;
    else if (coord_mode == "align_corners") x = out > 1 ? double(o) * double(in - 1) / double(out - 1) : 0.0;
    else x = double(o) / scale;  // asymmetric
    if (!linear) {
      double r;
      if (nearest_mode == "floor") r = std::floor(x);
      else if (nearest_mode == "ceil") r = std::ceil(x);
      else if (nearest_mode == "round_prefer_ceil") r = std::floor(x + 0.5);
      else r = std::ceil(x - 0.5);  // round_prefer_floor
      idx.push_back(int32_t(std::min<double>(std::max(r, 0.0), double(in - 1))));
      continue;
    }
    x = std::min(std::max(x, 0.0), double(in - 1));  // (the specification clamps the coordinate to the image)
    const int64_t i0 = int64_t(std::floor(x)), i1 = std::min(i0 + 1, in - 1);
    const double w = x - double(i0);
    idx.push_back(int32_t(i0));
    idx.push_back(int32_t(i1));
    wgt.push_back(float(1.0 - w));  // (both weights from the f64 value, each rounded once: the kernel forms (1 - w) * a + w * b)
    wgt.push_back(float(w));
  }
}

}  // namespace infera_hip
