// svm.cpp -- SVMClassifier / SVMRegressor: validation, the load-time RBF center, SV tiles padded per class, slices, stage-2 layouts.
#include "svm.hpp"

#include <algorithm>
#include <cmath>

#include "plan.hpp"

namespace infera_hip {

namespace {

[[noreturn]] void fail(const std::string &why) { throw SvmError("unsupported operator form: " + why); }

std::vector<float> floats_of(const onnx::NodeDef &n, const char *k) {
  const onnx::Attribute *a = n.attr(k);
  return a ? a->floats : std::vector<float>{};
}

std::string num(int64_t v) { return std::to_string(v); }

}  // namespace

SvmPack pack_svm(const onnx::NodeDef &n, int64_t F) {
  SvmPack p;
  p.classifier = n.op == "SVMClassifier";
  p.F = F;

  // ---- kernel
  const std::string kt = n.attr_s("kernel_type", "LINEAR");
  if (kt == "LINEAR") p.kernel = kSvmLinear;
  else if (kt == "POLY") p.kernel = kSvmPoly;
  else if (kt == "RBF") p.kernel = kSvmRbf;
  else if (kt == "SIGMOID") p.kernel = kSvmSigmoid;
  else fail("unknown kernel_type '" + kt + "'");
  const std::vector<float> kp = floats_of(n, "kernel_params");
  if (!n.attr("kernel_params") && p.kernel != kSvmLinear) fail(kt + " kernel without kernel_params");
  if (n.attr("kernel_params") && kp.size() != 3) fail("kernel_params holds " + num(int64_t(kp.size())) + " values, expected 3 (gamma, coef0, degree)");
  if (kp.size() == 3) {
    p.gamma = kp[0];
    p.coef0 = kp[1];
    if (p.kernel == kSvmPoly) {
      const float d = kp[2];
      if (!(d == std::floor(d)) || d < 1.f || d > float(kSvmMaxDegree))
        fail("POLY degree " + std::to_string(d) + " is not an integer from 1 to " + num(kSvmMaxDegree));
      p.degree = int(d);
    }
  }

  // ---- post_transform
  const std::string pt = n.attr_s("post_transform", "NONE");
  if (pt != "NONE" && pt != "LOGISTIC" && pt != "SOFTMAX") fail("post_transform " + pt);

  // ---- support vectors, classes
  if (F > kSvmMaxF) fail("input width " + num(F) + " is above the cap of " + num(kSvmMaxF));
  const std::vector<float> sv = floats_of(n, "support_vectors"), coef = floats_of(n, "coefficients"), rho = floats_of(n, "rho");
  std::vector<int64_t> per_class;  // SVs per class block, in order
  if (p.classifier) {
    if (n.attr("classlabels_strings")) fail("string class labels cannot be returned as numbers");
    const auto *lab = n.attr_ints("classlabels_ints");
    if (!lab || lab->size() < 2) fail("needs at least two classlabels_ints");
    p.classes = int64_t(lab->size());
    if (p.classes > kSvmMaxClasses) fail("C = " + num(p.classes) + " classes, above the cap of " + num(kSvmMaxClasses));
    for (int64_t v : *lab) p.labels.push_back(float(v));
    const auto *vpc = n.attr_ints("vectors_per_class");
    if (!vpc || vpc->empty()) fail("no support vectors (the linear form without vectors_per_class is not supported)");
    if (int64_t(vpc->size()) != p.classes) fail("vectors_per_class holds " + num(int64_t(vpc->size())) + " entries, expected C = " + num(p.classes));
    for (int64_t v : *vpc) {
      if (v < 0) fail("vectors_per_class holds a negative entry (" + num(v) + ")");
      if (v > kSvmMaxSupport) fail("vectors_per_class entry " + num(v) + " is above the cap of " + num(kSvmMaxSupport));
      p.n_sv += v;
    }
    per_class = *vpc;
    p.Q = p.classes - 1;
  } else {
    p.n_sv = n.attr_i("n_supports", int64_t(coef.size()));
    p.one_class = n.attr_i("one_class", 0) != 0;
    per_class = {p.n_sv};
    p.Q = 1;
  }
  if (p.n_sv <= 0 || sv.empty()) fail("no support vectors (the linear form without support_vectors is not supported)");
  if (p.n_sv > kSvmMaxSupport) fail("n_SV = " + num(p.n_sv) + " support vectors, above the cap of " + num(kSvmMaxSupport));
  if (int64_t(sv.size()) % F != 0) fail("support_vectors holds " + num(int64_t(sv.size())) + " values, not a multiple of the input width " + num(F));
  if (int64_t(sv.size()) / F != p.n_sv)
    fail("support_vectors holds " + num(int64_t(sv.size()) / F) + " vectors of the input width " + num(F) + ", but " +
         (p.classifier ? "vectors_per_class sums to " : "n_supports is ") + num(p.n_sv));
  if (p.n_sv * F > kSvmMaxValues) fail("n_SV x F = " + num(p.n_sv * F) + " values, above the cap of " + num(kSvmMaxValues));
  if (int64_t(coef.size()) != p.Q * p.n_sv)
    fail("coefficients holds " + num(int64_t(coef.size())) + " values, expected " + (p.classifier ? "(C - 1) x n_SV = " : "n_SV = ") + num(p.Q * p.n_sv));
  const int64_t P = p.classifier ? p.classes * (p.classes - 1) / 2 : 1;
  if (int64_t(rho.size()) != P) fail("rho holds " + num(int64_t(rho.size())) + " values, expected " + num(P));
  p.rho = rho;
  if (p.classifier) {
    const bool ha = n.attr("prob_a") != nullptr, hb = n.attr("prob_b") != nullptr;
    if (ha != hb) fail(std::string("only ") + (ha ? "prob_a" : "prob_b") + " is given (probabilities need both)");
    if (ha) {
      p.prob_a = floats_of(n, "prob_a");
      p.prob_b = floats_of(n, "prob_b");
      if (int64_t(p.prob_a.size()) != P) fail("prob_a holds " + num(int64_t(p.prob_a.size())) + " values, expected " + num(P));
      if (int64_t(p.prob_b.size()) != P) fail("prob_b holds " + num(int64_t(p.prob_b.size())) + " values, expected " + num(P));
      if (p.classes > kSvmMaxProbClasses)
        fail("probabilities for C = " + num(p.classes) + " classes, above the cap of " + num(kSvmMaxProbClasses));
      p.probabilities = true;
    }
  }

  // ---- layout: class blocks padded to SV tiles, slices inside each class
  p.F_pad = (F + 7) / 8 * 8;
  std::vector<int64_t> tile0(per_class.size() + 1, 0), sv0(per_class.size() + 1, 0);
  for (size_t c = 0; c < per_class.size(); c++) {
    tile0[c + 1] = tile0[c] + (per_class[c] + kSvmTile - 1) / kSvmTile;
    sv0[c + 1] = sv0[c] + per_class[c];
  }
  p.tiles = tile0.back();
  const int64_t L = std::max(kSvmMinSliceTiles, (p.tiles + kSvmTargetSlices - 1) / kSvmTargetSlices);
  p.class_slice.push_back(0);
  for (size_t c = 0; c < per_class.size(); c++) {
    const int64_t T = tile0[c + 1] - tile0[c], k = (T + L - 1) / L;
    for (int64_t i = 0; i < k; i++) p.slice_tile.push_back(uint32_t(tile0[c] + T * i / k));
    p.class_slice.push_back(uint32_t(p.slice_tile.size()));
  }
  p.slices = int64_t(p.slice_tile.size());
  p.slice_tile.push_back(uint32_t(p.tiles));

  // ---- support vectors (RBF: centered on their mean, |s|^2), padded index -> original index
  const int64_t npad = p.tiles * kSvmTile;
  std::vector<int64_t> orig(size_t(npad), -1);
  for (size_t c = 0; c < per_class.size(); c++)
    for (int64_t m = 0; m < per_class[c]; m++) orig[size_t(tile0[c] * kSvmTile + m)] = sv0[c] + m;
  std::vector<double> mean(size_t(F), 0.0);
  if (p.kernel == kSvmRbf) {
    for (int64_t s = 0; s < p.n_sv; s++)
      for (int64_t k = 0; k < F; k++) mean[size_t(k)] += double(sv[size_t(s * F + k)]);
    p.center.assign(size_t(p.F_pad), 0.f);
    for (int64_t k = 0; k < F; k++) p.center[size_t(k)] = float(mean[size_t(k)] / double(p.n_sv));
    p.sv_norm.assign(size_t(npad), 0.f);
  }
  auto sval = [&](int64_t s, int64_t k) -> float {  // centered f32 value of padded SV s, feature k
    if (k >= F || orig[size_t(s)] < 0) return 0.f;
    const float v = sv[size_t(orig[size_t(s)] * F + k)];
    return p.kernel == kSvmRbf ? float(double(v) - double(p.center[size_t(k)])) : v;
  };
  p.sv.assign(size_t(npad * p.F_pad), 0.f);
  const int64_t G = p.F_pad / 8;
  for (int64_t t = 0; t < p.tiles; t++)
    for (int64_t g = 0; g < G; g++)
      for (int lane = 0; lane < 64; lane++)
        for (int j = 0; j < 4; j++)
          p.sv[size_t(((t * G + g) * 64 + lane) * 4 + j)] = sval(t * kSvmTile + (lane & 31), 8 * g + 4 * (lane >> 5) + j);
  if (p.kernel == kSvmRbf)
    for (int64_t s = 0; s < npad; s++) {
      double a = 0.0;
      for (int64_t k = 0; k < F; k++) a += double(sval(s, k)) * double(sval(s, k));
      p.sv_norm[size_t(s)] = float(a);
    }

  // ---- stage-2 coefficients
  auto cval = [&](int64_t q, int64_t s) -> float {  // coefficient row q of padded SV s
    if (q >= p.Q || orig[size_t(s)] < 0) return 0.f;
    return coef[size_t(q * p.n_sv + orig[size_t(s)])];
  };
  auto sv_of = [](int64_t t, int i, int h) { return t * kSvmTile + 8 * (i >> 2) + 4 * h + (i & 3); };
  if (p.Q <= kSvmValuMaxQ) {
    p.QW = p.Q <= 1 ? 1 : p.Q <= 2 ? 2 : p.Q <= 4 ? 4 : 8;
    p.coef.assign(size_t(p.tiles * 32 * p.QW), 0.f);
    for (int64_t t = 0; t < p.tiles; t++)
      for (int h = 0; h < 2; h++)
        for (int i = 0; i < 16; i++)
          for (int64_t q = 0; q < p.QW; q++) p.coef[size_t(((t * 2 + h) * 16 + i) * p.QW + q)] = cval(q, sv_of(t, i, h));
  } else {
    const int64_t QT = (p.Q + 31) / 32;
    p.QW = 32 * QT;
    p.coef.assign(size_t(p.tiles * QT * 1024), 0.f);
    for (int64_t t = 0; t < p.tiles; t++)
      for (int64_t qt = 0; qt < QT; qt++)
        for (int i4 = 0; i4 < 4; i4++)
          for (int lane = 0; lane < 64; lane++)
            for (int j = 0; j < 4; j++)
              p.coef[size_t((((t * QT + qt) * 4 + i4) * 64 + lane) * 4 + j)] = cval(32 * qt + (lane & 31), sv_of(t, 4 * i4 + j, lane >> 5));
  }
  return p;
}

}  // namespace infera_hip
