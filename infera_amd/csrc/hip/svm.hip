// svm.hip -- ai.onnx.ml SVMRegressor / SVMClassifier on gfx950 (semantics: INTEGRATION.md section 2.6; tables: host/svm.hpp).
//
// svm_kernel_kernel: a wave owns 32 table rows, a workgroup 1, 2 or 4 waves (as many as keep the row tiles within 64 KB of LDS;
// one wave and up to 129 KB for F > 504).  The rows are staged in LDS once (row stride F_pad + 4 floats: conflict-free
// ds_read_b128), centered on the load-time SV mean for RBF, a NaN or +-Inf feature staged as NaN (0 . NaN = NaN against every SV, the
// padding ones included: such a row is NaN throughout, whatever the class sizes), and their squared norms summed in a fixed order.
// Block b works on row tile b / S and SV slice b % S; a slice is a run of 32-SV tiles inside one class block, fixed at load from the
// model alone.
// Per SV tile:
//   stage 1  K^T[sv, row] = S . X^T on v_mfma_f32_32x32x2_f32 (exact f32: a k-ordered fma chain), A = S straight from L2 in
//            fragment order (one 16-B load per lane feeds four k-steps), B = X from LDS.  k order inside each group of 8 features
//            is 0,4,1,5,2,6,3,7 (the dense.hip permutation): S is packed with the same order, nothing else changes.
//   epilogue on the VALU, in registers, while the other waves of the SIMD issue MFMAs: RBF exp(-gamma * max(|x|^2 + |s|^2 - 2 x.s, 0))
//            (a NaN row stays NaN), POLY (gamma x.s + coef0)^degree by squaring, SIGMOID tanh, LINEAR x.s.
//   stage 2  lane (r, h) holds K for row r and SVs 8 (i >> 2) + 4 h + (i & 3), i = 0..15.  Up to 8 coefficient rows (regressor,
//            binary, C <= 9): a VALU dot product per lane, the two lane halves added in fixed order at the end of the slice.  More
//            rows: a second MFMA with the K registers as its B operand as they are (k-step i of half h is that SV), A = the
//            coefficients packed in the matching order; each SV feeds only the C - 1 rows of its own class block (2 n_SV (C - 1)
//            flop per row, not 2 n_SV P), because the class blocks are padded to whole tiles.
// The slice's sums go to part[slice][row][Q] with plain stores.  svm_reduce_kernel (one lane per row) adds a class's slices in slice
// order (f64), forms d_p = A_i[j - 1] + A_j[i] + rho[p], and produces the value, the one-class sign, the decisions, the votes and
// label, or Platt's sigmoid + libsvm's pairwise coupling (f64, C <= 16).  No float atomics anywhere: a row's bits depend only on the
// model and the row, never on the row count, the chunking or the call path.
//
// Bound: 2 F_pad n_SV (+ 2 * 32 n_SV per 32 coefficient rows above 8) MFMA flop per row at 157.3 TFLOP/s; the exp / tanh epilogue
// (16 per lane per tile, 8 issue cycles each) hides behind the 64-cycle MFMAs only while F_pad >= ~32.
#include "device_common.hpp"

#include "../host/plan.hpp"

#include <cmath>

namespace infera_hip::kern {

namespace {

constexpr int kMaxWaves = 4;
constexpr int kLdsBudget = 64 * 1024;

template <int KT>
__device__ __forceinline__ float kernel_fn(float dot, float xn, float sn, float gamma, float coef0, int degree) {
  if constexpr (KT == kSvmRbf) {
    float d2 = xn + sn - 2.f * dot;
    d2 = d2 < 0.f ? 0.f : d2;  // (cancellation; NaN stays NaN)
    return __expf(-gamma * d2);
  } else if constexpr (KT == kSvmPoly) {
    float b = gamma * dot + coef0, r = 1.f;
    for (int e = degree; e; e >>= 1) {
      if (e & 1) r *= b;
      b *= b;
    }
    return r;
  } else if constexpr (KT == kSvmSigmoid) {
    return tanhf(gamma * dot + coef0);
  } else {
    return dot;
  }
}

// QW: stage-2 width, 1 / 2 / 4 / 8 (VALU) or 32 / 64 (MFMA)
template <int KT, int QW>
__global__ __launch_bounds__(kMaxWaves * 64) void svm_kernel_kernel(const float *__restrict__ x, int F, int F_pad, const float *__restrict__ center,
                                                                   const f32x4 *__restrict__ sv, const float *__restrict__ sv_norm,
                                                                   const float *__restrict__ coef, const uint32_t *__restrict__ slice_tile,
                                                                   float *__restrict__ part, int64_t nr, int S, int Q, float gamma, float coef0,
                                                                   int degree) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int nw = int(blockDim.x >> 6), wave = int(threadIdx.x >> 6), lane = int(threadIdx.x & 63), r = lane & 31, h = lane >> 5;
  const int s = int(blockIdx.x % unsigned(S));
  const int64_t row0 = int64_t(blockIdx.x / unsigned(S)) * (32 * nw) + 32 * wave;
  const int stride = F_pad + 4;
  float *tile = lds + wave * 32 * stride;
  for (int e = lane; e < 32 * F_pad; e += 64) {
    const int rr = e / F_pad, k = e - rr * F_pad;
    const int64_t g = row0 + rr;
    float v = 0.f;
    if (k < F && g < nr) {
      v = x[g * F + k];
      if constexpr (KT == kSvmRbf) v -= center[k];
      if (!(fabsf(v) < INFINITY)) v = NAN;  // the non-finite rule of INTEGRATION.md 2.6: NaN and +-Inf alike poison their row
    }
    tile[rr * stride + k] = v;
  }
  __syncthreads();
  float xn = 0.f;
  if constexpr (KT == kSvmRbf) {  // |x - center|^2: each lane half sums half of the features, halves added in order
    const int half = F_pad / 2;
    float a = 0.f;
    for (int k = h * half; k < (h + 1) * half; k++) a = fmaf(tile[r * stride + k], tile[r * stride + k], a);
    const float o = __shfl_xor(a, 32);
    xn = h ? o + a : a + o;
  }

  constexpr bool kMfma2 = QW >= 32;
  constexpr int QT = kMfma2 ? QW / 32 : 1;
  float a2[kMfma2 ? 1 : QW];
  f32x16 m2[QT];
#pragma unroll
  for (int q = 0; q < (kMfma2 ? 1 : QW); q++) a2[q] = 0.f;
#pragma unroll
  for (int qt = 0; qt < QT; qt++)
#pragma unroll
    for (int i = 0; i < 16; i++) m2[qt][i] = 0.f;

  const int G = F_pad / 8;
  const float *xr = tile + r * stride + 4 * h;
  const uint32_t t_end = slice_tile[s + 1];
  for (uint32_t t = slice_tile[s]; t < t_end; t++) {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.f;
    const f32x4 *st = sv + int64_t(t) * G * 64 + lane;
    for (int g = 0; g < G; g++) {
      const f32x4 a4 = st[g * 64];
      const f32x4 b4 = *reinterpret_cast<const f32x4 *>(xr + 8 * g);
#pragma unroll
      for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j], b4[j], acc, 0, 0, 0);
    }
    // acc[i] = x_r . s for SV 32 t + 8 (i >> 2) + 4 h + (i & 3)
    float sn[16];
#pragma unroll
    for (int i = 0; i < 16; i++) sn[i] = KT == kSvmRbf ? sv_norm[int64_t(t) * 32 + 8 * (i >> 2) + 4 * h + (i & 3)] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = kernel_fn<KT>(acc[i], xn, sn[i], gamma, coef0, degree);
    if constexpr (!kMfma2) {
      const float *cf = coef + (int64_t(t) * 2 + h) * 16 * QW;
#pragma unroll
      for (int i = 0; i < 16; i++)
#pragma unroll
        for (int q = 0; q < QW; q++) a2[q] = fmaf(acc[i], cf[i * QW + q], a2[q]);
    } else {
#pragma unroll
      for (int qt = 0; qt < QT; qt++) {
        const f32x4 *cf = reinterpret_cast<const f32x4 *>(coef) + (int64_t(t) * QT + qt) * 4 * 64 + lane;
#pragma unroll
        for (int i4 = 0; i4 < 4; i4++) {
          const f32x4 c4 = cf[i4 * 64];
#pragma unroll
          for (int j = 0; j < 4; j++) m2[qt] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4[j], acc[4 * i4 + j], m2[qt], 0, 0, 0);
        }
      }
    }
  }

  const int64_t row = row0 + r;
  float *out = part + (int64_t(s) * nr + row) * Q;
  if constexpr (!kMfma2) {
#pragma unroll
    for (int q = 0; q < QW; q++) {
      const float o = __shfl_xor(a2[q], 32);
      a2[q] = h ? o + a2[q] : a2[q] + o;
    }
    if (h == 0 && row < nr)
#pragma unroll
      for (int q = 0; q < QW; q++)
        if (q < Q) out[q] = a2[q];
  } else {
    if (row < nr)
#pragma unroll
      for (int qt = 0; qt < QT; qt++)
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const int q = 32 * qt + 8 * (i >> 2) + 4 * h + (i & 3);
          if (q < Q) out[q] = m2[qt][i];
        }
  }
}

constexpr int kReduceBlock = 64;
constexpr int kMaxC = 64, kMaxProbC = 16;

__device__ __forceinline__ double platt(double d, double A, double B) {  // libsvm's overflow-safe sigmoid, clamped (NaN stays NaN)
  const double f = d * A + B;
  double p = f >= 0.0 ? exp(-f) / (1.0 + exp(-f)) : 1.0 / (1.0 + exp(f));
  if (p < 1e-7) p = 1e-7;
  if (p > 1.0 - 1e-7) p = 1.0 - 1e-7;
  return p;
}

// part: [S][nr][Q]; class_slice: first slice per class (C + 1); mode: host/plan.hpp SvmOut
__global__ __launch_bounds__(kReduceBlock) void svm_reduce_kernel(const float *__restrict__ part, const uint32_t *__restrict__ class_slice,
                                                                 const float *__restrict__ rho, const float *__restrict__ labels,
                                                                 const float *__restrict__ prob_a, const float *__restrict__ prob_b,
                                                                 float *__restrict__ y, int64_t nr, int Q, int C, int mode) {
  const int64_t stride = int64_t(gridDim.x) * kReduceBlock;
  for (int64_t row = int64_t(blockIdx.x) * kReduceBlock + threadIdx.x; row < nr; row += stride) {
    auto block = [&](int c, int q) {  // sum over class block c, coefficient row q: its slices in order
      double v = 0.0;
      for (uint32_t s = class_slice[c]; s < class_slice[c + 1]; s++) v += double(part[(int64_t(s) * nr + row) * Q + q]);
      return v;
    };
    if (mode == kSvmValue || mode == kSvmOneClass) {
      const double d = block(0, 0) + double(rho[0]);
      y[row] = mode == kSvmValue ? float(d) : (d > 0.0 ? 1.f : -1.f);
      continue;
    }
    auto decision = [&](int i, int j, int p) { return block(i, j - 1) + block(j, i) + double(rho[p]); };
    const int P = C * (C - 1) / 2;
    if (mode == kSvmLabel) {
      int votes[kMaxC];
      for (int c = 0; c < C; c++) votes[c] = 0;
      for (int i = 0, p = 0; i < C; i++)
        for (int j = i + 1; j < C; j++, p++) votes[decision(i, j, p) > 0.0 ? i : j]++;
      int best = 0;
      for (int c = 1; c < C; c++)
        if (votes[c] > votes[best]) best = c;  // the first maximum
      y[row] = labels[best];
      continue;
    }
    if (mode == kSvmDecision) {
      if (C == 2) {
        const double d = decision(0, 1, 0);
        y[2 * row] = float(d);
        y[2 * row + 1] = float(-d);
      } else {
        for (int i = 0, p = 0; i < C; i++)
          for (int j = i + 1; j < C; j++, p++) y[row * P + p] = float(decision(i, j, p));
      }
      continue;
    }
    // kSvmProb
    if (C == 2) {
      const double r01 = platt(decision(0, 1, 0), double(prob_a[0]), double(prob_b[0]));
      y[2 * row] = float(r01);
      y[2 * row + 1] = float(1.0 - r01);
      continue;
    }
    double Qm[kMaxProbC][kMaxProbC], Qp[kMaxProbC], pr[kMaxProbC];
    bool nan = false;
    for (int t = 0; t < C; t++) Qm[t][t] = 0.0;
    for (int i = 0, p = 0; i < C; i++)
      for (int j = i + 1; j < C; j++, p++) {
        const double rij = platt(decision(i, j, p), double(prob_a[p]), double(prob_b[p])), rji = 1.0 - rij;
        nan = nan || rij != rij;
        Qm[i][i] += rji * rji;  // (for each t, in ascending order of the other class: libsvm's order)
        Qm[j][j] += rij * rij;
        Qm[i][j] = Qm[j][i] = -rji * rij;
      }
    if (nan) {
      for (int t = 0; t < C; t++) y[row * C + t] = NAN;
      continue;
    }
    // libsvm multiclass_probability (Wu, Lin and Weng 2004, method 2)
    const int max_iter = C > 100 ? C : 100;
    const double eps = 0.005 / C;
    for (int t = 0; t < C; t++) pr[t] = 1.0 / C;
    for (int it = 0; it < max_iter; it++) {
      double pQp = 0.0;
      for (int t = 0; t < C; t++) {
        Qp[t] = 0.0;
        for (int j = 0; j < C; j++) Qp[t] += Qm[t][j] * pr[j];
        pQp += pr[t] * Qp[t];
      }
      double max_error = 0.0;
      for (int t = 0; t < C; t++) max_error = fmax(max_error, fabs(Qp[t] - pQp));
      if (max_error < eps) break;
      for (int t = 0; t < C; t++) {
        const double diff = (-Qp[t] + pQp) / Qm[t][t];
        pr[t] += diff;
        pQp = (pQp + diff * (diff * Qm[t][t] + 2.0 * Qp[t])) / (1.0 + diff) / (1.0 + diff);
        for (int j = 0; j < C; j++) {
          Qp[j] = (Qp[j] + diff * Qm[t][j]) / (1.0 + diff);
          pr[j] /= (1.0 + diff);
        }
      }
    }
    for (int t = 0; t < C; t++) y[row * C + t] = float(pr[t]);
  }
}

template <int KT, int QW>
bool kernel_launch(hipStream_t s, const float *x, int F, int F_pad, const float *center, const float *sv, const float *sv_norm, const float *coef,
                   const uint32_t *slice_tile, float *part, int64_t rows, int S, int Q, float gamma, float coef0, int degree) {
  int nw = kMaxWaves;
  while (nw > 1 && size_t(nw) * 32 * size_t(F_pad + 4) * 4 > size_t(kLdsBudget)) nw /= 2;
  const size_t lds = size_t(nw) * 32 * size_t(F_pad + 4) * 4;
  auto kernel = svm_kernel_kernel<KT, QW>;
  if (lds > size_t(kLdsBudget) &&  // F > 504: one wave, dynamic LDS beyond 64 KB is opt-in
      hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
    return false;
  const int64_t tiles = (rows + 32 * nw - 1) / (32 * nw);
  hipLaunchKernelGGL(kernel, dim3(unsigned(tiles * S)), dim3(unsigned(64 * nw)), lds, s, x, F, F_pad, center, reinterpret_cast<const f32x4 *>(sv),
                     sv_norm, coef, slice_tile, part, rows, S, Q, gamma, coef0, degree);
  return true;
}

template <int KT>
bool kernel_dispatch(hipStream_t s, const float *x, int F, int F_pad, const float *center, const float *sv, const float *sv_norm, const float *coef,
                     const uint32_t *slice_tile, float *part, int64_t rows, int S, int Q, int QW, float gamma, float coef0, int degree) {
#define INFERA_SVM_QW(W) \
  if (QW == W) return kernel_launch<KT, W>(s, x, F, F_pad, center, sv, sv_norm, coef, slice_tile, part, rows, S, Q, gamma, coef0, degree);
  INFERA_SVM_QW(1) INFERA_SVM_QW(2) INFERA_SVM_QW(4) INFERA_SVM_QW(8) INFERA_SVM_QW(32) INFERA_SVM_QW(64)
#undef INFERA_SVM_QW
  return false;  // (no such stage-2 width: host/svm.cpp writes 1, 2, 4, 8, 32 or 64)
}

}  // namespace

bool svm_kernel(hipStream_t s, const float *x, int F, int F_pad, int kernel, const float *center, const float *sv, const float *sv_norm, const float *coef,
                const uint32_t *slice_tile, float *part, int64_t rows, int S, int Q, int QW, float gamma, float coef0, int degree) {
  if (rows <= 0) return true;
  switch (kernel) {
    case kSvmPoly: return kernel_dispatch<kSvmPoly>(s, x, F, F_pad, center, sv, sv_norm, coef, slice_tile, part, rows, S, Q, QW, gamma, coef0, degree);
    case kSvmRbf: return kernel_dispatch<kSvmRbf>(s, x, F, F_pad, center, sv, sv_norm, coef, slice_tile, part, rows, S, Q, QW, gamma, coef0, degree);
    case kSvmSigmoid: return kernel_dispatch<kSvmSigmoid>(s, x, F, F_pad, center, sv, sv_norm, coef, slice_tile, part, rows, S, Q, QW, gamma, coef0, degree);
    default: return kernel_dispatch<kSvmLinear>(s, x, F, F_pad, center, sv, sv_norm, coef, slice_tile, part, rows, S, Q, QW, gamma, coef0, degree);
  }
}

void svm_reduce(hipStream_t s, const float *part, const uint32_t *class_slice, const float *rho, const float *labels, const float *prob_a,
                const float *prob_b, float *y, int64_t rows, int Q, int C, int mode) {
  if (rows <= 0) return;
  const int64_t g = std::min<int64_t>(4096, (rows + kReduceBlock - 1) / kReduceBlock);
  hipLaunchKernelGGL(svm_reduce_kernel, dim3(unsigned(g)), dim3(kReduceBlock), 0, s, part, class_slice, rho, labels, prob_a, prob_b, y, rows, Q, C, mode);
}

}  // namespace infera_hip::kern
