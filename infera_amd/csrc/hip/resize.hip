// resize.hip -- ONNX Resize / Upsample (nearest, linear) of an [N,C,H,W] tensor: an HBM-bound helper.  The source tables come from the
// lowering (host/deconv.cpp: the operator specification's coordinate formulas in f64); the kernel is grid-stride over the output, one
// element per lane in NCHW and one channel quad (16 bytes) per lane in channel-quad planes.  Linear: the horizontal interpolation first,
// then the vertical one, each as fma(w, b, (1 - w) * a) with 1 - w from the table: two roundings per interpolation, written with fmaf so
// that the form does not depend on the compiler's contraction setting.
#include "device_common.hpp"

#include <algorithm>

namespace infera_hip::kern {

namespace {

constexpr int kBlock = 256;

// w0 * a + w1 * b with two roundings: the product w0 * a, then the fused multiply-add
__device__ __forceinline__ float lerp(float a, float b, float w0, float w1) { return fmaf(w1, b, __fmul_rn(w0, a)); }
__device__ __forceinline__ f32x4 lerp(f32x4 a, f32x4 b, float w0, float w1) {
  return f32x4{lerp(a[0], b[0], w0, w1), lerp(a[1], b[1], w0, w1), lerp(a[2], b[2], w0, w1), lerp(a[3], b[3], w0, w1)};
}

// T = float (NCHW: planes = rows * C) or f32x4 (channel-quad planes: planes = rows * C / 4)
template <typename T, bool LINEAR>
__global__ __launch_bounds__(kBlock) void resize2d_kernel(const T *__restrict__ X, T *__restrict__ Y, int64_t total, int H, int W, int OH, int OW,
                                                         const int *__restrict__ row_idx, const int *__restrict__ col_idx,
                                                         const float *__restrict__ row_wgt, const float *__restrict__ col_wgt) {
  for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < total; e += int64_t(gridDim.x) * kBlock) {
    const int ow = int(e % OW);
    int64_t t = e / OW;
    const int oh = int(t % OH);
    const T *src = X + (t / OH) * int64_t(H) * W;
    if constexpr (!LINEAR) {
      Y[e] = src[int64_t(row_idx[oh]) * W + col_idx[ow]];
    } else {
      const int y0 = row_idx[2 * oh], y1 = row_idx[2 * oh + 1], x0 = col_idx[2 * ow], x1 = col_idx[2 * ow + 1];
      const float wy0 = row_wgt[2 * oh], wy1 = row_wgt[2 * oh + 1], wx0 = col_wgt[2 * ow], wx1 = col_wgt[2 * ow + 1];
      Y[e] = lerp(lerp(src[int64_t(y0) * W + x0], src[int64_t(y0) * W + x1], wx0, wx1), lerp(src[int64_t(y1) * W + x0], src[int64_t(y1) * W + x1], wx0, wx1), wy0, wy1);
    }
  }
}

}  // namespace

void resize2d(hipStream_t s, const float *X, float *Y, int64_t rows, int C, int H, int W, int OH, int OW, const int *row_idx, const int *col_idx,
              const float *row_wgt, const float *col_wgt, bool linear, bool cq) {
  const int64_t total = rows * (cq ? C / 4 : C) * OH * OW;
  if (total <= 0) return;
  const dim3 grid(unsigned(std::min<int64_t>((total + kBlock - 1) / kBlock, 65536)));
  auto *X4 = reinterpret_cast<const f32x4 *>(X);
  auto *Y4 = reinterpret_cast<f32x4 *>(Y);
  if (cq && linear) hipLaunchKernelGGL((resize2d_kernel<f32x4, true>), grid, dim3(kBlock), 0, s, X4, Y4, total, H, W, OH, OW, row_idx, col_idx, row_wgt, col_wgt);
  else if (cq) hipLaunchKernelGGL((resize2d_kernel<f32x4, false>), grid, dim3(kBlock), 0, s, X4, Y4, total, H, W, OH, OW, row_idx, col_idx, row_wgt, col_wgt);
  else if (linear) hipLaunchKernelGGL((resize2d_kernel<float, true>), grid, dim3(kBlock), 0, s, X, Y, total, H, W, OH, OW, row_idx, col_idx, row_wgt, col_wgt);
  else hipLaunchKernelGGL((resize2d_kernel<float, false>), grid, dim3(kBlock), 0, s, X, Y, total, H, W, OH, OW, row_idx, col_idx, row_wgt, col_wgt);
}

}  // namespace infera_hip::kern
