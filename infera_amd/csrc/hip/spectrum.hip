// spectrum.hip -- the Spectrum step (INTEGRATION.md section 2.6 "Spectral front ends"): the ONNX DFT and STFT operators on
// real signals x [rows, C, L] -- framing, window, an n-point real transform per frame, and complex / power / magnitude results in either
// layout, in one launch.  n = 2 h is a power of two in [8, 4096]; the kernel is instantiated per log2(h).
//
// Work split.  A work group of 4 waves owns one signal and a run of Fw consecutive frames.  It stages the span those frames cover,
//   (Fw - 1) min(hop, n) + n samples (hop >= n: the frames' own samples only, the gaps are never read), into LDS once -- 16-byte loads where
//   the host found pointer, row stride and run start aligned, else word loads; zeros beyond L -- so that a sample of n / hop overlapping
//   frames is read from memory once per work group.  Then each wave transforms `batches` batches of G frames side by side, G = max(1, 512 / h):
//   a batch is M = G h >= 512 complex points, P = M / 64 = 8, 16 or 32 per lane, so no lane idles for want of points at any n (G > 1 up to
//   n = 512, not only up to n = 64).  A grid of at most kMaxBlocks work groups strides over the (signal, run) units.
// Transform.  The frame is packed as z[j] = w[2j] x[2j] + i w[2j+1] x[2j+1] (the window multiplied on the read from the staged span) and
//   transformed as an h-point complex Stockham autosort FFT, decimation in time.  A pass of radix R over sub-transforms of length Ns reads
//   z[j + t h / R], t < R (consecutive lanes: consecutive addresses), multiplies by T[t k h / (Ns R)], k = j mod Ns, from the table (no
//   sincos in the kernel), runs the R-point butterfly in registers and writes to (j / Ns) Ns R + k + t Ns.  Radices: 8 while more than 4
//   levels or exactly 3 remain, else 4 -- every log2(h) in [2, 11] is a sum of 3s and 2s, so the radix-2 pass is never needed ("8.8.4").
//   Between passes the points go through the wave's own LDS region; a wave reads all its P points before it writes any, so one region
//   serves as source and destination and there is no work-group barrier inside a frame.
// Bank conflicts.  In this formulation the reads of a pass are contiguous and the WRITES are strided (by R points in the first pass).  Point
//   a lies at a + a / 32: the 8-point stride of 32 consecutive lanes then meets 32 different 8-byte columns.  NOT checked with counters.
// Split.  X[k] = 1/2 (Z[k] + conj Z[h-k]) - i/2 w^k (Z[k] - conj Z[h-k]), w^k = exp(-2 pi i k / n) from the table, k <= h; onesided = 0
//   writes X[n-k] = conj X[k] from the same values.  Epilogue: complex (re, im) with -0 written as +0; power fl(fl(re re) + fl(im im));
//   magnitude sqrtf(power) -- the correctly rounded f32 square root (hipcc's default).  Frames-major results are stored contiguously along
//   bins straight from the wave's region.  bins_major: the waves keep their batches' Z until all are done, then the work group passes the
//   results chunk of bins by chunk of bins through a [bins][Fw + 1] LDS tile (it lies over the dead staged span) and stores contiguously
//   along frames.
// Every value is a fixed sequence of separately rounded f32 operations (contraction is off) that depends on the model and the frame's own
// samples only: not on Fw, the frame's slot in its batch, the grid or the rows around it.  No atomics.  64-bit element offsets.
#include "device_common.hpp"

#include <algorithm>

#include "../host/spectrum.hpp"

#pragma clang fp contract(off)

namespace infera_hip::kern {

namespace {

constexpr int kBlock = 64 * kSpectrumWaves;
constexpr int kMaxBlocks = 2048;

struct SpectrumArgs {
  const float *x, *win;
  const float2 *tw, *split;
  float *y;
  int64_t units, in_stride, total;  // (signal, run) pairs; floats between two signals; floats of a signal
  int valid, hop, frames, bins, runs;  // valid: samples a separately staged frame reads (the rest is zero padding)
  int Fw, log_fw, batches, fs, span, stage_floats, tile_bins;  // fs = min(hop, n): floats between two frames of the staged span
  int mode;
  bool bins_major, vec4, separate;  // separate: the frames are staged one by one, n floats each (hop >= n, and DFT)
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int pad(int a) { return a + (a >> 5); }
__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
  const float p0 = a.x * w.x, p1 = a.y * w.y, p2 = a.x * w.y, p3 = a.y * w.x;
  return make_float2(p0 - p1, p2 + p3);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // a * (-i)

// natural-order 4-point transform of (a0, a1, a2, a3)
__device__ __forceinline__ void fft4(float2 &a0, float2 &a1, float2 &a2, float2 &a3) {
  const float2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = mul_mi(csub(a1, a3));
  a0 = cadd(t0, t2), a1 = cadd(t1, t3), a2 = csub(t0, t2), a3 = csub(t1, t3);
}
template <int R>
__device__ __forceinline__ void butterfly(float2 *v) {
  if constexpr (R == 4) {
    fft4(v[0], v[1], v[2], v[3]);
  } else {
    fft4(v[0], v[2], v[4], v[6]);  // E
    fft4(v[1], v[3], v[5], v[7]);  // O
    constexpr float kHalfSqrt = 0.70710678118654752440f;
    const float2 o1 = make_float2(kHalfSqrt * (v[3].x + v[3].y), kHalfSqrt * (v[3].y - v[3].x));   // O[1] exp(-i pi / 4)
    const float2 o2 = mul_mi(v[5]);                                                                  // O[2] (-i)
    const float2 o3 = make_float2(kHalfSqrt * (v[7].y - v[7].x), kHalfSqrt * (-v[7].y - v[7].x));  // O[3] exp(-3 i pi / 4)
    const float2 e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6], o0 = v[1];
    v[0] = cadd(e0, o0), v[4] = csub(e0, o0);
    v[1] = cadd(e1, o1), v[5] = csub(e1, o1);
    v[2] = cadd(e2, o2), v[6] = csub(e2, o2);
    v[3] = cadd(e3, o3), v[7] = csub(e3, o3);
  }
}

// the passes from sub-transform length 2^LOGNS on, over the wave's batch of G frames: src = the batch's first staged frame (read by the
// first pass only), ex = the wave's region
template <int LOGH, int LOGNS>
__device__ __forceinline__ void fft_passes(const float *src, int fs, const float *__restrict__ win, const float2 *__restrict__ tw, float2 *ex, int lane) {
  constexpr int REM = LOGH - LOGNS, LR = (REM == 2 || REM == 4) ? 2 : 3, R = 1 << LR;
  constexpr int H = 1 << LOGH, M = H > int(kSpectrumBatchPoints) ? H : int(kSpectrumBatchPoints), P = M / 64, NB = P / R;
  constexpr int LHR = LOGH - LR, HR = 1 << LHR, NS = 1 << LOGNS;
  float2 v[NB][R];
#pragma unroll
  for (int q = 0; q < NB; q++) {
    const int b = lane + 64 * q, g = b >> LHR, j = b & (HR - 1);
#pragma unroll
    for (int t = 0; t < R; t++) {
      const int i = j + t * HR;
      if constexpr (LOGNS == 0) {
        const float *f = src + g * fs + 2 * i;
        v[q][t] = make_float2(f[0] * win[2 * i], f[1] * win[2 * i + 1]);
      } else {
        v[q][t] = ex[pad(g * H + i)];
      }
    }
  }
  wave_sync();
#pragma unroll
  for (int q = 0; q < NB; q++) {
    const int b = lane + 64 * q, g = b >> LHR, j = b & (HR - 1), k = j & (NS - 1);
    if constexpr (LOGNS > 0) {
#pragma unroll
      for (int t = 1; t < R; t++) v[q][t] = cmul(v[q][t], tw[(t * k) << (LOGH - LOGNS - LR)]);
    }
    butterfly<R>(v[q]);
    const int base = g * H + (((j >> LOGNS) << (LOGNS + LR)) | k);
#pragma unroll
    for (int t = 0; t < R; t++) ex[pad(base + t * NS)] = v[q][t];
  }
  wave_sync();
  if constexpr (LOGNS + LR < LOGH) fft_passes<LOGH, LOGNS + LR>(src, fs, win, tw, ex, lane);
}

// bin k < bins of frame slot g from the wave's region: the split pass, the mirrored half, the mode.  Complex: (re, im); else (value, -)
template <int LOGH>
__device__ __forceinline__ float2 bin_value(const float2 *ex, const float2 *__restrict__ split, int g, int k, int mode) {
  constexpr int H = 1 << LOGH;
  const int kk = k <= H ? k : 2 * H - k;
  const float2 A = ex[pad(g * H + (kk & (H - 1)))], Z = ex[pad(g * H + ((H - kk) & (H - 1)))], w = split[kk];
  const float er = 0.5f * (A.x + Z.x), ei = 0.5f * (A.y - Z.y), dr = 0.5f * (A.x - Z.x), di = 0.5f * (A.y + Z.y);
  const float p0 = w.x * di, p1 = w.y * dr, p2 = w.y * di, p3 = w.x * dr;
  float re = er + (p0 + p1), im = ei + (p2 - p3);
  if (k > H) im = -im;
  if (mode == kSpectrumComplex) return make_float2(re + 0.f, im + 0.f);
  const float r2 = re * re, i2 = im * im, pw = r2 + i2;
  return make_float2(mode == kSpectrumPower ? pw : sqrtf(pw), 0.f);
}

template <int LOGH>
__global__ __launch_bounds__(kBlock) void spectrum_kernel(const SpectrumArgs a) {
  constexpr int H = 1 << LOGH, N = 2 * H, M = H > int(kSpectrumBatchPoints) ? H : int(kSpectrumBatchPoints), G = M / H, MP = M + M / 32;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *stage = lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float2 *ex0 = reinterpret_cast<float2 *>(lds + a.stage_floats) + wave * (a.bins_major ? a.batches : 1) * MP;
  const bool cplx = a.mode == kSpectrumComplex;
  for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
    const int64_t sig = u / a.runs;
    const int f0 = int(u - sig * a.runs) * a.Fw;
    const float *xs = a.x + sig * a.in_stride;
    // ---- the span of this run, once ----
    if (a.vec4) {
      for (int p = 4 * tid; p < a.span; p += 4 * kBlock) {
        const int64_t gi = a.separate ? int64_t(f0 + (p >> (LOGH + 1))) * a.hop + (p & (N - 1)) : int64_t(f0) * a.hop + p;
        f32x4 q = {0.f, 0.f, 0.f, 0.f};
        if (gi < a.total && (!a.separate || (p & (N - 1)) < a.valid)) q = *reinterpret_cast<const f32x4 *>(xs + gi);
        *reinterpret_cast<f32x4 *>(stage + p) = q;
      }
    } else {
      for (int p = tid; p < a.span; p += kBlock) {
        const int64_t gi = a.separate ? int64_t(f0 + (p >> (LOGH + 1))) * a.hop + (p & (N - 1)) : int64_t(f0) * a.hop + p;
        stage[p] = gi < a.total && (!a.separate || (p & (N - 1)) < a.valid) ? xs[gi] : 0.f;
      }
    }
    __syncthreads();
    // ---- each wave: its batches ----
    const int bins = a.bins;
    for (int q = 0; q < a.batches; q++) {
      const int fb = (q * kSpectrumWaves + wave) * G;  // the batch's first frame, counted from f0
      if (f0 + fb >= a.frames) continue;
      float2 *ex = ex0 + (a.bins_major ? q * MP : 0);
      fft_passes<LOGH, 0>(stage + fb * a.fs, a.fs, a.win, a.tw, ex, lane);
      if (a.bins_major) continue;
      for (int e = lane; e < G * bins; e += 64) {
        const int g = e / bins, k = e - g * bins, f = f0 + fb + g;
        if (f >= a.frames) break;
        const float2 val = bin_value<LOGH>(ex, a.split, g, k, a.mode);
        const int64_t o = (sig * a.frames + f) * bins + k;
        if (cplx) reinterpret_cast<float2 *>(a.y)[o] = val;
        else a.y[o] = val.x;
      }
      wave_sync();
    }
    if (a.bins_major) {
      // ---- bins before frames: through the tile, a chunk of bins at a time ----
      const int fwp = a.Fw + 1, nf = min(a.Fw, a.frames - f0);
      float *tile = stage;
      __syncthreads();  // (every wave is done with the staged span)
      for (int c0 = 0; c0 < bins; c0 += a.tile_bins) {
        const int nb = min(a.tile_bins, bins - c0);
        for (int q = 0; q < a.batches; q++) {
          const int fb = (q * kSpectrumWaves + wave) * G;
          if (f0 + fb >= a.frames) continue;
          const float2 *ex = ex0 + q * MP;
          for (int e = lane; e < G * nb; e += 64) {
            const int g = e / nb, kb = e - g * nb;
            const float2 val = bin_value<LOGH>(ex, a.split, g, c0 + kb, a.mode);
            if (cplx) reinterpret_cast<float2 *>(tile)[kb * fwp + fb + g] = val;
            else tile[kb * fwp + fb + g] = val.x;
          }
        }
        __syncthreads();
        for (int t = tid; t < (nb << a.log_fw); t += kBlock) {
          const int kb = t >> a.log_fw, fl = t & (a.Fw - 1);
          if (fl >= nf) continue;
          const int64_t o = (sig * bins + c0 + kb) * a.frames + f0 + fl;
          if (cplx) reinterpret_cast<float2 *>(a.y)[o] = reinterpret_cast<const float2 *>(tile)[kb * fwp + fl];
          else a.y[o] = tile[kb * fwp + fl];
        }
        __syncthreads();
      }
    } else {
      __syncthreads();  // (the next unit stages over this span)
    }
  }
}

template <int LOGH>
bool launch(hipStream_t s, const SpectrumArgs &a, unsigned grid, size_t lds) {
  auto *kernel = spectrum_kernel<LOGH>;
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)) != hipSuccess) return false;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, a);
  return true;
}

}  // namespace

bool spectrum(hipStream_t s, const float *x, float *y, const SpectrumPack &p, const float *win, const float *tw, const float *split, int64_t rows) {
  const int64_t n = p.n, h = n / 2;
  if (n < kSpectrumMinN || n > kSpectrumMaxN || (n & (n - 1)) != 0 || !win || !tw || !split || p.hop < 1 || p.frames < 1 || p.C < 1 || p.L < 1 ||
      p.bins != (p.onesided ? h + 1 : n) || p.lds_bytes > 160 * 1024 || p.Fw < 1 || (p.Fw & (p.Fw - 1)) != 0 || p.L > INT32_MAX || p.hop > INT32_MAX ||
      (p.stft && (p.frames - 1) * p.hop + n > p.L) || (!p.stft && (p.bins_major || p.hop != n)))
    return false;
  if (rows <= 0) return true;
  SpectrumArgs a;
  a.x = x, a.win = win, a.y = y;
  a.tw = reinterpret_cast<const float2 *>(tw), a.split = reinterpret_cast<const float2 *>(split);
  // DFT: one frame per signal -- the call's rows * C signals are the frames of ONE signal, L apart, each zero beyond min(L, n)
  const int64_t frames = p.stft ? p.frames : rows * p.C, hop = p.stft ? p.hop : p.L;
  if (frames > INT32_MAX) return false;
  a.separate = !p.stft || p.hop >= n;
  a.valid = int(p.stft ? n : std::min(p.L, n));
  a.hop = int(hop), a.frames = int(frames), a.bins = int(p.bins);
  a.runs = int((frames + p.Fw - 1) / p.Fw);
  a.units = (p.stft ? rows * p.C : 1) * a.runs;
  a.in_stride = p.L, a.total = p.stft ? p.L : rows * p.C * p.L;
  a.Fw = p.Fw, a.batches = p.batches, a.fs = int(std::min(p.hop, n)), a.span = int(p.span);
  a.log_fw = __builtin_ctz(unsigned(p.Fw));
  const int64_t M = std::max<int64_t>(h, kSpectrumBatchPoints), Mpad = M + M / 32;
  a.stage_floats = int((p.lds_bytes - 8 * kSpectrumWaves * (p.bins_major ? p.batches : 1) * Mpad) / 4);
  a.mode = p.mode, a.bins_major = p.bins_major;
  a.tile_bins = int(std::max<int64_t>(1, kSpectrumTileFloats / ((p.Fw + 1) * (p.mode == kSpectrumComplex ? 2 : 1))));
  // 16-byte loads: every signal, every run's first sample (separate: every frame) and the signal's end on a 16-byte boundary
  a.vec4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && p.L % 4 == 0 && (a.separate ? hop % 4 == 0 : (int64_t(p.Fw) * p.hop) % 4 == 0);
  const unsigned grid = unsigned(std::min<int64_t>(a.units, kMaxBlocks));
  const size_t lds = size_t(p.lds_bytes);
  switch (__builtin_ctzll(uint64_t(h))) {
    case 2: return launch<2>(s, a, grid, lds);
    case 3: return launch<3>(s, a, grid, lds);
    case 4: return launch<4>(s, a, grid, lds);
    case 5: return launch<5>(s, a, grid, lds);
    case 6: return launch<6>(s, a, grid, lds);
    case 7: return launch<7>(s, a, grid, lds);
    case 8: return launch<8>(s, a, grid, lds);
    case 9: return launch<9>(s, a, grid, lds);
    case 10: return launch<10>(s, a, grid, lds);
    case 11: return launch<11>(s, a, grid, lds);
    default: return false;
  }
}

}  // namespace infera_hip::kern
