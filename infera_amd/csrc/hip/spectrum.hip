// spectrum.hip -- the Spectrum step (INTEGRATION.md section 2.6 "Spectral front ends"): the ONNX DFT and STFT operators on
// real signals x [rows, C, L] -- framing, window, an n-point real transform per frame, and complex / power / magnitude results in either
// layout, in one launch.  n = 2 h in [8, 4096].  For a power of two the kernel is instantiated per log2(h); any other h = 2^a 3^b 5^c (STFT
// only) runs the MIXED-RADIX instantiations at the end of this header, on the same work split, staging, split pass and epilogue.
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
// Centred frames.  An STFT may stand for the Pad in front of it (pad_left, pad_right, reflect or zeros): frames are then counted on the padded
//   signal.  A run whose span lies inside the signal is staged as ever, from a start shifted by pad_left (16-byte loads where that start is
//   aligned too); a run at either edge is staged by word loads through the index map (padded_sample).  Either way a staged sample is a bit
//   copy, so a centred model gives the bits of the un-centred model on the explicitly padded signal.
// Mixed radix (spectrum_kernel<-16>, <-32>: at most 16 / 32 points per lane).  h, Ns and h / R are run-time values; the radix of a pass is
//   compile-time and dispatched per pass from the table in the kernel arguments (radices 5, 3, 8, 4, 2 in the order of host
//   spectrum_radices).  A batch is G = ceil(512 / h) frames, M = G h points, M / R butterflies per pass dealt to the lanes 64 apart, the
//   tail lanes guarded.  b / (h / R) and j / Ns are (b * magic) >> 32 with the host's per-pass reciprocals -- exact for these ranges (host/
//   spectrum.hpp), checked for every served (h, pass) by tests/test_spectrum_mixed.py -- so a pass has no integer division.  Exchange: as
//   above, ONE region per wave, all of the wave's points read into registers before any is written; the register arrays are sized by the
//   compile-time bound on the points per lane, so they index statically.  Chosen over two ping-pong regions because it halves the exchange
//   LDS (bins_major keeps up to 2048 points per wave until the tile takes them), which is what keeps lds_bytes under 160 KiB at n = 4050.
//   G need not be a power of two but Fw is (the tile indexes by log_fw): the slots of the last batch behind Fw stay idle.  The a + a / 32
//   padding is kept; with strides that are no powers of two its conflicts are NOT measured.
//   Radix 3: t = a1 + a2, X0 = a0 + t, m = a0 - t / 2, X1,2 = m -+ i (sqrt 3 / 2)(a1 - a2).  Radix 5: t1 = a1 + a4, t2 = a2 + a3, t5 = t1 + t2,
//   X0 = a0 + t5, m = a0 - t5 / 4, d = (sqrt 5 / 4)(t1 - t2), X1,4 = (m + d) -+ i (s1 u1 + s2 u2), X2,3 = (m - d) -+ i (s2 u1 - s1 u2), u1 = a1 -
//   a4, u2 = a2 - a3, s1,2 = sin(2 pi / 5), sin(4 pi / 5): equal inputs give m = d = u = 0 exactly, so a frame of ones has one non-zero bin.
// Every value is a fixed sequence of separately rounded f32 operations (contraction is off) that depends on the model and the frame's own
// samples only: not on Fw, the frame's slot in its batch, the grid or the rows around it.  No atomics.  64-bit element offsets.
#include "device_common.hpp"

#include <algorithm>
#include <type_traits>

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
  int pad_mode, pad_left, pad_right;  // the absorbed Pad (host/spectrum.hpp SpectrumPad); `total` stays the unpadded length
};
// what the mixed-radix instantiations read besides: run-time h, frames per batch and the pass table (the power-of-two kernels do not carry it)
struct MixedArgs : SpectrumArgs {
  int h, G, npass;
  SpectrumPass pass[kSpectrumMaxPasses];
};
template <int LOGH>
using ArgsOf = std::conditional_t<(LOGH < 0), MixedArgs, SpectrumArgs>;

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
  if constexpr (R == 2) {
    const float2 a0 = v[0], a1 = v[1];
    v[0] = cadd(a0, a1), v[1] = csub(a0, a1);
  } else if constexpr (R == 3) {
    constexpr float kS = 0.86602540378443864676f;  // sqrt(3) / 2
    const float2 t = cadd(v[1], v[2]), d = csub(v[1], v[2]);
    const float2 m = make_float2(v[0].x - 0.5f * t.x, v[0].y - 0.5f * t.y), e = make_float2(kS * d.y, kS * d.x);
    v[0] = cadd(v[0], t);
    v[1] = make_float2(m.x + e.x, m.y - e.y), v[2] = make_float2(m.x - e.x, m.y + e.y);
  } else if constexpr (R == 5) {
    constexpr float kD = 0.55901699437494742410f, kS1 = 0.95105651629515357212f, kS2 = 0.58778525229247312917f;  // sqrt(5) / 4, sin(2 pi / 5), sin(4 pi / 5)
    const float2 t1 = cadd(v[1], v[4]), t2 = cadd(v[2], v[3]), u1 = csub(v[1], v[4]), u2 = csub(v[2], v[3]);
    const float2 t5 = cadd(t1, t2), dt = csub(t1, t2);
    const float2 m = make_float2(v[0].x - 0.25f * t5.x, v[0].y - 0.25f * t5.y), d = make_float2(kD * dt.x, kD * dt.y);
    const float2 p = cadd(m, d), q = csub(m, d);
    const float a1x = kS1 * u1.x, a1y = kS1 * u1.y, a2x = kS2 * u2.x, a2y = kS2 * u2.y, b1x = kS2 * u1.x, b1y = kS2 * u1.y, b2x = kS1 * u2.x, b2y = kS1 * u2.y;
    const float2 e = make_float2(a1x + a2x, a1y + a2y), f = make_float2(b1x - b2x, b1y - b2y);  // X1,4 = p -+ i e, X2,3 = q -+ i f
    v[0] = cadd(v[0], t5);
    v[1] = make_float2(p.x + e.y, p.y - e.x), v[4] = make_float2(p.x - e.y, p.y + e.x);
    v[2] = make_float2(q.x + f.y, q.y - f.x), v[3] = make_float2(q.x - f.y, q.y + f.x);
  } else if constexpr (R == 4) {
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
// (LOGH < 0: h at run time, and Z[k mod h], Z[(h - k) mod h] by selects instead of masks)
template <int LOGH>
__device__ __forceinline__ float2 bin_value(const int h, const float2 *ex, const float2 *__restrict__ split, int g, int k, int mode) {
  const int H = LOGH < 0 ? h : 1 << (LOGH < 0 ? 0 : LOGH);
  const int kk = k <= H ? k : 2 * H - k;
  const int i0 = LOGH < 0 ? (kk == H ? 0 : kk) : (kk & (H - 1)), i1 = LOGH < 0 ? (kk == 0 ? 0 : H - kk) : ((H - kk) & (H - 1));
  const float2 A = ex[pad(g * H + i0)], Z = ex[pad(g * H + i1)], w = split[kk];
  const float er = 0.5f * (A.x + Z.x), ei = 0.5f * (A.y - Z.y), dr = 0.5f * (A.x - Z.x), di = 0.5f * (A.y + Z.y);
  const float p0 = w.x * di, p1 = w.y * dr, p2 = w.y * di, p3 = w.x * dr;
  float re = er + (p0 + p1), im = ei + (p2 - p3);
  if (k > H) im = -im;
  if (mode == kSpectrumComplex) return make_float2(re + 0.f, im + 0.f);
  const float r2 = re * re, i2 = im * im, pw = r2 + i2;
  return make_float2(mode == kSpectrumPower ? pw : sqrtf(pw), 0.f);
}

// ---- the mixed-radix passes: h = 2^a 3^b 5^c at run time (the header's "Mixed radix") ----
__device__ __forceinline__ int div_by(int b, int d, unsigned magic) { return d == 1 ? b : int(__umulhi(unsigned(b), magic)); }

// one pass of radix R over the wave's batch: nbf = G h / R butterflies, butterfly b = lane + 64 q; gmax: the batch's frame slots that are
// staged (the others transform zeros); PMAX: the compile-time bound on the points per lane
template <int R, int PMAX>
__device__ __forceinline__ void mixed_pass(const SpectrumPass &ps, int h, int nbf, int gmax, const float *src, int fs, const float *__restrict__ win,
                                           const float2 *__restrict__ tw, float2 *ex, int lane) {
  constexpr int NB = (PMAX + R - 1) / R;
  const bool first = ps.ns == 1;
  float2 v[NB][R];
#pragma unroll
  for (int q = 0; q < NB; q++) {
    const int b = lane + 64 * q;
    if (b < nbf) {
      const int g = div_by(b, ps.hr, ps.magic_hr), j = b - g * ps.hr;
#pragma unroll
      for (int t = 0; t < R; t++) {
        const int i = j + t * ps.hr;
        if (first) {
          const float *f = src + g * fs + 2 * i;
          v[q][t] = g < gmax ? make_float2(f[0] * win[2 * i], f[1] * win[2 * i + 1]) : make_float2(0.f, 0.f);
        } else {
          v[q][t] = ex[pad(g * h + i)];
        }
      }
    }
  }
  wave_sync();
#pragma unroll
  for (int q = 0; q < NB; q++) {
    const int b = lane + 64 * q;
    if (b < nbf) {
      const int g = div_by(b, ps.hr, ps.magic_hr), j = b - g * ps.hr, jn = div_by(j, ps.ns, ps.magic_ns), k = j - jn * ps.ns;
      if (!first) {
#pragma unroll
        for (int t = 1; t < R; t++) v[q][t] = cmul(v[q][t], tw[t * k * ps.tws]);
      }
      butterfly<R>(v[q]);
      const int base = g * h + jn * ps.ns * R + k;
#pragma unroll
      for (int t = 0; t < R; t++) ex[pad(base + t * ps.ns)] = v[q][t];
    }
  }
  wave_sync();
}

template <int PMAX>
__device__ __forceinline__ void mixed_passes(const MixedArgs &a, const float *src, int gmax, float2 *ex, int lane) {
  for (int i = 0; i < a.npass; i++) {
    const SpectrumPass ps = a.pass[i];
    const int nbf = a.G * ps.hr;
    switch (ps.radix) {
      case 8: mixed_pass<8, PMAX>(ps, a.h, nbf, gmax, src, a.fs, a.win, a.tw, ex, lane); break;
      case 5: mixed_pass<5, PMAX>(ps, a.h, nbf, gmax, src, a.fs, a.win, a.tw, ex, lane); break;
      case 4: mixed_pass<4, PMAX>(ps, a.h, nbf, gmax, src, a.fs, a.win, a.tw, ex, lane); break;
      case 3: mixed_pass<3, PMAX>(ps, a.h, nbf, gmax, src, a.fs, a.win, a.tw, ex, lane); break;
      default: mixed_pass<2, PMAX>(ps, a.h, nbf, gmax, src, a.fs, a.win, a.tw, ex, lane); break;
    }
  }
}

// the staged float p of a separately staged run -> (frame of the run, offset in the frame): shift and mask for a power of two, else one
// division per thread and run, then carried along the thread's stride
template <int LOGH>
struct FrameIndex {
  int n, fr = 0, off = 0, sf = 0, so = 0;
  __device__ __forceinline__ FrameIndex(int n_, int p, int step) : n(n_) {
    if constexpr (LOGH < 0) fr = p / n, off = p - fr * n, sf = step / n, so = step - sf * n;
  }
  __device__ __forceinline__ void at(int p) {
    if constexpr (LOGH >= 0) fr = p >> (LOGH + 1), off = p & ((2 << LOGH) - 1);
  }
  __device__ __forceinline__ void next() {
    if constexpr (LOGH < 0) {
      off += so, fr += sf;
      if (off >= n) off -= n, fr++;
    }
  }
};

// sample i of the PADDED signal xs[0, L): the index map of an absorbed Pad; zero beyond the padded signal (frames that do not exist)
__device__ __forceinline__ float padded_sample(const float *__restrict__ xs, int64_t i, const SpectrumArgs &a) {
  if (i >= a.total + a.pad_left + a.pad_right) return 0.f;
  int64_t s = i - a.pad_left;
  if (s < 0 || s >= a.total) {
    if (a.pad_mode != kSpectrumPadReflect) return 0.f;
    s = s < 0 ? -s : 2 * (a.total - 1) - s;
  }
  return xs[s];
}

// LOGH >= 2: n = 2^(LOGH + 1).  LOGH = -16, -32: the mixed-radix kernel with at most 16 / 32 points per lane.  PAD: the step stands for a Pad
// (its own instantiations, so that a model without one runs the code it ran before)
template <int LOGH, bool PAD>
__global__ __launch_bounds__(kBlock) void spectrum_kernel(const ArgsOf<LOGH> a) {
  constexpr bool kMixed = LOGH < 0;
  constexpr int HC = kMixed ? 0 : 1 << (kMixed ? 0 : LOGH), MC = HC > int(kSpectrumBatchPoints) ? HC : int(kSpectrumBatchPoints);
  int H = HC, G = MC / (kMixed ? 1 : HC);
  if constexpr (kMixed) H = a.h, G = a.G;
  const int N = 2 * H, M = G * H, MP = M + M / 32;
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
    // an absorbed Pad shifts the signal by pad_left under the staged span; a run that leaves the signal on either side goes through the map
    bool through_map = false;
    if constexpr (PAD) {
      const int64_t first = int64_t(f0) * a.hop - a.pad_left, reach = a.separate ? int64_t(a.Fw - 1) * a.hop + N : int64_t(a.span);
      through_map = first < 0 || first + reach > a.total;
    }
    if (through_map) {
      FrameIndex<LOGH> fi(N, tid, kBlock);
      for (int p = tid; p < a.span; p += kBlock, fi.next()) {
        fi.at(p);
        stage[p] = padded_sample(xs, a.separate ? int64_t(f0 + fi.fr) * a.hop + fi.off : int64_t(f0) * a.hop + p, a);
      }
    } else if (a.vec4) {
      FrameIndex<LOGH> fi(N, 4 * tid, 4 * kBlock);
      for (int p = 4 * tid; p < a.span; p += 4 * kBlock, fi.next()) {
        fi.at(p);
        const int64_t gi = (a.separate ? int64_t(f0 + fi.fr) * a.hop + fi.off : int64_t(f0) * a.hop + p) - (PAD ? a.pad_left : 0);
        f32x4 q = {0.f, 0.f, 0.f, 0.f};
        if (gi < a.total && (!a.separate || fi.off < a.valid)) q = *reinterpret_cast<const f32x4 *>(xs + gi);
        *reinterpret_cast<f32x4 *>(stage + p) = q;
      }
    } else {
      FrameIndex<LOGH> fi(N, tid, kBlock);
      for (int p = tid; p < a.span; p += kBlock, fi.next()) {
        fi.at(p);
        const int64_t gi = (a.separate ? int64_t(f0 + fi.fr) * a.hop + fi.off : int64_t(f0) * a.hop + p) - (PAD ? a.pad_left : 0);
        stage[p] = gi < a.total && (!a.separate || fi.off < a.valid) ? xs[gi] : 0.f;
      }
    }
    __syncthreads();
    // ---- each wave: its batches ----
    const int bins = a.bins;
    for (int q = 0; q < a.batches; q++) {
      const int fb = (q * kSpectrumWaves + wave) * G;  // the batch's first frame, counted from f0
      if (f0 + fb >= a.frames || (kMixed && fb >= a.Fw)) continue;  // (mixed: the last batch may begin behind Fw)
      float2 *ex = ex0 + (a.bins_major ? q * MP : 0);
      if constexpr (kMixed) mixed_passes<-LOGH>(a, stage + fb * a.fs, min(G, a.Fw - fb), ex, lane);
      else fft_passes<LOGH, 0>(stage + fb * a.fs, a.fs, a.win, a.tw, ex, lane);
      if (a.bins_major) continue;
      for (int e = lane; e < G * bins; e += 64) {
        const int g = e / bins, k = e - g * bins, f = f0 + fb + g;
        if (f >= a.frames || (kMixed && fb + g >= a.Fw)) break;
        const float2 val = bin_value<LOGH>(H, ex, a.split, g, k, a.mode);
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
          if (f0 + fb >= a.frames || (kMixed && fb >= a.Fw)) continue;
          const float2 *ex = ex0 + q * MP;
          const int ng = kMixed ? min(G, a.Fw - fb) : G;  // (mixed: the slots behind Fw have no column in the tile)
          for (int e = lane; e < ng * nb; e += 64) {
            const int g = e / nb, kb = e - g * nb;
            const float2 val = bin_value<LOGH>(H, ex, a.split, g, c0 + kb, a.mode);
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

template <int LOGH, bool PAD>
bool launch_as(hipStream_t s, const ArgsOf<LOGH> &a, unsigned grid, size_t lds) {
  auto *kernel = spectrum_kernel<LOGH, PAD>;
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)) != hipSuccess) return false;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, a);
  return true;
}
template <int LOGH>
bool launch(hipStream_t s, const ArgsOf<LOGH> &a, unsigned grid, size_t lds) {
  return a.pad_mode != kSpectrumPadNone ? launch_as<LOGH, true>(s, a, grid, lds) : launch_as<LOGH, false>(s, a, grid, lds);
}

}  // namespace

bool spectrum(hipStream_t s, const float *x, float *y, const SpectrumPack &p, const float *win, const float *tw, const float *split, int64_t rows) {
  const int64_t n = p.n, h = n / 2;
  const bool mixed = (h & (h - 1)) != 0, padded = p.pad_mode != kSpectrumPadNone;
  if (n < kSpectrumMinN || n > kSpectrumMaxN || n % 2 || !win || !tw || !split || p.hop < 1 || p.frames < 1 || p.C < 1 || p.L < 1 ||
      p.bins != (p.onesided ? h + 1 : n) || p.lds_bytes > 160 * 1024 || p.Fw < 1 || (p.Fw & (p.Fw - 1)) != 0 || p.L > INT32_MAX || p.hop > INT32_MAX ||
      p.pad_left < 0 || p.pad_right < 0 || p.padded() > INT32_MAX || (!padded && (p.pad_left || p.pad_right)) ||
      (p.pad_mode == kSpectrumPadReflect && (p.pad_left >= p.L || p.pad_right >= p.L)) ||
      (p.stft && (p.frames - 1) * p.hop + n > p.padded()) || (!p.stft && (p.bins_major || p.hop != n || mixed || padded)))
    return false;
  const int64_t G = p.per_wave, M = G * h, Mpad = M + M / 32;
  if (mixed) {
    // the schedule the kernel trusts: its radices multiply to h, its batch is within the points a lane can hold, its slots cover Fw
    int64_t prod = 1;
    for (const SpectrumPass &ps : p.passes) {
      if ((ps.radix != 2 && ps.radix != 3 && ps.radix != 4 && ps.radix != 5 && ps.radix != 8) || ps.ns != prod || ps.hr * ps.radix != h || int64_t(ps.tws) * ps.ns * ps.radix != h) return false;
      prod *= ps.radix;
    }
    if (prod != h || p.passes.size() > size_t(kSpectrumMaxPasses) || G != (kSpectrumBatchPoints + h - 1) / h || M > 2048) return false;
  } else if (G != std::max<int64_t>(h, kSpectrumBatchPoints) / h) {
    return false;
  }
  const int64_t keep = p.bins_major ? p.batches : 1, stage_floats = (p.lds_bytes - 8 * kSpectrumWaves * keep * Mpad) / 4;
  if (p.batches < 1 || int64_t(p.batches) * kSpectrumWaves * G < p.Fw || stage_floats < ((p.span + 3) / 4) * 4) return false;
  if (rows <= 0) return true;
  MixedArgs a;
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
  a.stage_floats = int(stage_floats);
  a.mode = p.mode, a.bins_major = p.bins_major;
  a.pad_mode = p.pad_mode, a.pad_left = int(p.pad_left), a.pad_right = int(p.pad_right);
  a.h = int(h), a.G = int(G), a.npass = int(p.passes.size());
  for (size_t i = 0; i < p.passes.size(); i++) a.pass[i] = p.passes[i];
  a.tile_bins = int(std::max<int64_t>(1, kSpectrumTileFloats / ((p.Fw + 1) * (p.mode == kSpectrumComplex ? 2 : 1))));
  // 16-byte loads: every signal, every run's first sample (separate: every frame, in the signal and in the staged span) and the signal's end on
  // a 16-byte boundary
  a.vec4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && p.L % 4 == 0 && p.pad_left % 4 == 0 && (a.separate ? hop % 4 == 0 && n % 4 == 0 : (int64_t(p.Fw) * p.hop) % 4 == 0);
  const unsigned grid = unsigned(std::min<int64_t>(a.units, kMaxBlocks));
  const size_t lds = size_t(p.lds_bytes);
  if (mixed) return M <= 1024 ? launch<-16>(s, a, grid, lds) : launch<-32>(s, a, grid, lds);
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
