// spectrum.hpp -- spectral front ends as one step kind (INTEGRATION.md 2.6 "Spectral front ends"): what the lowering packs
// for a Spectrum step (the ONNX DFT and STFT operators on a real signal) and what its kernel (hip/spectrum.hip) reads.
//   in   [rows, C, L]        real signals, rows first, flat in their buffer (C = 1 for STFT)
//   out  frame f of a signal is samples [f * hop, f * hop + n), zero beyond L (DFT: one frame, padded or truncated to n), times the window;
//        X[k] = sum_j frame[j] exp(-2 pi i j k / n) for k < bins (bins = n / 2 + 1 onesided, else n), written as
//          complex    (re, im) interleaved      power  fl(fl(re re) + fl(im im))      magnitude  sqrtf(power)
//        in the layout [rows, C, frames, bins (, 2)] or, bins_major, [rows, C, bins, frames (, 2)].
// n is in [kSpectrumMinN, kSpectrumMaxN]: a power of two (DFT and STFT), or for STFT any even n whose half h = 2^a 3^b 5^c (the mixed-radix
// kernel).  An STFT may stand for a Pad of the time axis in front of it (torch.stft(center=True)): frame f is then samples
// [f * hop, f * hop + n) of the PADDED signal, padded index i reading sample s = i - pad_left of the signal -- reflect: s < 0 -> -s,
// s >= L -> 2 (L - 1) - s; constant: zero outside [0, L).  The tables are computed in float64 and rounded to f32 once.
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace infera_hip {

constexpr int64_t kSpectrumMinN = 8, kSpectrumMaxN = 4096;
constexpr int kSpectrumWaves = 4;                    // waves of a work group: each transforms one batch of frames at a time
constexpr int64_t kSpectrumBatchPoints = 512;        // complex points a wave transforms side by side: at least this many (8 per lane)
constexpr int64_t kSpectrumStageFloats = 8192;       // the staged span a work group aims for (it takes what one batch per wave needs at least)
constexpr int64_t kSpectrumTileFloats = 8192;        // bins_major: the transposing tile
constexpr int64_t kSpectrumMaxKeep = 2048;           // bins_major: complex points a wave keeps in its exchange region until the tile has taken them

constexpr int kSpectrumMaxPasses = 8;                // passes of a mixed-radix schedule (h = 1458 = 2 * 3^6 needs 7)

enum SpectrumMode : int { kSpectrumComplex = 0, kSpectrumPower = 1, kSpectrumMagnitude = 2 };
enum SpectrumPad : int { kSpectrumPadNone = 0, kSpectrumPadConstant = 1, kSpectrumPadReflect = 2 };

// One pass of the mixed-radix transform: radix R over sub-transforms of length ns; hr = h / R butterflies per frame; tws = h / (ns R), the
// table stride of the pass.  b / hr and j / ns are taken as (b * magic) >> 32, magic = floor(2^32 / d) + 1: exact for b < 2^32 / d, and b,
// d <= 2048 here (d = 1 needs no division).
struct SpectrumPass {
  int radix = 0, ns = 0, hr = 0, tws = 0;
  uint32_t magic_ns = 0, magic_hr = 0;
};

struct SpectrumPack {
  // geometry
  int64_t L = 0, C = 1, n = 0, hop = 0, frames = 1, bins = 0;
  bool onesided = true, bins_major = false, stft = false;
  bool rank4 = false;  // DFT: the input has a channel axis, [N, C, L, 1]
  int mode = kSpectrumComplex;
  int64_t pad_left = 0, pad_right = 0;  // STFT: the absorbed Pad of the time axis (L is the unpadded length)
  int pad_mode = kSpectrumPadNone;
  int64_t padded() const { return L + pad_left + pad_right; }
  // tables (pack_spectrum)
  std::vector<float> window;   // [n]; ones without a window
  std::vector<float> twiddle;  // [n / 2][2]: exp(-2 pi i m / (n / 2)), the n/2-point transform's
  std::vector<float> split;    // [n / 2 + 1][2]: exp(-2 pi i k / n), the real-split pass's
  // launch shape (pack_spectrum): frames a wave transforms side by side, batches per wave, frames per work group
  int per_wave = 1, batches = 1, Fw = 4;
  int64_t span = 0;            // staged floats of a work group
  int64_t lds_bytes = 0;
  std::string form;            // the radix schedule and the frames per wave, e.g. "8.8.4/2", mixed "5.5.8/3"
  std::vector<SpectrumPass> passes;  // n / 2 not a power of two: the mixed-radix schedule (else empty: the kernel per log2(n / 2))
  int64_t out_per_signal() const { return frames * bins * (mode == kSpectrumComplex ? 2 : 1); }
};

// why this geometry cannot be served ("" = it can): n in range and a power of two, or for STFT even with n / 2 = 2^a 3^b 5^c; the result
// within 2^31 elements per row
std::string spectrum_refusal(bool stft, int64_t n, int64_t C, int64_t frames, int64_t bins, bool complex_out);

// fills the tables and the launch shape from the geometry (window: empty = rectangular, else n values)
void pack_spectrum(SpectrumPack &p);

// the radix schedule of the h-point complex transform, h = 2^log_h, log_h in [2, 11]: passes of radix 8 and 4 ("8.8.4")
std::string spectrum_schedule(int log_h);
// the radices of the h-point transform for any h = 2^a 3^b 5^c: the 5s, then the 3s, then the 8s and 4s of spectrum_schedule(a), or a lone 2
// last when a = 1 (the odd radices first: their passes then run at the small sub-transform lengths, where the table stride is large)
std::vector<int> spectrum_radices(int64_t h);

}  // namespace infera_hip
