// spectrum.hpp -- spectral front ends as one step kind (INTEGRATION.md 2.6 "Spectral front ends"): what the lowering packs
// for a Spectrum step (the ONNX DFT and STFT operators on a real signal) and what its kernel (hip/spectrum.hip) reads.
//   in   [rows, C, L]        real signals, rows first, flat in their buffer (C = 1 for STFT)
//   out  frame f of a signal is samples [f * hop, f * hop + n), zero beyond L (DFT: one frame, padded or truncated to n), times the window;
//        X[k] = sum_j frame[j] exp(-2 pi i j k / n) for k < bins (bins = n / 2 + 1 onesided, else n), written as
//          complex    (re, im) interleaved      power  fl(fl(re re) + fl(im im))      magnitude  sqrtf(power)
//        in the layout [rows, C, frames, bins (, 2)] or, bins_major, [rows, C, bins, frames (, 2)].
// n is a power of two in [kSpectrumMinN, kSpectrumMaxN].  The tables are computed in float64 and rounded to f32 once.
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

enum SpectrumMode : int { kSpectrumComplex = 0, kSpectrumPower = 1, kSpectrumMagnitude = 2 };

struct SpectrumPack {
  // geometry
  int64_t L = 0, C = 1, n = 0, hop = 0, frames = 1, bins = 0;
  bool onesided = true, bins_major = false, stft = false;
  bool rank4 = false;  // DFT: the input has a channel axis, [N, C, L, 1]
  int mode = kSpectrumComplex;
  // tables (pack_spectrum)
  std::vector<float> window;   // [n]; ones without a window
  std::vector<float> twiddle;  // [n / 2][2]: exp(-2 pi i m / (n / 2)), the n/2-point transform's
  std::vector<float> split;    // [n / 2 + 1][2]: exp(-2 pi i k / n), the real-split pass's
  // launch shape (pack_spectrum): frames a wave transforms side by side, batches per wave, frames per work group
  int per_wave = 1, batches = 1, Fw = 4;
  int64_t span = 0;            // staged floats of a work group
  int64_t lds_bytes = 0;
  std::string form;            // the radix schedule and the frames per wave, e.g. "8.8.4/2"
  int64_t out_per_signal() const { return frames * bins * (mode == kSpectrumComplex ? 2 : 1); }
};

// why this geometry cannot be served ("" = it can): n a power of two in range, the result within 2^31 elements per row
std::string spectrum_refusal(int64_t n, int64_t C, int64_t frames, int64_t bins, bool complex_out);

// fills the tables and the launch shape from the geometry (window: empty = rectangular, else n values)
void pack_spectrum(SpectrumPack &p);

// the radix schedule of the h-point complex transform, h = 2^log_h, log_h in [2, 11]: passes of radix 8 and 4 ("8.8.4")
std::string spectrum_schedule(int log_h);

}  // namespace infera_hip
