// spectrum.cpp -- the tables and the launch shape of a Spectrum step (host/spectrum.hpp).
#include "spectrum.hpp"

#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace infera_hip {

namespace {

// exp(-2 pi i k / n) in float64 with the exact values on the axes and equal parts on the diagonals: the angle is reduced to [0, pi / 4]
// first, so that a frame of ones, a zero row and the Nyquist bin come out exactly
void unit_root(int64_t k, int64_t n, double *re, double *im) {
  k %= n;
  const int64_t quarter = n / 4;  // (n >= 4)
  const int64_t q = k / quarter, r = k % quarter;
  double c = 1.0, s = 0.0;
  if (r != 0) {
    const double pi = 3.14159265358979323846;
    if (8 * r == n) c = s = std::sqrt(0.5);
    else if (8 * r < n) c = std::cos(2.0 * pi * double(r) / double(n)), s = std::sin(2.0 * pi * double(r) / double(n));
    else c = std::sin(2.0 * pi * double(quarter - r) / double(n)), s = std::cos(2.0 * pi * double(quarter - r) / double(n));
  }
  // exp(-i (q pi / 2 + a)) = (-i)^q (c - i s)
  switch (q) {
    case 0: *re = c, *im = -s; break;
    case 1: *re = -s, *im = -c; break;
    case 2: *re = -c, *im = s; break;
    default: *re = s, *im = c; break;
  }
}

int log2_of(int64_t v) {
  int l = 0;
  while ((int64_t(1) << l) < v) l++;
  return l;
}

}  // namespace

std::string spectrum_schedule(int log_h) {
  std::string s;
  for (int rem = log_h; rem > 0;) {
    const int r = (rem == 2 || rem == 4) ? 2 : 3;
    s += (s.empty() ? "" : ".") + std::to_string(1 << r);
    rem -= r;
  }
  return s;
}

std::string spectrum_refusal(int64_t n, int64_t C, int64_t frames, int64_t bins, bool complex_out) {
  if (n < 1 || (n & (n - 1)) != 0) return "a transform length of " + std::to_string(n) + " is not a power of two (not supported yet)";
  if (n < kSpectrumMinN) return "a transform length of " + std::to_string(n) + " is below " + std::to_string(kSpectrumMinN);
  if (n > kSpectrumMaxN) return "a transform length of " + std::to_string(n) + " is above " + std::to_string(kSpectrumMaxN);
  int64_t per_row = 0;
  if (__builtin_mul_overflow(C, frames, &per_row) || __builtin_mul_overflow(per_row, bins * (complex_out ? 2 : 1), &per_row) || per_row > (int64_t(1) << 31))
    return "its result has more than 2^31 elements per row";
  return "";
}

void pack_spectrum(SpectrumPack &p) {
  const int64_t n = p.n, h = n / 2;
  if (p.window.empty()) p.window.assign(size_t(n), 1.f);
  p.twiddle.resize(size_t(2 * h));
  for (int64_t m = 0; m < h; m++) {
    double re, im;
    unit_root(m, h, &re, &im);
    p.twiddle[size_t(2 * m)] = float(re), p.twiddle[size_t(2 * m + 1)] = float(im);
  }
  p.split.resize(size_t(2 * (h + 1)));
  for (int64_t k = 0; k <= h; k++) {
    double re, im;
    unit_root(k, n, &re, &im);
    p.split[size_t(2 * k)] = float(re), p.split[size_t(2 * k + 1)] = float(im);
  }
  // the launch shape: a wave transforms `per_wave` frames side by side (at least kSpectrumBatchPoints complex points: 8 per lane), a work
  // group `batches` such batches per wave over one staged span
  const int64_t M = std::max(h, kSpectrumBatchPoints), G = M / h, round = kSpectrumWaves * G, s = std::min(p.hop, n);
  const int64_t rounds_all = p.stft ? (p.frames + round - 1) / round : INT64_MAX;  // (DFT: the call's signals are the frames)
  int64_t k;
  if (p.bins_major) k = std::max<int64_t>(1, std::min(4 / G, kSpectrumMaxKeep / M));  // (the wave keeps them all until the tile takes them)
  else k = std::max<int64_t>(1, std::min<int64_t>(((kSpectrumStageFloats - n) / s + 1) / round, 64));
  k = std::min(k, rounds_all);
  while (k & (k - 1)) k &= k - 1;  // (a power of two: so is Fw)
  p.per_wave = int(G), p.batches = int(k), p.Fw = int(round * k);
  p.span = (int64_t(p.Fw) - 1) * s + n;
  const int64_t Mpad = M + M / 32;
  const int64_t stage = ((std::max(p.span, p.bins_major ? kSpectrumTileFloats : int64_t(0)) + 3) / 4) * 4;
  p.lds_bytes = 4 * stage + 8 * kSpectrumWaves * (p.bins_major ? k : 1) * Mpad;
  p.form = spectrum_schedule(log2_of(h)) + "/" + std::to_string(G);
}

}  // namespace infera_hip
