// spectrum.cpp -- the tables and the launch shape of a Spectrum step (host/spectrum.hpp).
#include "spectrum.hpp"

#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace infera_hip {

namespace {

// exp(-2 pi i k / n) in float64 for any n >= 1, with the exact values on the axes (n | 4 k) and equal parts on the diagonals (n | 8 k, odd
// quotient): the angle is reduced to [0, pi / 4] in integers first, so that a frame of ones, a zero row and the Nyquist bin come out exactly.
// Both halves of a quadrant take cos and sin of the SAME float64 argument, so T[n - m] = conj T[m] bit for bit.  (For 4 | n the argument is
// 2 pi (k mod n/4) / n scaled by 4 / 4: the values of the power-of-two tables are unchanged.)
void unit_root(int64_t k, int64_t n, double *re, double *im) {
  k %= n;
  const int64_t q = 4 * k / n, r = 4 * k - q * n;  // the quadrant, and the angle in it as r / (4 n) of a turn
  double c = 1.0, s = 0.0;
  if (r != 0) {
    const double pi = 3.14159265358979323846;
    if (2 * r == n) c = s = std::sqrt(0.5);
    else if (2 * r < n) c = std::cos(2.0 * pi * double(r) / double(4 * n)), s = std::sin(2.0 * pi * double(r) / double(4 * n));
    else c = std::sin(2.0 * pi * double(n - r) / double(4 * n)), s = std::cos(2.0 * pi * double(n - r) / double(4 * n));
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

std::vector<int> spectrum_radices(int64_t h) {
  std::vector<int> r;
  int a = 0;
  while (h % 5 == 0) r.push_back(5), h /= 5;
  while (h % 3 == 0) r.push_back(3), h /= 3;
  while (h % 2 == 0) a++, h /= 2;
  if (h != 1) return {};
  for (int rem = a; rem > 1;) {
    const int l = (rem == 2 || rem == 4) ? 2 : 3;
    r.push_back(1 << l);
    rem -= l;
  }
  if (a == 1) r.push_back(2);
  return r;
}

std::string spectrum_refusal(bool stft, int64_t n, int64_t C, int64_t frames, int64_t bins, bool complex_out) {
  const bool pow2 = n >= 1 && (n & (n - 1)) == 0;
  if (!stft && !pow2) return "a transform length of " + std::to_string(n) + " is not a power of two (not supported yet)";
  if (n < kSpectrumMinN) return "a transform length of " + std::to_string(n) + " is below " + std::to_string(kSpectrumMinN);
  if (n > kSpectrumMaxN) return "a transform length of " + std::to_string(n) + " is above " + std::to_string(kSpectrumMaxN);
  if (!pow2) {
    if (n % 2) return "a frame length of " + std::to_string(n) + " is odd (only even lengths)";
    int64_t rest = n / 2;
    for (int64_t f : {2, 3, 5})
      while (rest % f == 0) rest /= f;
    if (rest != 1) {
      int64_t f = 7;
      while (rest % f) f++;
      return "half the frame length of " + std::to_string(n) + " has the prime factor " + std::to_string(f) + " (only 2, 3 and 5)";
    }
  }
  int64_t per_row = 0;
  if (__builtin_mul_overflow(C, frames, &per_row) || __builtin_mul_overflow(per_row, bins * (complex_out ? 2 : 1), &per_row) || per_row > (int64_t(1) << 31))
    return "its result has more than 2^31 elements per row";
  return "";
}

void pack_spectrum(SpectrumPack &p) {
  const int64_t n = p.n, h = n / 2;
  const bool mixed = (h & (h - 1)) != 0;
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
  // what the kernel's exact results rest on: the axis points are 0 and +-1 and the diagonal points +-fl(sqrt 1/2) in both parts (any n);
  // T[h - m] = conj T[m] bit for bit, and split[h - k] = (-re, im) of split[k]
  const float diag = float(std::sqrt(0.5));
  for (int64_t k = 0; k <= h; k++) {
    const float re = std::fabs(p.split[size_t(2 * k)]), im = std::fabs(p.split[size_t(2 * k + 1)]);
    if (((4 * k) % n == 0 && re + im != 1.f) || ((8 * k) % n == 0 && (4 * k) % n != 0 && (re != diag || im != diag)))
      throw InferaError::onnx("internal: the Spectrum tables of n = " + std::to_string(n) + " are not exact at " + std::to_string(k));
  }
  for (int64_t m = 1; m < h; m++)
    if (p.twiddle[size_t(2 * m)] != p.twiddle[size_t(2 * (h - m))] || p.twiddle[size_t(2 * m + 1)] != -p.twiddle[size_t(2 * (h - m) + 1)] ||
        p.split[size_t(2 * m)] != -p.split[size_t(2 * (h - m))] || p.split[size_t(2 * m + 1)] != p.split[size_t(2 * (h - m) + 1)])
      throw InferaError::onnx("internal: the Spectrum tables of n = " + std::to_string(n) + " are not symmetric at " + std::to_string(m));
  // the launch shape: a wave transforms `per_wave` frames side by side (at least kSpectrumBatchPoints complex points: 8 per lane), a work
  // group `batches` such batches per wave over one staged span
  const int64_t G = mixed ? (kSpectrumBatchPoints + h - 1) / h : std::max(h, kSpectrumBatchPoints) / h, M = G * h;
  const int64_t round = kSpectrumWaves * G, s = std::min(p.hop, n);
  const int64_t rounds_all = p.stft ? (p.frames + round - 1) / round : INT64_MAX;  // (DFT: the call's signals are the frames)
  int64_t k;
  if (p.bins_major) k = std::max<int64_t>(1, mixed ? kSpectrumMaxKeep / M : std::min(4 / G, kSpectrumMaxKeep / M));  // (the wave keeps them all until the tile takes them)
  else k = std::max<int64_t>(1, std::min<int64_t>(((kSpectrumStageFloats - n) / s + 1) / round, 64));
  k = std::min(k, rounds_all);
  if (!mixed) {
    while (k & (k - 1)) k &= k - 1;  // (a power of two: so is Fw)
    p.Fw = int(round * k);
  } else {
    // G need not be a power of two: Fw is the largest one within the k rounds, and the slots behind it stay idle
    int64_t fw = round * k;
    while (fw & (fw - 1)) fw &= fw - 1;
    p.Fw = int(fw);
    k = (fw + round - 1) / round;
    int ns = 1;
    for (int r : spectrum_radices(h)) {
      SpectrumPass ps;
      ps.radix = r, ps.ns = ns, ps.hr = int(h / r), ps.tws = int(h / (int64_t(ns) * r));
      ps.magic_ns = uint32_t((uint64_t(1) << 32) / uint64_t(ns) + 1), ps.magic_hr = uint32_t((uint64_t(1) << 32) / uint64_t(ps.hr) + 1);  // (unused where the divisor is 1)
      p.passes.push_back(ps);
      ns *= r;
    }
  }
  p.per_wave = int(G), p.batches = int(k);
  p.span = (int64_t(p.Fw) - 1) * s + n;
  const int64_t Mpad = M + M / 32;
  const int64_t stage = ((std::max(p.span, p.bins_major ? kSpectrumTileFloats : int64_t(0)) + 3) / 4) * 4;
  p.lds_bytes = 4 * stage + 8 * kSpectrumWaves * (p.bins_major ? k : 1) * Mpad;
  if (!mixed) {
    p.form = spectrum_schedule(log2_of(h)) + "/" + std::to_string(G);
  } else {
    for (const SpectrumPass &ps : p.passes) p.form += (p.form.empty() ? "" : ".") + std::to_string(ps.radix);
    p.form += "/" + std::to_string(G);
  }
}

}  // namespace infera_hip
