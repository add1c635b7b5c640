// deformconv_index.cpp -- the coordinate function of the DeformConv kernels (host/deformconv.hpp) on the CPU, under AddressSanitizer and
// UndefinedBehaviorSanitizer (`make -f deformconv_index.mk`): at a few extents and base positions, over the edge values of an offset -- exactly
// -1, exactly H, H - 1 + 2^-20, +-inf, +-1e30, NaN, -0, denormals, a sweep through [-4, 4] and a sweep of bit patterns -- every corner is either
// flagged absent or has an offset inside the plane, and the corners are read from a plane of exactly H * W floats, so a wrong offset is a
// sanitizer report.  A host program with its own main: it is never loaded into Python and needs no GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../infera_amd/csrc/host/deformconv.hpp"

using namespace infera_hip;

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> values = {-1.f, -0.f, 0.f, inf, -inf, 1e30f, -1e30f, nan, std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max(),
                               -std::numeric_limits<float>::max(), 2147483648.f, -2147483648.f, 16777216.f, std::nextafterf(-1.f, -2.f), std::nextafterf(-2.f, -3.f)};
  for (int i = -400; i <= 400; i++) values.push_back(float(i) / 100.f);
  for (uint32_t hi = 0; hi < 512; hi++)  // every sign and exponent, three mantissas each
    for (uint32_t lo : {0u, 1u, 0x7FFFFFu}) {
      const uint32_t bits = (hi << 23) | lo;
      float v;
      std::memcpy(&v, &bits, 4);
      values.push_back(v);
    }
  const int extents[][2] = {{1, 1}, {1, 9}, {5, 7}, {2, 1}, {64, 3}, {1 << 20, 1}, {1, 1 << 20}, {40000, 50000}};
  long checked = 0, failures = 0;
  for (const auto &hw : extents) {
    const int H = hw[0], W = hw[1];
    const bool small = int64_t(H) * W <= (1 << 20);
    std::vector<float> plane(small ? size_t(H) * W : 0, 1.f);  // (the large extents are checked by range alone)
    std::vector<float> vy = values, vx = values;
    for (int size : {H, W}) {  // the values at this extent's own edges, as offsets from base 0
      std::vector<float> &v = size == H ? vy : vx;
      v.push_back(float(size)), v.push_back(float(size - 1) + 0x1p-20f), v.push_back(std::nextafterf(float(size), 0.f)), v.push_back(float(size + 1));
    }
    for (int by : {0, -3, H - 1, H + 2, -(3 << 20), 3 << 20})
      for (int bx : {0, -3, W - 1, W + 2, -(3 << 20), 3 << 20})
        for (size_t iy = 0; iy < vy.size(); iy++)
          for (size_t ix = iy % 7; ix < vx.size(); ix += 7) {  // (every value on each axis, a seventh of the pairs)
            const float oy = vy[iy], ox = vx[ix];
            const DeformTap t = deform_tap(by, bx, oy, ox, H, W);
            const float sy = float(by) + oy, sx = float(bx) + ox;
            const bool in_nan = std::isnan(sy) || std::isnan(sx);
            if (in_nan != t.nan) failures++, std::printf("NaN flag %d for coordinates (%g, %g)\n", int(t.nan), sy, sx);
            float acc = 0.f;
            for (int k = 0; k < 4; k++) {
              const bool inside = (t.inside >> k) & 1u;
              if (t.off[k] < 0 || int64_t(t.off[k]) >= int64_t(H) * W || (!inside && t.off[k] != 0) || std::isnan(t.w[k]) || t.w[k] < 0.f || t.w[k] > 1.f) {
                failures++;
                std::printf("H %d W %d base (%d, %d) offset (%g, %g): corner %d offset %d inside %d weight %g\n", H, W, by, bx, oy, ox, k, t.off[k], int(inside), t.w[k]);
              }
              if (inside && small) acc += plane[size_t(t.off[k])] * t.w[k];
            }
            // strictly inside the plane the four weights sum to one; at or beyond -1 or the extent nothing is read
            if (!in_nan && small && sy >= 0.f && sy <= float(H - 1) && sx >= 0.f && sx <= float(W - 1) && std::fabs(acc - 1.f) > 1e-5f)
              failures++, std::printf("weights sum to %g at (%g, %g) in %d x %d\n", acc, sy, sx, H, W);
            // (exactly at -1 a corner of the plane is present, with weight 0)
            float carried = 0.f;
            for (int k = 0; k < 4; k++) carried += ((t.inside >> k) & 1u) ? t.w[k] : 0.f;
            if (!in_nan && (sy <= -1.f || sy >= float(H) || sx <= -1.f || sx >= float(W)) && carried != 0.f)
              failures++, std::printf("a pixel carries weight %g at (%g, %g) outside %d x %d\n", carried, sy, sx, H, W);
            checked++;
          }
  }
  std::printf("deformconv_index: %ld coordinate pairs checked, %ld failures\n", checked, failures);
  return failures ? 1 : 0;
}
