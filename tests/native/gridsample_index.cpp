// gridsample_index.cpp -- the coordinate function of the GridSample kernel (host/gridsample.hpp) on the CPU, under AddressSanitizer and
// UndefinedBehaviorSanitizer (`make -f gridsample_index.mk`): for every mode, padding and align_corners, at a few extents, over the edge values of a
// grid -- +-1 exactly, just beyond, +-inf, +-1e30, NaN, -0, denormals, a sweep through [-3, 3] -- every tap is either flagged absent or has an
// offset inside the plane, and the taps are read from a plane of exactly H * W floats, so a wrong offset is a sanitizer report.
// A host program with its own main: it is never loaded into Python and needs no GPU.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../infera_amd/csrc/host/gridsample.hpp"

using namespace infera_hip;

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> values = {-1.f, 1.f, -0.f, 0.f, inf, -inf, 1e30f, -1e30f, nan, std::nextafterf(1.f, 2.f), std::nextafterf(-1.f, -2.f),
                               std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max(), -std::numeric_limits<float>::max(), 3.4e38f, 2147483648.f,
                               -2147483648.f, 16777216.f};
  for (int i = -300; i <= 300; i++) values.push_back(float(i) / 100.f);
  const int extents[][2] = {{1, 1}, {1, 9}, {5, 7}, {2, 1}, {64, 3}, {1 << 24, 1}, {1, 1 << 24}, {40000, 50000}};
  long checked = 0, failures = 0;
  for (const auto &hw : extents) {
    const int H = hw[0], W = hw[1];
    const bool small = int64_t(H) * W <= (1 << 20);
    std::vector<float> plane(small ? size_t(H) * W : 0, 1.f);  // (the large extents are checked by range alone)
    for (int mode : {kGridBilinear, kGridNearest})
      for (int pad : {kGridZeros, kGridBorder, kGridReflection})
        for (int align = 0; align < 2; align++)
          for (float gx : values)
            for (float gy : values) {
              const GridTaps t = gridsample_taps(gx, gy, H, W, mode, pad, align != 0);
              const bool in_nan = std::isnan(gx) || std::isnan(gy);
              if (in_nan && !t.nan) failures++, std::printf("NaN in, no NaN flag: %g %g\n", gx, gy);
              float acc = 0.f;
              for (int k = 0; k < (mode == kGridNearest ? 1 : 4); k++) {
                const bool inside = (t.inside >> k) & 1u;
                if (t.off[k] < 0 || int64_t(t.off[k]) >= int64_t(H) * W || (!inside && t.off[k] != 0) || std::isnan(t.w[k])) {
                  failures++;
                  std::printf("H %d W %d mode %d pad %d align %d g (%g, %g): tap %d offset %d inside %d weight %g\n", H, W, mode, pad, align, gx, gy, k, t.off[k], int(inside), t.w[k]);
                }
                if (inside && small) acc += plane[size_t(t.off[k])] * t.w[k];
              }
              if (!in_nan && !t.nan && pad == kGridBorder && mode == kGridBilinear && small && std::fabs(acc - 1.f) > 1e-5f)  // border never reads nothing
                failures++, std::printf("border weights do not sum to one: %g at (%g, %g) in %d x %d\n", acc, gx, gy, H, W);
              checked++;
            }
  }
  // the affine form: the coordinates of every corner position under edge thetas go through the same function
  const float thetas[][6] = {{1, 0, 0, 0, 1, 0}, {inf, 0, 0, 0, -inf, 0}, {nan, 1, 1, 1, 1, 1}, {1e30f, -1e30f, 1e30f, 3.f, -2.f, 0.5f}, {0, 0, 0, 0, 0, 0}};
  for (const auto &th : thetas)
    for (int align = 0; align < 2; align++)
      for (int oh : {0, 5})
        for (int ow : {0, 10}) {
          float gx, gy;
          affinegrid_point(th, oh, ow, 6, 11, align != 0, &gx, &gy);
          const GridTaps t = gridsample_taps(gx, gy, 5, 7, kGridBilinear, kGridReflection, align != 0);
          for (int k = 0; k < 4; k++)
            if (t.off[k] < 0 || t.off[k] >= 35) failures++;
          checked++;
        }
  std::printf("gridsample_index: %ld coordinate pairs checked, %ld failures\n", checked, failures);
  return failures ? 1 : 0;
}
