// conv3d.hpp -- the geometry of a Conv3d / Pool3d step and how the conv3d kernels split it (hip/conv3d.hip).  Pure
// functions of the geometry: the lowering decides the kernel with them at load, plan.cpp reports the decision, steps.cpp packs and launches by it.
#pragma once

#include <cstdint>

namespace infera_hip {

struct Conv3dGeom {
  int C = 0, D = 0, H = 0, W = 0, M = 0, OD = 0, OH = 0, OW = 0;
  int kd = 1, kh = 1, kw = 1, sd = 1, sh = 1, sw = 1, pf = 0, pt = 0, pl = 0, dd = 1, dh = 1, dw = 1, groups = 1;
};

constexpr int kConv3dMaxKernel = 64;         // largest kernel extent on any axis
constexpr int kConv3dTilePos = 64;           // consecutive output positions of one work group: two 32-column MFMA tiles
constexpr int kConv3dLdsBudget = 64 * 1024;  // bytes of LDS one work group may stage its input window in (what a kernel gets without opting in)

// Step::out_mode of a Conv3d step
enum Conv3dExec : int { kConv3dGeneric = 0, kConv3dMfmaStaged = 1, kConv3dMfmaDirect = 2 };

// conv3d_mfma's split of a layer.  k runs over (channel chunk, kz, ky, kx, channel inside the chunk): CC channels per chunk, Kp = chunks *
// taps * CC rows of packed weights (zero beyond C), Mp = M rounded up to whole 32-channel tiles.  The staged window of one chunk is, per
// channel, one padded input line of Wpad floats for each (output row, kz, ky) of the up to nR output rows (n, od, oh) that kConv3dTilePos
// consecutive positions touch: E floats, CC * E * 4 bytes in all.
struct Conv3dSplit {
  int CC = 0, chunks = 0, taps = 0, Mp = 0, nR = 0, Wpad = 0;
  int64_t Kp = 0, E = 0, lds_bytes = 0;
  bool fits = false;  // lds_bytes <= kConv3dLdsBudget
};
inline Conv3dSplit conv3d_split(const Conv3dGeom &g) {
  Conv3dSplit s;
  s.CC = g.C > 4 ? 8 : g.C > 2 ? 4 : 2;
  s.chunks = (g.C + s.CC - 1) / s.CC;
  s.taps = g.kd * g.kh * g.kw;
  s.Kp = int64_t(s.chunks) * s.taps * s.CC;
  s.Mp = (g.M + 31) / 32 * 32;
  s.nR = (kConv3dTilePos - 1 + g.OW - 1) / g.OW + 1;
  s.Wpad = (g.OW - 1) * g.sw + (g.kw - 1) * g.dw + 1;
  s.E = int64_t(s.nR) * g.kd * g.kh * s.Wpad;
  s.lds_bytes = s.E * s.CC * 4;
  s.fits = s.lds_bytes <= kConv3dLdsBudget;
  return s;
}
// the kernel that serves the layer: the MFMA form takes groups == 1 (stage: INFERA_CONV3D_STAGE=1, the window through LDS where it fits; the
// default reads every tap from global memory, which measured faster: DESIGN.md 3.25), the generic one the rest
inline int conv3d_exec(const Conv3dGeom &g, bool stage) {
  if (g.groups != 1) return kConv3dGeneric;
  return stage && conv3d_split(g).fits ? kConv3dMfmaStaged : kConv3dMfmaDirect;
}

}  // namespace infera_hip
