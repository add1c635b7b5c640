// mlp_device.inc -- DEVICE code of the whole-chain fused MLP (see mlp_fused.hip for the design notes).
//
// Self-contained on purpose (needs only <hip/hip_runtime.h>): the same text is compiled ahead of time
// into libinfera.so for the benchmark shapes (mlp_fused.hip) and handed to hipRTC at infera_load_model
// time for any other chain shape that fits (mlp_jit.cpp), which is what "the graph is lowered to fused
// kernels at load time" means for MLPs the build never saw.
namespace infera_hip {
namespace kern {
namespace mlpdev {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using i64 = long long;  // (no <cstdint> under hipRTC)

// Parameter-free activations a fused chain may carry between layers (codes = plan.hpp Act).
template <int KIND>
__device__ __forceinline__ float act_c(float v) {
  if constexpr (KIND == 1) return v > 0.f ? v : 0.f;
  if constexpr (KIND == 2) return 1.0f / (1.0f + expf(-v));
  if constexpr (KIND == 3) return tanhf(v);
  return v;
}

constexpr int kLdsBytes = 160 * 1024;

// P1/P2: fragment prefetch depth (units) for layer 1 / layer 2.  NL2: layer-2 fragment groups kept
// in LDS (-1 = as many as fit).  L3V: evaluate the last layer on the VALU (requires D3 <= 4).
// NR2: layer-2 fragment units pinned in REGISTERS for the lifetime of the wave (-1 = all that do not fit
// in LDS): at one wave per SIMD the kernel owns 512 registers per lane and the tile body needs ~360.
template <int D0_, int D1_, int D2_, int D3_, int A1_, int A2_, int A3_, int WAVES_, int P1_ = 3, int P2_ = 16, int NL2_ = -1,
          int NR2_ = 0, bool L3V_ = (D3_ <= 4)>
struct Cfg {
  static constexpr int D0 = D0_, D1 = D1_, D2 = D2_, D3 = D3_;
  static constexpr int A1 = A1_, A2 = A2_, A3 = A3_, WAVES = WAVES_, P1 = P1_, P2 = P2_;
  static constexpr bool L3V = L3V_;
  static_assert(D0 % 8 == 0 && D1 % 32 == 0 && D2 % 32 == 0 && D3 >= 1 && D3 <= 32, "unsupported chain shape");
  static_assert(!L3V || D3 <= 4, "VALU last layer is for narrow heads only");
  static constexpr int G0 = D0 / 8, G1 = D1 / 8, G2 = D2 / 8;  // groups of 4 k-steps per layer input
  static constexpr int MT1 = D1 / 32, MT2 = D2 / 32, MT3 = 1;  // 32-wide output tiles per layer
  static constexpr int GRP2 = MT2 * 256;                       // floats per layer-2 fragment group
  // ---- packed blob (global memory), floats ----
  static constexpr int OFF_W1 = 0, N_W1 = G0 * MT1 * 256;
  static constexpr int OFF_W2 = OFF_W1 + N_W1, N_W2 = G1 * GRP2;
  static constexpr int OFF_SMALL = OFF_W2 + N_W2;
  //   small block: bias quads [mt][rg][h][4] for layers 1,2; then layer 3 (fragments, or VALU weight
  //   quads [kt][rg][h][m][4]); then layer-3 bias (quads, or D3 plain floats padded to 4)
  static constexpr int S_B1 = 0, N_B1 = MT1 * 32;
  static constexpr int S_B2 = S_B1 + N_B1, N_B2 = MT2 * 32;
  static constexpr int S_W3 = S_B2 + N_B2, N_W3 = L3V ? MT2 * 32 * D3 : G2 * MT3 * 256;
  static constexpr int S_B3 = S_W3 + N_W3, N_B3 = L3V ? 4 : MT3 * 32;
  static constexpr int N_SMALL = S_B3 + N_B3;
  static constexpr int N_TOTAL = OFF_SMALL + N_SMALL;
  // ---- LDS image: [W1][first NL2 groups of W2][small] ----
  static constexpr int FIT2 = (kLdsBytes / 4 - N_W1 - N_SMALL) / GRP2;
  static_assert(FIT2 >= 0, "layer-1 fragments + small block exceed 160 KiB of LDS");
  static constexpr int NL2 = NL2_ < 0 ? (FIT2 > G1 ? G1 : FIT2) : NL2_;
  static_assert(NL2 <= FIT2 && NL2 <= G1, "requested LDS share of layer 2 does not fit");
  static constexpr int NR2 = NR2_ < 0 ? (G1 - NL2) * MT2 : NR2_;  // units held in registers
  static_assert(NR2 <= (G1 - NL2) * MT2, "more register-resident units than layer 2 has outside LDS");
  static constexpr int L_W1 = 0, L_W2 = N_W1, L_SMALL = N_W1 + NL2 * GRP2;
  static constexpr int N_LDS = L_SMALL + N_SMALL;
  static_assert(N_LDS * 4 <= kLdsBytes && (L_SMALL % 4) == 0, "LDS image exceeds 160 KiB");
};

// XCM: X is a column-major chunk [D0][rows] (DuckDB's flat columns copied as they lie, SURVEY.md 7 "hard parts") --
// each of a lane's four k-values is then one dword of a 128-byte run shared with its 31 row neighbours.
template <class C, bool XCM = false>
__global__ __launch_bounds__(C::WAVES * 64) void mlp3_kernel(const float *__restrict__ X, const float *__restrict__ packed,
                                                            float *__restrict__ Y, i64 rows) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;

  // ---- stage the LDS image once per workgroup (coalesced 16 B loads) ----
  {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(packed);
    f32x4 *dst = reinterpret_cast<f32x4 *>(lds);
    for (int i = threadIdx.x; i < C::L_SMALL / 4; i += C::WAVES * 64) dst[i] = src[i];  // W1 + first NL2 groups of W2
    const f32x4 *ssrc = reinterpret_cast<const f32x4 *>(packed + C::OFF_SMALL);
    f32x4 *sdst = reinterpret_cast<f32x4 *>(lds + C::L_SMALL);
    for (int i = threadIdx.x; i < C::N_SMALL / 4; i += C::WAVES * 64) sdst[i] = ssrc[i];
  }
  __syncthreads();

  const f32x4 *w1 = reinterpret_cast<const f32x4 *>(lds + C::L_W1) + lane;
  const f32x4 *w2l = reinterpret_cast<const f32x4 *>(lds + C::L_W2) + lane;
  const float *small = lds + C::L_SMALL;
  const f32x4 *b1 = reinterpret_cast<const f32x4 *>(small + C::S_B1) + h;
  const f32x4 *b2 = reinterpret_cast<const f32x4 *>(small + C::S_B2) + h;
  const f32x4 *w3 = reinterpret_cast<const f32x4 *>(small + C::S_W3) + (C::L3V ? h * C::D3 : lane);
  const float *b3 = small + C::S_B3;
  const f32x4 *w2g_base = reinterpret_cast<const f32x4 *>(packed + C::OFF_W2) + lane;

  const i64 ntiles = (rows + 31) >> 5;
  const i64 tstride = i64(gridDim.x) * C::WAVES;
  i64 tile = i64(blockIdx.x) * C::WAVES + wave;
  if (tile >= ntiles) return;

  auto load_x = [&](f32x4(&x)[C::G0], i64 t) {
    i64 row = (t << 5) + r;
    if (row >= rows) row = rows - 1;  // tail rows recompute the last row; their stores are masked
    if constexpr (XCM) {
      const float *p = X + i64(4 * h) * rows + row;
#pragma unroll
      for (int g = 0; g < C::G0; g++)
#pragma unroll
        for (int j = 0; j < 4; j++) x[g][j] = p[i64(8 * g + j) * rows];
    } else {
      const f32x4 *p = reinterpret_cast<const f32x4 *>(X + row * C::D0 + 4 * h);
#pragma unroll
      for (int g = 0; g < C::G0; g++) x[g] = p[2 * g];
    }
  };

  constexpr int U1 = C::G0 * C::MT1, P1 = C::P1;  // LDS fragments: ~128-cycle latency, unit = 256 cycles
  constexpr int U2 = C::G1 * C::MT2, P2 = C::P2;  // layer-2 ring depth (L2 fragments need ~1-2k cycles)
  constexpr int U2L = C::NL2 * C::MT2;            // units [0, U2L) come from LDS,
  constexpr int U2R = U2L + C::NR2;               //       [U2L, U2R) from registers, [U2R, U2) from L2
  constexpr int U3 = C::G2, P3 = 2;
  constexpr int NQ = C::MT2 * 4;                  // accumulator quads of layer 2 (VALU head slices)
  static_assert(U1 >= P1 && U2 >= P2 && (C::L3V || U3 >= P3) && (!C::L3V || U1 > NQ), "chain too small for the pipeline depths");

  // ---- narrow head on the VALU: y[m] += sum_j w3[k(q,j)][m] * act2(acc2 quad q + b2 quad q) ----
  float yacc[C::L3V ? C::D3 : 1];
  auto head_slice = [&](const f32x16(&p2)[C::MT2], int q) {
    const int kt = q / 4, rg = q % 4;
    const f32x4 bq = b2[q * 2];
    f32x4 hv;
#pragma unroll
    for (int j = 0; j < 4; j++) hv[j] = act_c<C::A2>(p2[kt][4 * rg + j] + bq[j]);
#pragma unroll
    for (int m = 0; m < (C::L3V ? C::D3 : 0); m++) {
      const f32x4 wq = w3[q * 2 * C::D3 + m];
#pragma unroll
      for (int j = 0; j < 4; j++) yacc[m] = fmaf(wq[j], hv[j], yacc[m]);
    }
  };
  auto head_store = [&](i64 t) {
    const i64 row = (t << 5) + r;
#pragma unroll
    for (int m = 0; m < (C::L3V ? C::D3 : 0); m++) {
      const float tot = yacc[m] + __shfl_xor(yacc[m], 32);  // the two lane halves hold disjoint k
      if (h == 0 && t >= 0 && row < rows) Y[row * C::D3 + m] = act_c<C::A3>(tot + b3[m]);
      yacc[m] = 0.f;
    }
  };

  // layer-2 fragments that fit neither LDS nor the per-tile working set's shadow: loaded ONCE per wave
  // and kept in registers (loop invariant on purpose).
  f32x4 wreg[C::NR2 > 0 ? C::NR2 : 1];
#pragma unroll
  for (int i = 0; i < C::NR2; i++) wreg[i] = w2g_base[(U2L + i) * 64];

  f32x4 x[C::G0];
  load_x(x, tile);
  f32x16 pend[C::MT2];  // layer-2 accumulators of the previous tile, consumed by the VALU head
#pragma unroll
  for (int mt = 0; mt < C::MT2; mt++)
#pragma unroll
    for (int i = 0; i < 16; i++) pend[mt][i] = 0.f;
#pragma unroll
  for (int m = 0; m < (C::L3V ? C::D3 : 1); m++) yacc[m] = 0.f;
  i64 pend_tile = -1;

  for (; tile < ntiles; tile += tstride) {
    const bool has_next = tile + tstride < ntiles;
    // The fragment addresses are loop invariant and hipcc's LICM would hoist all layer-2 loads out of
    // the tile loop (= W2 held in 256 VGPRs, everything else spilled).  Launder an integer offset per
    // tile (not the pointer itself: that drops it to the flat address space, and flat loads also count
    // on lgkmcnt, i.e. every LDS wait would wait for L2).
    int zero = 0;
    asm volatile("" : "+s"(zero));
    const f32x4 *w2g = w2g_base + zero;
    auto frag2 = [&](int u) -> f32x4 { return u < U2L ? w2l[u * 64] : (u < U2R ? wreg[u - U2L] : w2g[u * 64]); };
    constexpr int LAST_G = U2R < U2 ? U2 - P2 - 1 : -1;  // unit that issues the last L2 fragment load (-1: none)

    // ================= layer 1: acc1[mt] = W1^T . X^T   (+ VALU head of the previous tile) =================
    f32x16 acc1[C::MT1];
#pragma unroll
    for (int mt = 0; mt < C::MT1; mt++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc1[mt][i] = 0.f;
    {
      f32x4 ring1[P1];
#pragma unroll
      for (int u = 0; u < P1; u++) ring1[u] = w1[u * 64];
#pragma unroll
      for (int u = 0; u < U1; u++) {
        const int g = u / C::MT1, mt = u % C::MT1;
        const f32x4 a = ring1[u % P1];
        if (u + P1 < U1) ring1[u % P1] = w1[(u + P1) * 64];
        if constexpr (C::L3V) {
          if (u < NQ) head_slice(pend, u);
          if (u == NQ) head_store(pend_tile);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) acc1[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], x[g][j], acc1[mt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    // ================= layer 2: acc2[mt] = W2^T . act1(acc1 + b1) =================
    f32x16 acc2[C::MT2];
#pragma unroll
    for (int mt = 0; mt < C::MT2; mt++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc2[mt][i] = 0.f;
    {
      f32x4 ring2[P2], bring1[2];
#pragma unroll
      for (int u = 0; u < P2; u++) ring2[u] = frag2(u);
      bring1[0] = b1[0];
#pragma unroll
      for (int g = 0; g < C::G1; g++) {
        const int kt = g / 4, rg = g % 4;
        const f32x4 bq = bring1[g % 2];
        if (g + 1 < C::G1) bring1[(g + 1) % 2] = b1[(g + 1) * 2];  // bias quad one group ahead
        float hv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) hv[j] = act_c<C::A1>(acc1[kt][4 * rg + j] + bq[j]);
#pragma unroll
        for (int mt = 0; mt < C::MT2; mt++) {
          const int u = g * C::MT2 + mt;
          const f32x4 a = ring2[u % P2];
          if (u + P2 < U2) ring2[u % P2] = frag2(u + P2);
          // Next tile's X rows (HBM): requested right after the LAST layer-2 L2 load of this tile.
          // vmcnt retires in order, so nothing in this tile waits behind HBM latency, and the request
          // still has the tail of layer 2 (P2 units) to land.  x is dead since the end of layer 1.
          if (u == (LAST_G >= 0 ? LAST_G : 0) && has_next) load_x(x, tile + tstride);
#pragma unroll
          for (int j = 0; j < 4; j++) acc2[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], hv[j], acc2[mt], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }

    if constexpr (C::L3V) {
      // hand the layer-2 accumulators to the next iteration's VALU head
#pragma unroll
      for (int mt = 0; mt < C::MT2; mt++) pend[mt] = acc2[mt];
      pend_tile = tile;
    } else {
      // ================= layer 3 on the matrix cores: acc3 = W3^T . act2(acc2 + b2)  (D3 <= 32) =================
      f32x16 acc3;
#pragma unroll
      for (int i = 0; i < 16; i++) acc3[i] = 0.f;
      f32x4 ring3[P3], bring2[2];
      bring2[0] = b2[0];
#pragma unroll
      for (int u = 0; u < P3; u++) ring3[u] = w3[u * 64];
#pragma unroll
      for (int g = 0; g < U3; g++) {
        const int kt = g / 4, rg = g % 4;
        const f32x4 bq = bring2[g % 2];
        if (g + 1 < U3) bring2[(g + 1) % 2] = b2[(g + 1) * 2];
        const f32x4 a = ring3[g % P3];
        if (g + P3 < U3) ring3[g % P3] = w3[(g + P3) * 64];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float hv = act_c<C::A2>(acc2[kt][4 * rg + j] + bq[j]);
          acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], hv, acc3, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // epilogue: Y[row, f] = act3(acc3 + b3), f = 8*rg + 4h + j < D3
      const i64 row = (tile << 5) + r;
      if (row < rows) {
        float *yrow = Y + row * C::D3;
        const f32x4 *b3q = reinterpret_cast<const f32x4 *>(b3) + h;
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const f32x4 bq = b3q[rg * 2];
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int f = 8 * rg + 4 * h + j;  // h is runtime: both halves test f < D3
            if (8 * rg + j < C::D3 && f < C::D3) yrow[f] = act_c<C::A3>(acc3[4 * rg + j] + bq[j]);
          }
        }
      }
    }
  }

  if constexpr (C::L3V) {  // drain: head of the last tile
#pragma unroll
    for (int q = 0; q < NQ; q++) head_slice(pend, q);
    head_store(pend_tile);
  }
}

// ---- two-waves-per-SIMD variant ------------------------------------------------------------------------
// Same math and packed blob as mlp3_kernel, but 8 waves per workgroup (two per SIMD, <= 256 registers
// each) so that one wave's VALU-only phases, s_waitcnt stalls and epilogue are covered by the sibling
// wave's MFMAs.  To fit 256 registers layer 1 is evaluated in SPLIT feature halves; each half is fed to
// layer 2 (a partial sum over that half's k range) before the next half is computed, so only
// MT1/SPLIT accumulator tiles are live at a time.  X stays in registers across the halves.  The narrow
// head runs on the VALU at the end of the tile (no cross-tile software pipelining needed here).
//
// TQ (tile queue): the waves of a launch do not run at equal speed (the two waves of a SIMD are arbitrated by age, and there
// is no barrier in the loop to re-align them), so a fixed share of the tiles leaves the faster ones gone while the slower
// ones still work alone on their SIMD.  With TQ a wave's FIRST tile is still blockIdx.x * NW + wave (no atomic before the
// first MFMA); every later one is W + atomicAdd(queue[0], 1), W = gridDim.x * NW, claimed by one lane at the top of the tile
// before -- it is the oldest entry of the in-order vmcnt counter by the time its value is needed, at the unit that requests
// the next tile's rows, a whole tile later, so it is never waited on.  Which wave computes a tile does not enter the
// arithmetic: same bits as the static form.
// queue[0] = head, queue[1] = done: both zero between launches.  A wave adds 1 to `done` when it leaves (also one that got
// no first tile); the wave that completes the count W has seen every claim of the launch return, and zeroes both words: no
// memset, no extra launch.  The two words belong to ONE stream's launches (they are not shared between concurrent kernels).
// TQ = false is the static form (tile += W), kept for within-process A/B runs.
template <class C, int SPLIT, int P2S, int NW, bool XCM = false, bool TQ = true>
__global__ __launch_bounds__(NW * 64) void mlp3_split_kernel(const float *__restrict__ X, const float *__restrict__ packed,
                                                        float *__restrict__ Y, i64 rows, unsigned *queue
#ifdef INFERA_MLP3_PROBES
                                                        , unsigned long long *probe  // [gridDim.x * NW][4], or null (tools/mlp_wave_residency.py)
#endif
) {
  static_assert(C::L3V && C::MT1 % SPLIT == 0 && C::G1 % SPLIT == 0, "split kernel: VALU head, even split");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(packed);
    f32x4 *dst = reinterpret_cast<f32x4 *>(lds);
    for (int i = threadIdx.x; i < C::L_SMALL / 4; i += NW * 64) dst[i] = src[i];
    const f32x4 *ssrc = reinterpret_cast<const f32x4 *>(packed + C::OFF_SMALL);
    f32x4 *sdst = reinterpret_cast<f32x4 *>(lds + C::L_SMALL);
    for (int i = threadIdx.x; i < C::N_SMALL / 4; i += NW * 64) sdst[i] = ssrc[i];
  }
  __syncthreads();
#ifdef INFERA_MLP3_PROBES
  // (the entry stamp is stored at once: held to the exit it would cost the tile loop two scalar registers)
  if (probe && lane == 0) probe[(i64(blockIdx.x) * NW + wave) * 4 + 1] = __builtin_amdgcn_s_memrealtime();  // 100 MHz
  unsigned probe_tiles = 0;
#endif
  const f32x4 *w1 = reinterpret_cast<const f32x4 *>(lds + C::L_W1) + lane;
  const f32x4 *w2l = reinterpret_cast<const f32x4 *>(lds + C::L_W2) + lane;
  const float *small = lds + C::L_SMALL;
  const f32x4 *b1 = reinterpret_cast<const f32x4 *>(small + C::S_B1) + h;
  const f32x4 *b2 = reinterpret_cast<const f32x4 *>(small + C::S_B2) + h;
  const f32x4 *w3 = reinterpret_cast<const f32x4 *>(small + C::S_W3) + h * C::D3;
  const float *b3 = small + C::S_B3;
  const f32x4 *w2g_base = reinterpret_cast<const f32x4 *>(packed + C::OFF_W2) + lane;

  const i64 ntiles = (rows + 31) >> 5;
  const i64 tstride = i64(gridDim.x) * NW;
  i64 tile = i64(blockIdx.x) * NW + wave;

  auto load_x = [&](f32x4(&x)[C::G0], i64 t) {
    i64 row = (t << 5) + r;
    if (row >= rows) row = rows - 1;
    if constexpr (XCM) {
      const float *p = X + i64(4 * h) * rows + row;
#pragma unroll
      for (int g = 0; g < C::G0; g++)
#pragma unroll
        for (int j = 0; j < 4; j++) x[g][j] = p[i64(8 * g + j) * rows];
    } else if constexpr (TQ) {
      // the same rows from a wave-uniform tile base plus a 32-bit lane offset (tail rows clamped as above): the lane-wide 64-bit
      // address of the static form costs the three-output kernel two spilled registers once the claim holds one
      const i64 lim = rows - 1 - (t << 5);
      const int rl = lim < 31 ? int(lim) : 31;
      const unsigned off = unsigned((r < rl ? r : rl) * C::D0 + 4 * h);
      const f32x4 *p = reinterpret_cast<const f32x4 *>(X + (t << 5) * C::D0 + off);
#pragma unroll
      for (int g = 0; g < C::G0; g++) x[g] = p[2 * g];
    } else {
      const f32x4 *p = reinterpret_cast<const f32x4 *>(X + row * C::D0 + 4 * h);
#pragma unroll
      for (int g = 0; g < C::G0; g++) x[g] = p[2 * g];
    }
  };

  constexpr int MTH = C::MT1 / SPLIT, G1H = C::G1 / SPLIT;
  constexpr int U1H = C::G0 * MTH, P1 = C::P1;
  constexpr int U2 = C::G1 * C::MT2, U2H = G1H * C::MT2, P2 = P2S;
  constexpr int U2L = C::NL2 * C::MT2;
  constexpr int NQ = C::MT2 * 4;
  // unit after which next tile's X may be requested: x must be dead (last split) and, if possible, the
  // last L2 fragment load of the tile already issued
  constexpr int LAST_G = U2L < U2 ? U2 - P2 - 1 : -1;
  constexpr int XPF = LAST_G > U2 - U2H ? LAST_G : U2 - U2H;
  static_assert(U1H >= P1 && U2H >= P2, "chain too small for the pipeline depths");

  f32x4 x[C::G0];
  if (tile < ntiles) load_x(x, tile);
  while (tile < ntiles) {
    i64 next = tile + tstride;
    // the claim for the NEXT tile: one lane, issued before this tile's ring loads, read at u == XPF
    unsigned claim = 0;
    if constexpr (TQ) {
      // (the offset in a vector register: with a wave-uniform address hipcc rewrites the atomic as a wave reduction and waits
      // for its result on the spot)
      unsigned lane_off = 0;
      asm volatile("" : "+v"(lane_off));
      if (lane == 0) claim = __hip_atomic_fetch_add(queue + lane_off, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    int zero = 0;
    asm volatile("" : "+s"(zero));
    const f32x4 *w2g = w2g_base + zero;
    auto frag2 = [&](int u) -> f32x4 { return u < U2L ? w2l[u * 64] : w2g[u * 64]; };

    f32x16 acc2[C::MT2];
#pragma unroll
    for (int mt = 0; mt < C::MT2; mt++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc2[mt][i] = 0.f;
    f32x4 ring2[P2];
#pragma unroll
    for (int u = 0; u < P2; u++) ring2[u] = frag2(u);

#pragma unroll
    for (int s = 0; s < SPLIT; s++) {
      // ---- layer 1, feature tiles [s*MTH, (s+1)*MTH) ----
      f32x16 acc1[MTH];
#pragma unroll
      for (int mt = 0; mt < MTH; mt++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc1[mt][i] = 0.f;
      {
        f32x4 ring1[P1];
#pragma unroll
        for (int u = 0; u < P1; u++) ring1[u] = w1[((u / MTH) * C::MT1 + s * MTH + (u % MTH)) * 64];
#pragma unroll
        for (int u = 0; u < U1H; u++) {
          const int g = u / MTH, mt = u % MTH;
          const f32x4 a = ring1[u % P1];
          if (u + P1 < U1H) ring1[u % P1] = w1[(((u + P1) / MTH) * C::MT1 + s * MTH + ((u + P1) % MTH)) * 64];
#pragma unroll
          for (int j = 0; j < 4; j++) acc1[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], x[g][j], acc1[mt], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // ---- layer 2, k groups [s*G1H, (s+1)*G1H): partial sums into acc2 ----
      f32x4 bring1[2];
      bring1[0] = b1[(s * G1H) * 2];
#pragma unroll
      for (int gl = 0; gl < G1H; gl++) {
        const int g = s * G1H + gl, ktl = gl / 4, rg = gl % 4;
        const f32x4 bq = bring1[gl % 2];
        if (gl + 1 < G1H) bring1[(gl + 1) % 2] = b1[(g + 1) * 2];
        float hv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) hv[j] = act_c<C::A1>(acc1[ktl][4 * rg + j] + bq[j]);
#pragma unroll
        for (int mt = 0; mt < C::MT2; mt++) {
          const int u = g * C::MT2 + mt;
          const f32x4 a = ring2[u % P2];
          if (u + P2 < U2) ring2[u % P2] = frag2(u + P2);
          if (u == XPF) {  // x is dead in the last split
            if constexpr (TQ) next = tstride + i64(unsigned(__builtin_amdgcn_readfirstlane(int(claim))));
            if (next < ntiles) load_x(x, next);
          }
#pragma unroll
          for (int j = 0; j < 4; j++) acc2[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], hv[j], acc2[mt], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    // ---- narrow head on the VALU ----
    float yacc[C::D3];
#pragma unroll
    for (int m = 0; m < C::D3; m++) yacc[m] = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int kt = q / 4, rg = q % 4;
      const f32x4 bq = b2[q * 2];
#pragma unroll
      for (int m = 0; m < C::D3; m++) {
        const f32x4 wq = w3[q * 2 * C::D3 + m];
#pragma unroll
        for (int j = 0; j < 4; j++) yacc[m] = fmaf(wq[j], act_c<C::A2>(acc2[kt][4 * rg + j] + bq[j]), yacc[m]);
      }
    }
    const i64 row = (tile << 5) + r;
#pragma unroll
    for (int m = 0; m < C::D3; m++) {
      const float tot = yacc[m] + __shfl_xor(yacc[m], 32);
      if (h == 0 && row < rows) Y[row * C::D3 + m] = act_c<C::A3>(tot + b3[m]);
    }
#ifdef INFERA_MLP3_PROBES
    probe_tiles++;
#endif
    tile = next;
  }
  // ---- leave: count this wave out; the last one of the launch hands the queue back as it found it ----
  // (lane 0 found anew: keeping `lane` alive across the loop for this costs the row-major kernel its 257th register)
  const bool first_lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u;
  if constexpr (TQ) {
    if (first_lane) {
      const unsigned nwaves = gridDim.x * NW;
      if (__hip_atomic_fetch_add(queue + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nwaves - 1) {
        __hip_atomic_store(queue, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(queue + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
#ifdef INFERA_MLP3_PROBES
  if (probe && first_lane) {  // one lane per wave, once per launch, plain vector stores
    const unsigned long long hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_REG_HW_ID: simd 5:4, cu 11:8, sh 12, se 15:13
    const unsigned long long xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);  // HW_REG_XCC_ID 3:0
    unsigned long long *p = probe + (i64(blockIdx.x) * NW + wave) * 4;
    p[0] = (unsigned long long)blockIdx.x | ((unsigned long long)wave << 20) | (xcc << 24) | ((hw & 0xffffull) << 32);
    p[2] = __builtin_amdgcn_s_memrealtime();
    p[3] = probe_tiles;
  }
#endif
}

// ---- latency-shaped variant for SHORT launches (one DataChunk through the host ABI) --------------------------------------
// A 2048-row chunk is 64 tiles: the persistent kernels give each tile to one wave (768 MFMAs = 20 us) behind a 160 KB LDS image
// per workgroup -- 50 us for 1.3 us worth of matrix work, most of the chip idle.  Here a WORKGROUP owns one 32-row tile and its
// four waves share the work of mlp3_split_kernel<C, 4, ...> in a way that keeps EVERY sum in that kernel's order, so the
// results are bit-identical (a chunk through the host ABI equals its slice of a device-resident scan, tests/test_parity_gpu.py):
//   * layer 1: wave w computes the feature tiles of the split kernel's slice w (MT1/4 tiles, same k order), weight fragments
//     straight from the packed blob in L2 (each is used once per workgroup: staging them in LDS would buy nothing);
//   * bias + activation, then the tile's activations go to LDS as [row][feature];
//   * layer 2: wave t < MT2 accumulates output tile t over all D1 inputs in the split kernel's (group, j) order, B operands
//     from that LDS image;
//   * the VALU head is a chain over the layer-2 tiles: wave 0 runs its part and hands its partial sums to wave 1 through LDS,
//     which continues the same fmaf chain and stores.
// XCM as above.  MT2 <= 4, VALU head; layer 1 in four slices (two / one when MT1 is no multiple of 4 / 2).
template <class C, bool XCM = false>
__global__ __launch_bounds__(256) void mlp3_tile_kernel(const float *__restrict__ X, const float *__restrict__ packed,
                                                        float *__restrict__ Y, i64 rows) {
  static_assert(C::L3V && C::MT2 <= 4, "tile kernel: VALU head, at most four layer-2 tiles");
  constexpr int NS1 = C::MT1 % 4 == 0 ? 4 : (C::MT1 % 2 == 0 ? 2 : 1);  // layer-1 slices = waves that take part in layer 1
  constexpr int MTH = C::MT1 / NS1;        // layer-1 tiles per such wave
  constexpr int U1 = C::G0 * MTH;          // layer-1 units of this wave
  constexpr int U2 = C::G1;                // layer-2 units of a wave (one output tile)
  constexpr int P = 16;                    // fragment ring depth: L2 latency (~2 us) against 0.1 us units
  constexpr int ROWF = C::D1 + 4;          // floats per activation row in LDS (16-byte aligned, rows 4 banks apart)
  __shared__ __attribute__((aligned(16))) float act[32 * ROWF];
  __shared__ float ypart[C::MT2 > 1 ? (C::MT2 - 1) * 64 * C::D3 : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const i64 tile = blockIdx.x;
  const f32x4 *w1 = reinterpret_cast<const f32x4 *>(packed + C::OFF_W1) + lane;
  const f32x4 *w2 = reinterpret_cast<const f32x4 *>(packed + C::OFF_W2) + lane;
  const float *small = packed + C::OFF_SMALL;
  const f32x4 *b1 = reinterpret_cast<const f32x4 *>(small + C::S_B1) + h;
  const f32x4 *b2 = reinterpret_cast<const f32x4 *>(small + C::S_B2) + h;
  const f32x4 *w3 = reinterpret_cast<const f32x4 *>(small + C::S_W3) + h * C::D3;
  const float *b3 = small + C::S_B3;

  // ---- layer 1: slice `wave` (hidden layers narrower than 128: fewer slices, the other waves wait at the barrier) ----
  const bool l1wave = wave < NS1;
  auto frag1 = [&](int u) { return w1[((u / MTH) * C::MT1 + (l1wave ? wave : 0) * MTH + (u % MTH)) * 64]; };
  f32x4 ring[P];
#pragma unroll
  for (int u = 0; u < P && u < U1; u++) ring[u] = frag1(u);
  f32x4 x[C::G0];
  {
    i64 row = (tile << 5) + r;
    if (row >= rows) row = rows - 1;
    if constexpr (XCM) {
      const float *p = X + i64(4 * h) * rows + row;
#pragma unroll
      for (int g = 0; g < C::G0; g++)
#pragma unroll
        for (int j = 0; j < 4; j++) x[g][j] = p[i64(8 * g + j) * rows];
    } else {
      const f32x4 *p = reinterpret_cast<const f32x4 *>(X + row * C::D0 + 4 * h);
#pragma unroll
      for (int g = 0; g < C::G0; g++) x[g] = p[2 * g];
    }
  }
  f32x16 acc1[MTH];
#pragma unroll
  for (int mt = 0; mt < MTH; mt++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc1[mt][i] = 0.f;
  if (l1wave) {
#pragma unroll
    for (int u = 0; u < U1; u++) {
      const int g = u / MTH, mt = u % MTH;
      const f32x4 a = ring[u % P];
      if (u + P < U1) ring[u % P] = frag1(u + P);
#pragma unroll
      for (int j = 0; j < 4; j++) acc1[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], x[g][j], acc1[mt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // layer-2 fragments of this wave's output tile: requested before the exchange so they are under way during it
  const bool l2wave = wave < C::MT2;
  auto frag2 = [&](int g) { return w2[(g * C::MT2 + (l2wave ? wave : 0)) * 64]; };
  if (l2wave) {
#pragma unroll
    for (int u = 0; u < P && u < U2; u++) ring[u] = frag2(u);
  }
  // bias + activation (the arithmetic the split kernel applies when it consumes the accumulators), then [row][feature] in LDS
  if (l1wave) {
#pragma unroll
    for (int mt = 0; mt < MTH; mt++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int g = (wave * MTH + mt) * 4 + q;  // layer-2 k group: features 8g + 4h + j
        const f32x4 bq = b1[g * 2];
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = act_c<C::A1>(acc1[mt][4 * q + j] + bq[j]);
        *reinterpret_cast<f32x4 *>(act + r * ROWF + 8 * g + 4 * h) = v;
      }
  }
  __syncthreads();
  // ---- layer 2: wave t owns output tile t ----
  f32x16 acc2;
#pragma unroll
  for (int i = 0; i < 16; i++) acc2[i] = 0.f;
  if (l2wave) {
    const f32x4 *arow = reinterpret_cast<const f32x4 *>(act + r * ROWF + 4 * h);
#pragma unroll
    for (int g = 0; g < U2; g++) {
      const f32x4 a = ring[g % P];
      if (g + P < U2) ring[g % P] = frag2(g + P);
      const f32x4 hv = arow[2 * g];
#pragma unroll
      for (int j = 0; j < 4; j++) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], hv[j], acc2, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // ---- head: the split kernel's fmaf chain over q = 4*tile + rg; tile t's wave continues from tile t-1's partial sums ----
  float yacc[C::D3];
#pragma unroll
  for (int m = 0; m < C::D3; m++) yacc[m] = 0.f;
#pragma unroll
  for (int t = 0; t < C::MT2; t++) {
    if (wave == t) {
      if (t > 0) {
#pragma unroll
        for (int m = 0; m < C::D3; m++) yacc[m] = ypart[((t - 1) * 64 + lane) * C::D3 + m];
      }
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const int q = t * 4 + rg;
        const f32x4 bq = b2[q * 2];
#pragma unroll
        for (int m = 0; m < C::D3; m++) {
          const f32x4 wq = w3[q * 2 * C::D3 + m];
#pragma unroll
          for (int j = 0; j < 4; j++) yacc[m] = fmaf(wq[j], act_c<C::A2>(acc2[4 * rg + j] + bq[j]), yacc[m]);
        }
      }
      if (t + 1 < C::MT2) {
#pragma unroll
        for (int m = 0; m < C::D3; m++) ypart[(t * 64 + lane) * C::D3 + m] = yacc[m];
      }
    }
    if (t + 1 < C::MT2) __syncthreads();  // (uniform: every wave passes every hand-over barrier)
  }
  if (wave == C::MT2 - 1) {
    const i64 row = (tile << 5) + r;
#pragma unroll
    for (int m = 0; m < C::D3; m++) {
      const float tot = yacc[m] + __shfl_xor(yacc[m], 32);
      if (h == 0 && row < rows) Y[row * C::D3 + m] = act_c<C::A3>(tot + b3[m]);
    }
  }
}

// ---- the same for the SHORTEST launches: 16-row tiles on v_mfma_f32_16x16x4_f32 (round 5) ------------------------------------
// mlp3_tile_kernel spends 3.9 us of a DataChunk's 12 in layer 2 with two of its four waves idle: an output tile's K-long sum is one
// chain of 32x32x2 instructions (64 cycles each) and a 32-row tile has only D2 / 32 of them.  Nothing about the SUMS ties them to that
// instruction: 32x32x2, 16x16x4 and a k-ascending fmaf chain give the same bits (tools/ubench/mfma_order_probe.hip,
// profiles/r05_mfma_order_probe.txt) -- a 32x32x2 adds its two k-values h = 0, 1 in that order, a 16x16x4 its four q = 0..3.  So here a
// workgroup owns SIXTEEN rows and every sum of the split kernel is reproduced on 16x16x4 blocks (16 features x 16 rows, 32 cycles per
// four k-values): the split kernel's k order inside a group of eight is 0 4 1 5 2 6 3 7 (instruction j takes k = 8g + j from the lanes
// h = 0 and 8g + 4 + j from h = 1), which two 16x16x4 instructions s = 0, 1 walk when lane quarter q feeds k = 8g + 4 (q & 1) + 2 s + (q >> 1).
// A lane's weight operands for both come out of the SAME 16-byte fragment word of the packed blob the 32-row kernels use (components
// q >> 1 and 2 + (q >> 1) of the word of lane half q & 1), so nothing is packed twice.
//   * layer 1: wave w computes the features [64 w, 64 w + 64) as D1 / 64 blocks -- half the chain length of the 32-row kernel;
//   * bias + activation, [row][feature] image in LDS;
//   * layer 2: block t of D2 / 16 belongs to wave t mod 4 -- all four waves busy, a quarter of the 32-row kernel's time;
//   * bias + activation of layer 2 to LDS, then 32 lanes run the split kernel's two head chains per row (lane halves h = 0 / 1:
//     features 8 q + 4 h + j, q ascending) and add them the way its __shfl_xor does.
// Twice the workgroups of the 32-row kernel for a chunk (128 for 2048 rows), each a quarter of the LDS.  Bit-identical to the split
// kernel, hence to mlp3_tile_kernel (tests/test_parity_gpu.py: host path == device-resident scan; tests/test_mlp_tile16_gpu.py).
template <class C, bool XCM = false>
__global__ __launch_bounds__(256) void mlp3_tile16_kernel(const float *__restrict__ X, const float *__restrict__ packed,
                                                          float *__restrict__ Y, i64 rows) {
  static_assert(C::L3V && C::D1 % 64 == 0 && C::D2 % 16 == 0 && C::D2 <= 128, "16-row tile kernel: VALU head, D1 in 64s, D2 <= 128");
  constexpr int NB1W = C::D1 / 64;        // layer-1 blocks (16 features) per wave
  constexpr int NB2 = C::D2 / 16;         // layer-2 blocks
  constexpr int NB2W = (NB2 + 3) / 4;     // ... per wave: blocks wave, wave + 4
  constexpr int U1 = C::G0 * NB1W, U2 = C::G1 * NB2W;
  constexpr int P = 16;                   // fragment ring depth (as mlp3_tile_kernel; 8: the same 8.6 us per chunk, 32: 9.2)
  constexpr int ROWF = C::D1 + 4, ROWH = C::D2 + 4;
  __shared__ __attribute__((aligned(16))) float act[16 * ROWF];
  __shared__ __attribute__((aligned(16))) float hid[16 * ROWH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4, hq = q & 1;
  const bool jq = (q >> 1) != 0;
  const i64 tile = blockIdx.x;
  const f32x4 *w1 = reinterpret_cast<const f32x4 *>(packed + C::OFF_W1) + hq * 32 + n;
  const f32x4 *w2 = reinterpret_cast<const f32x4 *>(packed + C::OFF_W2) + hq * 32 + n;
  const float *small = packed + C::OFF_SMALL;

  // fragment word of layer-1 unit u = (group g, block t of this wave): feature block fb = wave * NB1W + t sits in the 32-wide tile fb >> 1,
  // lanes 16 (fb & 1) .. + 15 of it
  auto frag1 = [&](int u) {
    const int g = u / NB1W, fb = wave * NB1W + u % NB1W;
    return w1[(g * C::MT1 + (fb >> 1)) * 64 + 16 * (fb & 1)];
  };
  f32x4 ring[P];
#pragma unroll
  for (int u = 0; u < P && u < U1; u++) ring[u] = frag1(u);
  float xs[2 * C::G0];  // this lane's B operands: k = 8 g + 4 (q & 1) + 2 s + (q >> 1)
  {
    i64 row = tile * 16 + n;
    if (row >= rows) row = rows - 1;
    if constexpr (XCM) {
      const float *p = X + i64(4 * hq + (jq ? 1 : 0)) * rows + row;
#pragma unroll
      for (int g = 0; g < C::G0; g++) {
        xs[2 * g] = p[i64(8 * g) * rows];
        xs[2 * g + 1] = p[i64(8 * g + 2) * rows];
      }
    } else {
      const f32x4 *p = reinterpret_cast<const f32x4 *>(X + row * C::D0 + 4 * hq);
#pragma unroll
      for (int g = 0; g < C::G0; g++) {
        const f32x4 v = p[2 * g];
        xs[2 * g] = jq ? v[1] : v[0];
        xs[2 * g + 1] = jq ? v[3] : v[2];
      }
    }
  }
  f32x4 acc1[NB1W];
#pragma unroll
  for (int t = 0; t < NB1W; t++) acc1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < U1; u++) {
    const int g = u / NB1W, t = u % NB1W;
    const f32x4 a = ring[u % P];
    if (u + P < U1) ring[u % P] = frag1(u + P);
    acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(jq ? a[1] : a[0], xs[2 * g], acc1[t], 0, 0, 0);
    acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(jq ? a[3] : a[2], xs[2 * g + 1], acc1[t], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
  // layer-2 fragments of this wave's blocks: under way during the exchange
  auto frag2 = [&](int u) {
    const int g = u / NB2W, fb = wave + 4 * (u % NB2W);
    return w2[(g * C::MT2 + ((fb < NB2 ? fb : 0) >> 1)) * 64 + 16 * (fb & 1)];
  };
#pragma unroll
  for (int u = 0; u < P && u < U2; u++) ring[u] = frag2(u);
  // bias + activation (the split kernel's arithmetic when it consumes the accumulators): accumulator element i of lane (n, q) is feature
  // 16 fb + 4 q + i of row n, and the bias quads lie in feature order
  {
    const f32x4 *b1 = reinterpret_cast<const f32x4 *>(small + C::S_B1);
#pragma unroll
    for (int t = 0; t < NB1W; t++) {
      const int fb = wave * NB1W + t;
      const f32x4 bq = b1[4 * fb + q];
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = act_c<C::A1>(acc1[t][i] + bq[i]);
      *reinterpret_cast<f32x4 *>(act + n * ROWF + 16 * fb + 4 * q) = v;
    }
  }
  __syncthreads();
  // ---- layer 2 ----
  f32x4 acc2[NB2W];
#pragma unroll
  for (int t = 0; t < NB2W; t++) acc2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    const f32x4 *arow = reinterpret_cast<const f32x4 *>(act + n * ROWF + 4 * hq);
#pragma unroll
    for (int u = 0; u < U2; u++) {
      const int g = u / NB2W, t = u % NB2W;
      const f32x4 a = ring[u % P];
      if (u + P < U2) ring[u % P] = frag2(u + P);
      const f32x4 hv = arow[2 * g];
      acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(jq ? a[1] : a[0], jq ? hv[1] : hv[0], acc2[t], 0, 0, 0);
      acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(jq ? a[3] : a[2], jq ? hv[3] : hv[2], acc2[t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  {
    const f32x4 *b2 = reinterpret_cast<const f32x4 *>(small + C::S_B2);
#pragma unroll
    for (int t = 0; t < NB2W; t++) {
      const int fb = wave + 4 * t;
      if (fb < NB2) {
        const f32x4 bq = b2[4 * fb + q];
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = act_c<C::A2>(acc2[t][i] + bq[i]);
        *reinterpret_cast<f32x4 *>(hid + n * ROWH + 16 * fb + 4 * q) = v;
      }
    }
  }
  __syncthreads();
  // ---- head: per row the split kernel's two fmaf chains (lane halves h = 0 / 1), then their sum ----
  if (wave == 0 && lane < 32) {
    const int hr = lane & 15, h = lane >> 4;
    const f32x4 *w3 = reinterpret_cast<const f32x4 *>(small + C::S_W3);
    const float *b3 = small + C::S_B3;
    float yacc[C::D3];
#pragma unroll
    for (int m = 0; m < C::D3; m++) yacc[m] = 0.f;
#pragma unroll
    for (int qq = 0; qq < C::D2 / 8; qq++) {
      const f32x4 hv = *reinterpret_cast<const f32x4 *>(hid + hr * ROWH + 8 * qq + 4 * h);
#pragma unroll
      for (int m = 0; m < C::D3; m++) {
        const f32x4 wq = w3[(2 * qq + h) * C::D3 + m];
#pragma unroll
        for (int j = 0; j < 4; j++) yacc[m] = fmaf(wq[j], hv[j], yacc[m]);
      }
    }
    const i64 row = tile * 16 + hr;
#pragma unroll
    for (int m = 0; m < C::D3; m++) {
      const float tot = yacc[m] + __shfl_xor(yacc[m], 16);
      if (h == 0 && row < rows) Y[row * C::D3 + m] = act_c<C::A3>(tot + b3[m]);
    }
  }
}

}  // namespace mlpdev
}  // namespace kern
}  // namespace infera_hip
