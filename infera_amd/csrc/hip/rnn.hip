// rnn.hip -- ONNX LSTM / GRU / RNN on gfx950 (semantics: INTEGRATION.md section 2.6; tables: host/recurrent.hpp).  Ahead-of-time
// kernels, one per operator; sizes are run-time arguments (nothing is specialised at load).
//
// rnn_kernel: a workgroup owns 16 table rows and one direction for all T steps; rows lie on the MFMA N axis.  Per step the gate
// pre-activations are [W | R] . [x_t ; h_{t-1}] on v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fma chain per output):
//   A = [W | R] straight from L2 in fragment order (host/recurrent.hpp RnnPack::wr: one 16-byte load per lane feeds four k-steps of one
//       gate; the G gates of a k-group are adjacent, so their MFMAs are independent accumulators back to back),
//   B = [x_t ; h_{t-1}] from LDS as [k][16 rows]: lane l reads word 64 q + l of k-group q -- linear, conflict-free.
// The hidden units are 16-unit tiles spread over the workgroup's waves (min(H / 16, 8) waves, up to 4 tiles each: H <= 512).  A wave
// computes all G gates of its tiles, so lane (row n, units 4 (l >> 4) .. + 3) holds every gate of its own (unit, row) elements: the sigma /
// tanh tail, c_t and the copy of h_{t-1} it needs stay in its registers for the whole sequence.  h_t goes to the other of two LDS
// copies (one exchange per step: every wave needs all of h_t as the B operand of step t + 1) and, in Y mode, to HBM once.  x_{t+1} is
// fetched into registers before the MFMAs of step t and stored to LDS behind the step's barrier.  This is the "units split across
// the waves" form for every H: the single-wave form that feeds D registers back as the next B operand without LDS is not built (it
// serves H <= 64 only and needs sizes at compile time).  W | R are re-read from L2 every step (73 KB for LSTM H = 64, F = 8; the
// 128 workgroups of a 2048-row chunk share it), not held in LDS.
//   GRU linear_before_reset = 0 needs r before R_h (r (.) h): r (.) h_{t-1} is exchanged through the not-yet-written h copy and gate
//   h's recurrent product runs as a second phase (two more barriers per step).
// Directions of a bidirectional layer are blockIdx.y.  Padded units (H..Hp) have zero weights, biases and state, and their h is written
// as 0 whatever their accumulators hold (0 . inf = NaN under an infinite reading), so a row's padded units never reach its real ones.
// Input: row-major [rows, T, F], or ONE column-major staged chunk [T * F][rows] (x_colmajor): the same loads with another index.
// A row's bits depend on the model and the row only: no atomics, the k order is fixed, rows never mix (a NaN poisons its own column).
// Per-row sequence lengths (sequence_lens, a column of the row-major input buffer) are the LENS = true instantiations: see rnn_kernel.
//
// Occupancy: a 2048-row DataChunk is 128 tiles = 128 workgroups per direction on 256 CUs -- half the chip, one workgroup per CU,
// min(H / 16, 8) waves each.  The recurrence is serial in T, so a chunk's time is T x (MFMA chain + sigma / tanh tail + 2 barriers);
// rows beyond ~4096 add workgroups side by side at no cost until every CU holds several.  profiles/r10_recurrent.txt has the figures.
#include "device_common.hpp"

#include "../host/recurrent.hpp"

namespace infera_hip::kern {

namespace {

constexpr int kRnnMaxWaves = 8, kRnnTilesPerWave = 4, kRnnPrefetch = 2;

// Per-row sequence lengths (LENS kernels; INTEGRATION.md 2.6 "Padded windows"): row r holds len = src[r * ld + off] valid steps (truncated
// toward zero first when is_int), 0 <= len <= T.  Any other value (NaN included) counts as 0 and sets the call's failure word to `node`.
struct RnnLens {
  const float *src;
  int64_t ld;
  int off;
  bool is_int;
  int *err;
  int node;
};

// LENS = false is the fixed-length kernel: every lengths statement below stands behind `if constexpr (LENS)`, and the lengths argument
// exists in the LENS = true signature alone (LA: one RnnLens, or nothing).
// LENS = true: a row with length L gives what the layer gives on its first L steps alone.  The tile's 16 lengths lie in 16 words of LDS
// behind the h copies (x_t is fetched by element, so a thread needs the length of any of the 16 rows); the step loop runs to the tile's
// longest row (the same value in every wave: the barriers stay uniform).  At step s a row is active iff s < L and stands at t = s
// (forward) or L - 1 - s (reverse); an inactive row is not read (its x_t is 0 without a load), keeps h and c by selects, still writes its
// kept h to the other LDS copy (the double buffer flips every step) and writes Y[s] = 0 (s >= L in both directions).
template <int OP, bool LENS, typename... LA>
__global__ __launch_bounds__(kRnnMaxWaves * 64) void rnn_kernel(const float *__restrict__ x, const f32x4 *__restrict__ wr, const float *__restrict__ bias,
                                                               const float *__restrict__ bias2, const float *__restrict__ h0,
                                                               const float *__restrict__ c0, float *__restrict__ y, int64_t nr, int T, int F, int H,
                                                               int Fp, int Hp, int D, bool reverse1, bool lbr, bool relu, int mode, bool xcm, LA... la) {
  static_assert(sizeof...(LA) == (LENS ? 1 : 0), "LENS: one RnnLens argument");
  constexpr int G = OP == kRnnLstm ? 4 : OP == kRnnGru ? 3 : 1;
  constexpr int NA = OP == kRnnGru ? 4 : G;  // GRU: z, r, W_h x, R_h h
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *xb = lds;            // [Fp][16]
  float *hb = lds + Fp * 16;  // [2][Hp][16]
  [[maybe_unused]] int *ln = reinterpret_cast<int *>(hb + 2 * Hp * 16);  // LENS: [16]
  const int tid = int(threadIdx.x), nth = int(blockDim.x), nw = nth >> 6, wave = tid >> 6, lane = tid & 63, n = lane & 15, kq = lane >> 4;
  const int d = int(blockIdx.y);
  const bool rev = D == 2 ? d == 1 : reverse1;
  const int64_t row0 = int64_t(blockIdx.x) * 16, row = row0 + n;
  const int HT = Hp >> 4, XQ = Fp >> 4, KQ = XQ + HT, NE = F * 16;
  wr += int64_t(d) * HT * KQ * G * 64;
  bias += d * G * Hp;
  bias2 += d * Hp;
  h0 += d * Hp;
  c0 += d * Hp;

  [[maybe_unused]] int Ln = 0, Tmax = T;  // LENS: this lane's row's length, the tile's longest
  if constexpr (LENS) {
    const RnnLens lens = (la, ...);
    if (tid < 16) {
      int L = 0;
      if (row0 + tid < nr) {
        float v = lens.src[(row0 + tid) * lens.ld + lens.off];
        if (lens.is_int) v = truncf(v);
        if (v >= 0.f && v <= float(T)) L = int(v);  // (a NaN fails both)
        else *lens.err = lens.node;
      }
      ln[tid] = L;
    }
    __syncthreads();
    Ln = ln[n];
    Tmax = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) Tmax = ln[i] > Tmax ? ln[i] : Tmax;
  }

  // element e of the 16 x F values of step t: its value and its LDS word.  LENS: t is the step count s, the element's own row's position
  // follows from its length, and an inactive row's element is 0 without a load
  auto xload = [&](int e, int t) -> float {
    int f, nn;
    if (xcm) f = e >> 4, nn = e & 15;
    else nn = e / F, f = e - nn * F;
    const int64_t g = row0 + nn;
    if (g >= nr) return 0.f;
    if constexpr (LENS) {
      const int L = ln[nn];
      if (t >= L) return 0.f;
      if (rev) t = L - 1 - t;
    }
    return xcm ? x[(int64_t(t) * F + f) * nr + g] : x[(g * T + t) * F + f];
  };
  auto xslot = [&](int e) -> int {
    if (xcm) return e;
    const int nn = e / F;
    return (e - nn * F) * 16 + nn;
  };
  float pf[kRnnPrefetch];
  auto prefetch = [&](int t) {
#pragma unroll
    for (int i = 0; i < kRnnPrefetch; i++) {
      const int e = tid + i * nth;
      pf[i] = e < NE ? xload(e, t) : 0.f;
    }
  };
  auto commit = [&](int t) {
#pragma unroll
    for (int i = 0; i < kRnnPrefetch; i++) {
      const int e = tid + i * nth;
      if (e < NE) xb[xslot(e)] = pf[i];
    }
    for (int e = tid + kRnnPrefetch * nth; e < NE; e += nth) xb[xslot(e)] = xload(e, t);
  };

  const int t_first = LENS ? 0 : rev ? T - 1 : 0;
  prefetch(t_first);
  commit(t_first);
  for (int e = NE + tid; e < Fp * 16; e += nth) xb[e] = 0.f;  // padded features
  for (int e = tid; e < Hp * 16; e += nth) hb[e] = h0[e >> 4];
  f32x4 c[kRnnTilesPerWave], hp[kRnnTilesPerWave];
#pragma unroll
  for (int q = 0; q < kRnnTilesPerWave; q++) {
    const int tile = wave + q * nw;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      c[q][i] = tile < HT && OP == kRnnLstm ? c0[16 * tile + 4 * kq + i] : 0.f;
      hp[q][i] = tile < HT ? h0[16 * tile + 4 * kq + i] : 0.f;
    }
  }
  __syncthreads();

  const int TS = LENS ? Tmax : T;
  for (int s = 0; s < TS; s++) {
    const int t = LENS ? (rev ? Ln - 1 - s : s) : rev ? T - 1 - s : s, cur = s & 1;
    [[maybe_unused]] const bool active = s < Ln;
    const float *hc = hb + cur * Hp * 16;
    float *hn = hb + (cur ^ 1) * Hp * 16;
    if (s + 1 < TS) prefetch(LENS ? s + 1 : rev ? t - 1 : t + 1);

    f32x4 acc[kRnnTilesPerWave][NA];
#pragma unroll
    for (int q = 0; q < kRnnTilesPerWave; q++) {
      const int tile = wave + q * nw;
#pragma unroll
      for (int g = 0; g < NA; g++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[q][g][i] = 0.f;
      if (tile >= HT) continue;
      const f32x4 *wt = wr + int64_t(tile) * KQ * G * 64 + lane;
      for (int kk = 0; kk < XQ; kk++) {
        f32x4 a[G];
#pragma unroll
        for (int g = 0; g < G; g++) a[g] = wt[(kk * G + g) * 64];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float b = xb[(16 * kk + 4 * j + kq) * 16 + n];
#pragma unroll
          for (int g = 0; g < G; g++) acc[q][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][j], b, acc[q][g], 0, 0, 0);
        }
      }
      for (int kk = 0; kk < HT; kk++) {
        f32x4 a[G];
#pragma unroll
        for (int g = 0; g < G; g++) a[g] = wt[((XQ + kk) * G + g) * 64];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float b = hc[(16 * kk + 4 * j + kq) * 16 + n];
#pragma unroll
          for (int g = 0; g < G; g++) {
            if (OP == kRnnGru && g == 2) {
              if (lbr) acc[q][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][j], b, acc[q][3], 0, 0, 0);
            } else {
              acc[q][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][j], b, acc[q][g], 0, 0, 0);
            }
          }
        }
      }
    }

    if (OP == kRnnGru && !lbr) {  // R_h (r (.) h_{t-1}): r (.) h through the free h copy, then gate h's recurrent product
#pragma unroll
      for (int q = 0; q < kRnnTilesPerWave; q++) {
        const int tile = wave + q * nw;
        if (tile >= HT) continue;
        const f32x4 br = *reinterpret_cast<const f32x4 *>(bias + 1 * Hp + 16 * tile + 4 * kq);
#pragma unroll
        for (int i = 0; i < 4; i++)  // (a padded unit: 0, not sigma(0 . inf) . 0)
          hn[(16 * tile + 4 * kq + i) * 16 + n] = 16 * tile + 4 * kq + i < H ? apply_act_c<2>(acc[q][1][i] + br[i], 0.f, 0.f) * hp[q][i] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kRnnTilesPerWave; q++) {
        const int tile = wave + q * nw;
        if (tile >= HT) continue;
        const f32x4 *wt = wr + int64_t(tile) * KQ * G * 64 + lane;
        for (int kk = 0; kk < HT; kk++) {
          const f32x4 a = wt[((XQ + kk) * G + 2) * 64];
#pragma unroll
          for (int j = 0; j < 4; j++)
            acc[q][NA - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], hn[(16 * kk + 4 * j + kq) * 16 + n], acc[q][NA - 1], 0, 0, 0);
        }
      }
      __syncthreads();
    }

#pragma unroll
    for (int q = 0; q < kRnnTilesPerWave; q++) {
      const int tile = wave + q * nw;
      if (tile >= HT) continue;
      const int j0 = 16 * tile + 4 * kq;
      f32x4 bg[G];
#pragma unroll
      for (int g = 0; g < G; g++) bg[g] = *reinterpret_cast<const f32x4 *>(bias + g * Hp + j0);
      f32x4 h;
      if constexpr (OP == kRnnLstm) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float gi = apply_act_c<2>(acc[q][0][i] + bg[0][i], 0.f, 0.f), go = apply_act_c<2>(acc[q][1][i] + bg[1][i], 0.f, 0.f);
          const float gf = apply_act_c<2>(acc[q][2][i] + bg[2][i], 0.f, 0.f), gc = apply_act_c<3>(acc[q][3][i] + bg[3][i], 0.f, 0.f);
          float cn;
          if constexpr (LENS) {
            // fma(f, c, i . g), written out: it is how the fixed-length instantiation contracts the line below, and around the select
            // the compiler would not (tests/test_recurrent_lens_gpu.py compares the two instantiations bit for bit)
            cn = __builtin_fmaf(gf, c[q][i], gi * gc);
            cn = active ? cn : c[q][i];
          } else {
            cn = gf * c[q][i] + gi * gc;
          }
          c[q][i] = cn;
          h[i] = go * apply_act_c<3>(cn, 0.f, 0.f);
        }
      } else if constexpr (OP == kRnnGru) {
        const f32x4 b2 = *reinterpret_cast<const f32x4 *>(bias2 + j0);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float z = apply_act_c<2>(acc[q][0][i] + bg[0][i], 0.f, 0.f);
          float pre;
          if (lbr) pre = acc[q][2][i] + apply_act_c<2>(acc[q][1][i] + bg[1][i], 0.f, 0.f) * (acc[q][3][i] + b2[i]) + bg[2][i];
          else pre = acc[q][2][i] + acc[q][3][i] + bg[2][i];
          h[i] = (1.f - z) * apply_act_c<3>(pre, 0.f, 0.f) + z * hp[q][i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float v = acc[q][0][i] + bg[0][i];
          h[i] = relu ? apply_act_c<1>(v, 0.f, 0.f) : apply_act_c<3>(v, 0.f, 0.f);
        }
      }
      // A padded unit's zero weights meet an infinite reading as 0 . inf = NaN: its h is 0 by definition, not by arithmetic, or the NaN
      // would reach every unit of the row through the next step's B operand (0 . NaN).
#pragma unroll
      for (int i = 0; i < 4; i++) h[i] = j0 + i < H ? h[i] : 0.f;
      if constexpr (LENS) {
#pragma unroll
        for (int i = 0; i < 4; i++) h[i] = active ? h[i] : hp[q][i];
      }
      hp[q] = h;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        hn[(j0 + i) * 16 + n] = h[i];
        if constexpr (LENS) {
          if (mode == kRnnY && j0 + i < H && row < nr) y[((row * T + (active ? t : s)) * D + d) * H + j0 + i] = active ? h[i] : 0.f;
        } else {
          if (mode == kRnnY && j0 + i < H && row < nr) y[((row * T + t) * D + d) * H + j0 + i] = h[i];
        }
      }
    }
    __syncthreads();  // h_t is complete; nobody reads x_t or h_{t-1} any more
    if (s + 1 < TS) {
      commit(LENS ? s + 1 : rev ? t - 1 : t + 1);
      __syncthreads();
    }
  }
  if constexpr (LENS) {  // no row of the tile reaches the steps Tmax .. T - 1: written zeros (the buffer is not cleared)
    if (mode == kRnnY) {
      const int64_t HR = int64_t(H) * 16;
      for (int64_t e = tid; e < HR * (T - Tmax); e += nth) {
        const int64_t tt = Tmax + e / HR, r = row0 + (e % HR) / H;
        if (r < nr) y[((r * T + tt) * D + d) * H + e % H] = 0.f;
      }
    }
  }

  if (mode != kRnnY) {
#pragma unroll
    for (int q = 0; q < kRnnTilesPerWave; q++) {
      const int tile = wave + q * nw;
      if (tile >= HT) continue;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int j = 16 * tile + 4 * kq + i;
        if (j < H && row < nr) y[(row * D + d) * H + j] = mode == kRnnYc ? c[q][i] : hp[q][i];
      }
    }
  }
}

// la: the RnnLens of a LENS launch, or nothing
template <int OP, bool LENS, typename... LA>
bool launch(hipStream_t s, const float *x, const float *wr, const float *bias, const float *bias2, const float *h0, const float *c0, float *y, int64_t rows,
            int T, int F, int H, int D, bool reverse, bool lbr, bool relu, int mode, bool xcm, LA... la) {
  const int Fp = (F + 15) / 16 * 16, Hp = (H + 15) / 16 * 16, HT = Hp / 16;
  const int nw = HT < kRnnMaxWaves ? HT : kRnnMaxWaves;
  const size_t lds = size_t(Fp + 2 * Hp) * 16 * 4 + (LENS ? 16 * 4 : 0);
  auto kernel = rnn_kernel<OP, LENS, LA...>;
  if (lds > 64 * 1024 &&  // dynamic LDS beyond 64 KB is opt-in (128 KB at the caps)
      hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
    return false;
  hipLaunchKernelGGL(kernel, dim3(unsigned((rows + 15) / 16), unsigned(D)), dim3(unsigned(64 * nw)), lds, s, x, reinterpret_cast<const f32x4 *>(wr), bias,
                     bias2, h0, c0, y, rows, T, F, H, Fp, Hp, D, reverse, lbr, relu, mode, xcm, la...);
  return true;
}

}  // namespace

static_assert(kRnnMaxH <= 16 * kRnnMaxWaves * kRnnTilesPerWave, "the hidden units of the cap fit the workgroup");

bool rnn(hipStream_t s, const float *x, const float *wr, const float *bias, const float *bias2, const float *h0, const float *c0, float *y, int64_t rows,
         int op, int T, int F, int H, int D, bool reverse, bool lbr, bool relu, int mode, bool x_colmajor, const float *lens, int64_t lens_ld, int lens_off,
         bool lens_int, int *err, int err_node) {
  if (rows <= 0) return true;
  // (lengths are read as a column of a row-major buffer beside a row-major x; the failure word is theirs)
  if (lens && (x_colmajor || !err || lens_off < 0 || lens_off >= lens_ld)) return false;
  const RnnLens ln{lens, lens_ld, lens_off, lens_int, err, err_node};
#define INFERA_RNN_LAUNCH(OP) \
  (lens ? launch<OP, true>(s, x, wr, bias, bias2, h0, c0, y, rows, T, F, H, D, reverse, lbr, relu, mode, x_colmajor, ln) \
        : launch<OP, false>(s, x, wr, bias, bias2, h0, c0, y, rows, T, F, H, D, reverse, lbr, relu, mode, x_colmajor))
  if (op == kRnnLstm) return INFERA_RNN_LAUNCH(kRnnLstm);
  if (op == kRnnGru) return INFERA_RNN_LAUNCH(kRnnGru);
  return INFERA_RNN_LAUNCH(kRnnPlain);
#undef INFERA_RNN_LAUNCH
}

}  // namespace infera_hip::kern
