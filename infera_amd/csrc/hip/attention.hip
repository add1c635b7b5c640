// attention.hip -- self-attention of a Transformer encoder on gfx950 (semantics: INTEGRATION.md section 2.6; caps: host/attention.hpp).
// Ahead-of-time kernels; every size is a run-time argument but the number of 16-column fragments of a head (1, 2, 4 or 8: dh <= 128).
//
// attention_kernel: for each table row and head, out = softmax(scale . Q K^T + mask) V over the row's T steps.  A workgroup owns one
// (row, head) and up to 64 queries of it: one wave per 16-query tile (min(4, ceil(T / 16)) waves).  Keys / values are walked in tiles of
// 32 in a fixed order with a running maximum and sum per query (online softmax), so T is not bounded by LDS; each K / V tile is staged
// in LDS once for all waves of the workgroup (16-byte global loads where dh, the row strides and the pointers allow, else word loads).
// Both products run on v_mfma_f32_16x16x4_f32 (exact f32, a fixed k order per output):
//   S^T[key][query] = K . Q^T:  A = K tile from LDS (lane (m, kq) reads the 16 bytes of key m at columns 16 c + 4 kq), B = Q^T held in
//       registers for the whole kernel.  The accumulator leaves lane (n, kq) with the scores of query n against keys 4 kq .. 4 kq + 3.
//   O^T[d][query]  += V^T . P^T: MFMA i of a 16-key tile takes as its four k indices the keys {4 kq + i}: lane (n, kq) then supplies
//       P[n][4 kq + i], which IS its accumulator register i -- the P fragment needs no re-layout through LDS or lane moves at all; only
//       the order in which the 16 keys of a tile are summed is permuted (fixed, so still deterministic).  A = V[4 kq + i][16 dt + m].
// LDS rows are padded by 4 words (stride dhp + 4) so that the 16 key rows a K read touches, and the 4 key rows a V read touches, start
// in different banks; whether the 16-byte K reads are then free of conflicts was not checked with counters.
// Only 1, 2, 4 and 8 column fragments are instantiated: dh in 33..48 runs the 4-fragment kernel and dh in 65..112 the 8-fragment one,
// with zero columns in the rest -- up to 2 x the MFMAs and LDS such a head needs (dh = 40 does the work of 64, dh = 80 that of 128).
// The scale is applied to the f32 scores (s = scale * (q . k) + mask), wherever the graph applied it.  Keys beyond T and keys whose mask
// entry is -inf are excluded BEFORE the maximum and get weight exactly 0 (no large negative number); padded head columns are zero in
// Q, K and V.  The per-query sum is kept as four per-lane partial sums (one per kq) added once at the end.  No atomics, nothing depends
// on the grid: a row's bits depend on the model and the row only, and a NaN stays in its own row (rows never share a workgroup).
//
// Short windows: T = 24 runs 2 waves per workgroup, T <= 16 one; a 2048-row chunk with 4 heads is still 8192 workgroups, so the chip is
// full, but each wave's MFMAs wait on its own shuffles and exponentials with little to overlap.  Packing several rows into one
// workgroup for small T and double buffering of the K / V tiles were considered and NOT built, so there is no A/B for them; what was
// measured is this one form (tools/transformer_time.py, profiles/r11_transformer.txt): its rate, its fraction of the f32 MFMA peak, and
// its time beside torch-ROCm's float32 scaled_dot_product_attention on the same tensors: 0.10 of the peak at T = 24 and 0.30 at T = 128
// (dh = 16: four MFMAs per product between shuffles and expf, nothing overlapped), 0.64 x / 0.83 x torch's time -- slower on neither.
//
// Row masks (attention_kernel<DT, true>; INTEGRATION.md 2.6 "Padded sequences"): a row's own key mask is T values of the
// model's input buffer.  The workgroup first turns them into a kept-bitmap in LDS (one ballot per 64 keys, at most 32 words).  With an
// excluding fill, in a row that keeps a key, a masked key is a key beyond T: staged as zeros without being read, its score -inf before
// the maximum; a 32-key tile whose word is 0 is skipped before its staging loads and a 16-key sub-tile whose half-word is 0 before its
// MFMAs -- both branches are the same in every thread of the workgroup.  Otherwise (a bias fill, or a row that keeps no key) the fill goes
// into the score and nothing is skipped.  The <DT, false> kernels are the code above, unchanged.
//
// The Attention operator (attention_kernel<DT, ROWMASK, FORM>; INTEGRATION.md 2.6 "The Attention operator").  FORM 0 is the
// kernel described above, instruction for instruction what it was before the operator came (its two extra arguments stand at the end of
// AttnArgs and are not read), so every model that loaded before returns the same bits at the same speed.  FORM 1: T queries against Tk
// keys (Q rows are T * ldq apart, K / V rows Tk * ldk / Tk * ldv, the constant mask is [T, Tk]) and grouped heads: query head g reads the
// K / V head g / G.  One workgroup still serves one query head: letting it serve the G heads of a group from one staged K / V tile was NOT
// built, so there is no A/B for it; what grouping saves today is K / V traffic through the cache (tools/attention_op_time.py).
// FORM 2 adds is_causal (key j counts for query i iff j <= i, top-left aligned): the workgroup's key loop ends at min(Tk, its last query
// + 1) -- one bound for all its threads, so the barriers stay matched -- a wave leaves the sub-tile loop at the first 16-key sub-tile that
// lies wholly above its last query (wave-uniform, no barrier inside that loop), and inside the diagonal tiles a key j > i gets the score
// -inf before the maximum, after any row-mask fill: exactly what a constant -inf mask entry gets.  A tile that is not visited contributes
// corr = 1, p = 0, so for finite inputs the result has the bits of the constant [T, T] causal mask through FORM 0 (tests/
// test_attention_op_gpu.py; the sign of an accumulator that underflowed to -0 is the one thing a visited all-masked tile would change).
// A NaN in K / V at step j reaches the queries i >= j as the definition says; a query i < j sees it (0 . NaN) only where its wave visited
// the key's tile.  The row-mask bitmap, its tile skipping and the causal bounds compose; no LDS beyond what ROWMASK has, no spills.
#include "device_common.hpp"

#include <cstdlib>

#include "../host/attention.hpp"

namespace infera_hip::kern {

namespace {

constexpr int kAttnKeyTile = 32, kAttnMaxWaves = 4;

struct AttnArgs {
  const float *q, *k, *v, *mask;
  float *y;
  int T, H, dh, ldq, ldk, ldv, offq, offk, offv;
  float scale;
  bool vec;
  // the row's own key mask (ROWMASK kernels; INTEGRATION.md 2.6 "Padded sequences"): key j of a row is kept iff rm[row * rm_ld + rm_off + j]
  // (truncated toward zero first when rm_int) != rm_cmp.  rm_excl: a masked key is a key beyond T (in rows that keep a key); else its
  // score is sc + rm_fill (rm_mode kRowMaskAdd) or rm_fill (kRowMaskReplace).  rm_skip: wholly masked tiles are not visited
  const float *rm;
  int64_t rm_ld;
  int rm_off;
  float rm_cmp, rm_fill;
  int rm_mode;
  bool rm_excl, rm_int, rm_skip;
  // the operator form (FORM > 0; INTEGRATION.md 2.6 "The Attention operator"): T queries against Tk keys, query head g reads K / V head
  // g / G (G = query heads per K / V head).  FORM 0 reads neither: Tk = T, G = 1
  int Tk, G;
};

// FORM 0: the pattern form's kernel, as it was; 1: the operator with Tk != T or grouped heads; 2: the operator under is_causal
template <int DT, bool ROWMASK, int FORM>
__global__ __launch_bounds__(kAttnMaxWaves * 64) void attention_kernel(AttnArgs a) {
  constexpr int DP = DT * 16, LS = DP + 4, QPR = DP / 4;
  constexpr bool CAUSAL = FORM == 2;
  __shared__ __attribute__((aligned(16))) float ks[kAttnKeyTile * LS];
  __shared__ __attribute__((aligned(16))) float vs[kAttnKeyTile * LS];
  __shared__ unsigned kept[ROWMASK ? kAttnMaxT / 32 : 1];  // ROWMASK: bit (j & 31) of word j / 32 = key j is kept
  const int tid = int(threadIdx.x), nth = int(blockDim.x), nw = nth >> 6, wave = tid >> 6, lane = tid & 63, n = lane & 15, kq = lane >> 4;
  const int64_t row = int64_t(blockIdx.x) / a.H;
  const int head = int(int64_t(blockIdx.x) - row * a.H), T = a.T, Tk = FORM ? a.Tk : a.T, dh = a.dh;
  const int qi = (int(blockIdx.y) * nw + wave) * 16 + n;
  const float *qp = a.q + row * T * a.ldq + a.offq + head * dh;
  const int kv_head = FORM ? head / a.G : head;
  const float *kp = a.k + row * Tk * a.ldk + a.offk + kv_head * dh;
  const float *vp = a.v + row * Tk * a.ldv + a.offv + kv_head * dh;
  // CAUSAL: key j counts for query i iff j <= i.  No query of the workgroup reads a key beyond its last query (the same bound in every
  // thread), and a wave visits no 16-key sub-tile that lies wholly above its own last query
  int kend = Tk;
  if constexpr (CAUSAL) {
    const int wg_last = (int(blockIdx.y) + 1) * nw * 16 < T ? (int(blockIdx.y) + 1) * nw * 16 : T;  // one past the workgroup's last query
    kend = wg_last < Tk ? wg_last : Tk;
  }
  [[maybe_unused]] const int wave_last = (int(blockIdx.y) * nw + wave) * 16 + 15;

  // up to four consecutive head columns of one step: zero beyond dh
  auto load4 = [&](const float *p, int d) -> f32x4 {
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (a.vec) {
      if (d < dh) r = *reinterpret_cast<const f32x4 *>(p + d);  // (dh % 4 == 0: a quad is inside or outside as a whole)
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (d + j < dh) r[j] = p[d + j];
    }
    return r;
  };

  f32x4 qr[DT], o[DT];
#pragma unroll
  for (int c = 0; c < DT; c++) {
    qr[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (qi < T) qr[c] = load4(qp + int64_t(qi) * a.ldq, 16 * c + 4 * kq);
    o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float m_run = -INFINITY, l_run = 0.f;

  // ROWMASK: the kept bitmap of the row (64 keys per ballot, so a wave writes two words at a time), and whether its masked keys are
  // excluded: only with an excluding fill AND a kept key.  Both are the same in every thread of the workgroup
  bool excl = false, skip = false;
  if constexpr (ROWMASK) {
    const float *mp = a.rm + row * a.rm_ld + a.rm_off;
    for (int base = wave * 64; base < Tk; base += nw * 64) {
      const int key = base + lane;
      bool kp = false;
      if (key < Tk) {
        const float mv = mp[key];
        kp = (a.rm_int ? truncf(mv) : mv) != a.rm_cmp;  // (a NaN is unequal: kept)
      }
      const unsigned long long b = __ballot(kp);
      if (lane == 0) {
        kept[base >> 5] = unsigned(b);
        kept[(base >> 5) + 1] = unsigned(b >> 32);
      }
    }
    __syncthreads();
    unsigned any = 0;
    for (int w = 0; w < (Tk + 31) >> 5; w++) any |= kept[w];
    excl = a.rm_excl && any != 0;
    skip = excl && a.rm_skip;
  }

  for (int k0 = 0; k0 < kend; k0 += kAttnKeyTile) {
    unsigned kw = 0xffffffffu;
    if constexpr (ROWMASK) {
      kw = kept[k0 >> 5];
      if (skip && kw == 0) continue;  // (the same branch in every thread: the barriers below stay matched)
    }
    __syncthreads();  // the previous tile has been read by every wave
    for (int e = tid; e < kAttnKeyTile * QPR; e += nth) {
      const int key = e / QPR, d = (e - key * QPR) * 4;
      f32x4 kk = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
      bool in = k0 + key < Tk;
      if constexpr (ROWMASK) in = in && (!excl || ((kw >> key) & 1u));  // an excluded key is never read
      if (in) {
        kk = load4(kp + int64_t(k0 + key) * a.ldk, d);
        vv = load4(vp + int64_t(k0 + key) * a.ldv, d);
      }
      *reinterpret_cast<f32x4 *>(ks + key * LS + d) = kk;
      *reinterpret_cast<f32x4 *>(vs + key * LS + d) = vv;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < kAttnKeyTile / 16; sub++) {
      if (k0 + 16 * sub >= Tk) break;
      if constexpr (CAUSAL)
        if (k0 + 16 * sub > wave_last) break;  // (the same in every lane of the wave; no barrier inside this loop)
      if constexpr (ROWMASK)
        if (skip && ((kw >> (16 * sub)) & 0xffffu) == 0) continue;
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < DT; c++) {
        const f32x4 kf = *reinterpret_cast<const f32x4 *>(ks + (16 * sub + n) * LS + 16 * c + 4 * kq);
#pragma unroll
        for (int j = 0; j < 4; j++) s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j], qr[c][j], s, 0, 0, 0);
      }
      float sc[4], mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int key = k0 + 16 * sub + 4 * kq + i;
        sc[i] = -INFINITY;
        if (key < Tk) {
          sc[i] = s[i] * a.scale;
          if (a.mask && qi < T) sc[i] += a.mask[int64_t(qi) * Tk + key];
          if constexpr (ROWMASK)
            if (!((kw >> (16 * sub + 4 * kq + i)) & 1u)) sc[i] = excl ? -INFINITY : a.rm_mode == kRowMaskAdd ? sc[i] + a.rm_fill : a.rm_fill;
          if constexpr (CAUSAL)
            if (key > qi) sc[i] = -INFINITY;  // (what a constant -inf mask entry gives)
        }
        mx = fmaxf(mx, sc[i]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run, mx);
      const float corr = m_new == -INFINITY ? 1.f : expf(m_run - m_new);
      float p[4], ps = 0.f;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        p[i] = sc[i] == -INFINITY ? 0.f : expf(sc[i] - m_new);
        ps += p[i];
      }
      l_run = l_run * corr + ps;
      m_run = m_new;
#pragma unroll
      for (int dt = 0; dt < DT; dt++) {
#pragma unroll
        for (int i = 0; i < 4; i++) o[dt][i] *= corr;
#pragma unroll
        for (int i = 0; i < 4; i++)
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vs[(16 * sub + 4 * kq + i) * LS + 16 * dt + n], p[i], o[dt], 0, 0, 0);
      }
    }
  }
  l_run += __shfl_xor(l_run, 16);
  l_run += __shfl_xor(l_run, 32);
  if (qi >= T) return;
  float *yp = a.y + (row * T + qi) * int64_t(a.H) * dh + head * dh;
#pragma unroll
  for (int dt = 0; dt < DT; dt++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int d = 16 * dt + 4 * kq + i;
      if (d < dh) yp[d] = o[dt][i] / l_run;
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int DT>
void launch_attention(hipStream_t s, dim3 grid, dim3 block, const AttnArgs &a, bool rowmask, bool causal) {
  const int form = causal ? 2 : a.Tk != a.T || a.G != 1 ? 1 : 0;
  if (rowmask) {
    if (form == 2) hipLaunchKernelGGL((attention_kernel<DT, true, 2>), grid, block, 0, s, a);
    else if (form == 1) hipLaunchKernelGGL((attention_kernel<DT, true, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((attention_kernel<DT, true, 0>), grid, block, 0, s, a);
  } else {
    if (form == 2) hipLaunchKernelGGL((attention_kernel<DT, false, 2>), grid, block, 0, s, a);
    else if (form == 1) hipLaunchKernelGGL((attention_kernel<DT, false, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((attention_kernel<DT, false, 0>), grid, block, 0, s, a);
  }
}

}  // namespace

bool attention(hipStream_t s, const float *q, const float *k, const float *v, const float *mask, float *y, int64_t rows, int T, int heads, int dh,
               const int64_t ld[3], const int64_t off[3], float scale, const float *rm, int64_t rm_ld, int rm_off, float rm_cmp, float rm_fill, int rm_mode,
               bool rm_excl, bool rm_int, int Tk, int kv_heads, bool causal) {
  if (rows <= 0) return true;
  if (Tk <= 0) Tk = T;
  if (kv_heads <= 0) kv_heads = heads;
  if (T < 1 || T > kAttnMaxT || Tk > kAttnMaxT || dh < 1 || dh > kAttnMaxDh || heads < 1 || heads > kAttnMaxHeads || heads % kv_heads != 0 || rows * heads > INT32_MAX)
    return false;
  if (rm && (mask || rm_off < 0 || int64_t(rm_off) + Tk > rm_ld)) return false;
  // INFERA_ATTN_SKIP=0 (read once per process): wholly masked tiles are visited like the others, with zeros staged and -inf scores -- the
  // same results; the A/B of tools/padded_time.py
  static const bool skip_tiles = !(getenv("INFERA_ATTN_SKIP") && atoi(getenv("INFERA_ATTN_SKIP")) == 0);
  AttnArgs a{q, k, v, mask, y, T, heads, dh, int(ld[0]), int(ld[1]), int(ld[2]), int(off[0]), int(off[1]), int(off[2]), scale, false,
             rm, rm_ld, rm_off, rm_cmp, rm_fill, rm_mode, rm_excl, rm_int, skip_tiles, Tk, heads / kv_heads};
  a.vec = dh % 4 == 0 && aligned16(q) && aligned16(k) && aligned16(v);
  for (int i = 0; i < 3; i++) a.vec = a.vec && ld[i] % 4 == 0 && off[i] % 4 == 0;
  const int tiles = (T + 15) / 16, nw = tiles < kAttnMaxWaves ? tiles : kAttnMaxWaves;
  const dim3 grid(unsigned(rows * heads), unsigned((tiles + nw - 1) / nw)), block(unsigned(64 * nw));
  const int dt = (dh + 15) / 16;
  if (dt <= 1) launch_attention<1>(s, grid, block, a, rm != nullptr, causal);
  else if (dt <= 2) launch_attention<2>(s, grid, block, a, rm != nullptr, causal);
  else if (dt <= 4) launch_attention<4>(s, grid, block, a, rm != nullptr, causal);
  else launch_attention<8>(s, grid, block, a, rm != nullptr, causal);
  return true;
}

}  // namespace infera_hip::kern
