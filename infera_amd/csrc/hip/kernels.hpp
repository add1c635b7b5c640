// kernels.hpp -- host-callable launchers for the gfx950 kernels.  Every launcher enqueues on the
// given stream and returns immediately; errors surface through hipGetLastError at the call site.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>
#include <vector>

namespace infera_hip::kern {

// Activation codes shared with plan.hpp (Act enum values).
struct ActParam {
  int kind = 0;  // plan.hpp Act: 0 none, 1 relu, 2 sigmoid, 3 tanh, 4 leaky-relu(a), 5 clip(a,b), 6.. elementwise-only kinds
  float a = 0.f, b = 0.f;
};

// ---- elementwise / reductions (eltwise.hip) --------------------------------------------------
void unary(hipStream_t s, const float *x, float *y, int64_t n, ActParam act);
// y = (sat(rne(x / scale) + zp) - zp) * scale with the range [qmin, qmax]   (QuantizeLinear -> DequantizeLinear)
void fake_quant(hipStream_t s, const float *x, float *y, int64_t n, float scale, int zp, int qmin, int qmax);
// y = float(half_rne(x)): the IEEE binary16 conversion (ties to even, subnormal halves kept, |x| >= 65520 -> +-inf, NaN stays NaN)
void round_half(hipStream_t s, const float *x, float *y, int64_t n);
// y[r, i] = act(x[r, i] (op) c[i])   (const_left: c (op) x)
void binary_const(hipStream_t s, const float *x, const float *c, float *y, int64_t rows, int64_t per_row, char op,
                  bool const_left, ActParam act);
void binary_act(hipStream_t s, const float *a, const float *b, float *y, int64_t n, char op, ActParam act);
// y[r, c, i] = act(a[r, c, i] (op) gate[r, c]): per-channel gate broadcast over the S positions of a channel
void binary_gate(hipStream_t s, const float *a, const float *gate, float *y, int64_t rows, int64_t C, int64_t S, char op, ActParam act,
                 bool cq);
// y[r, c, i] = act(x * scale[c] + shift[c]);  cq: activations in channel-quad planes [N][C/4][S][4] (conv.hip)
void affine_channel(hipStream_t s, const float *x, const float *scale, const float *shift, float *y, int64_t rows,
                    int64_t C, int64_t S, ActParam act, bool cq);
// row reduction + rescale over `len` with element stride `inner`, repeated rows*outer*inner times.
// mode 0 softmax, 1 log-softmax; 2 / 3 / 4: divide by max|x| / sum|x| / sqrt(sum x^2) (ai.onnx.ml Normalizer, divisor floored at 1e-30)
void softmax(hipStream_t s, const float *x, float *y, int64_t rows, int64_t outer, int64_t len, int64_t inner, int mode);
// dst[r, dst_off : dst_off+len] = src[r, src_off : src_off+len]  (Concat piece / Slice / Split); y[r] = float(argmax_j x[r, j])
void copy_cols(hipStream_t s, const float *src, float *dst, int64_t rows, int64_t len, int64_t src_stride, int64_t src_off,
               int64_t dst_stride, int64_t dst_off);
void argmax_rows(hipStream_t s, const float *x, float *y, int64_t rows, int64_t len);
// dst[r, 0:K] = src[r, :], zeros up to Kp columns
void pad_cols(hipStream_t s, const float *src, float *dst, int64_t rows, int64_t K, int64_t Kp);
// dst[rows][ncols] = transpose of src[ncols][rows]  (column-major staging of a columnar chunk)
void transpose_cm(hipStream_t s, const float *src, float *dst, int64_t rows, int64_t ncols);
// Zero-copy column gather: up to kMaxZeroCopyCols device-visible column-run pointers (registered host memory) -> [ncols][rows] f32
// in HBM.  type: 0 f32, 1 f64, 2 i32, 3 i64 (+8 = constant vector: one element); passed by value as the kernel argument (2.3 KB).
constexpr int kMaxZeroCopyCols = 256;
struct ColumnTable {
  const void *ptr[kMaxZeroCopyCols];
  unsigned char type[kMaxZeroCopyCols];
};
void gather_columns_device(hipStream_t s, const ColumnTable &tab, int ncols, int64_t rows, float *dst);
// synthetic table fill (SURVEY.md 8d generator), row-major [rows, ncols]
void synth_fill(hipStream_t s, float *dst, uint64_t seed, uint64_t row0, uint64_t rows, uint64_t ncols);

// ---- tree ensembles (trees.hip) ---------------------------------------------------------------
// part[S][rows][W] = per-slice sums of the leaves the rows of x [rows, F] reach; tab = host/trees.hpp TreePack::tab (records, roots, slices)
void tree_walk(hipStream_t s, const float *x, int F, const uint32_t *tab, int64_t n_nodes, int64_t n_trees, const float *leaves, int W, int S,
               float *part, int64_t rows);
// the slices summed in slice order (/ n_trees under AVERAGE, + base) -> scores [rows, W], or a host/plan.hpp TreeOut form
void tree_reduce(hipStream_t s, const float *part, const float *base, const float *labels, float *y, int64_t rows, int W, int S, int64_t n_trees,
                 bool average, int mode, bool is_signed);

// ---- support-vector machines (svm.hip) ---------------------------------------------------------
// part[S][rows][Q] = per-slice sums  sum_s coef[q][s] * K(x, s)  for x [rows, F]; tables: host/svm.hpp SvmPack (kernel: SvmKernelType).
// false: the kernel could not be given its LDS (F > 504 opts in to more than 64 KB) and nothing was launched
bool svm_kernel(hipStream_t s, const float *x, int F, int F_pad, int kernel, const float *center, const float *sv, const float *sv_norm, const float *coef,
                const uint32_t *slice_tile, float *part, int64_t rows, int S, int Q, int QW, float gamma, float coef0, int degree);
// the slices of each class summed in slice order, + rho -> a host/plan.hpp SvmOut form
void svm_reduce(hipStream_t s, const float *part, const uint32_t *class_slice, const float *rho, const float *labels, const float *prob_a,
                const float *prob_b, float *y, int64_t rows, int Q, int C, int mode);

// ---- distance models (nearest.hip) -------------------------------------------------------------
// x [rows, F] against the packed set of host/nearest.hpp NearestPack.  mode (NearestOut) kNearestMatrix / kNearestMatrixSqrt: out = d2 /
// sqrt(d2) [rows, M]; kNearestSelect: out = the per-slice best lists [rows][S][2 * nearest_list_width(k)] (host/nearest.hpp) (values, then index patterns)
// false: the kernel could not be given its LDS (F > 504 needs the opt-in beyond 64 KB)
bool nearest(hipStream_t s, const float *x, int F, int F_pad, const float *center, const float *ref, const float *ref_norm, const uint32_t *slice_tile,
             float *out, int64_t rows, int S, int M, int k, int mode);
// the slices merged in slice order -> the label [rows], the k nearest indices or their (sqrt) distances [rows, k]
void nearest_reduce(hipStream_t s, const float *part, float *y, int64_t rows, int S, int k, int mode);
// the k-NN vote over the same lists (host/nearest.hpp VotePack, VoteOut): cls [M] class indices in 0 .. C - 1 / target [M] (the one the
// mode reads), class_value [C]; y = the label [rows], the probabilities [rows, C] or the value [rows, 1].  w = 1 (uniform) or
// 1 / max(d, eps), d = d2 or sqrt(d2) (rooted).  false: the form is outside the kernel (C above kVoteMaxProbaClasses, k outside 1 .. min(16, M))
bool nearest_vote(hipStream_t s, const float *part, const int *cls, const float *target, const float *class_value, float *y, int64_t rows, int S, int M, int k,
                  int C, int mode, bool weighted, bool rooted, float eps);

// ---- reductions along the feature axis (reduce.hip) ----------------------------------------------
// y[v] = reduction op (host/plan.hpp ReduceOp) over the E elements of each of nvec vectors
void row_reduce(hipStream_t s, const float *x, float *y, int64_t nvec, int E, int op);
void argmin_rows(hipStream_t s, const float *x, float *y, int64_t rows, int64_t len);
// y [rows, k] = the k smallest / largest of x [rows, M], sorted (equal values by lower index, NaN last): the values, or the indices as f32
void topk_rows(hipStream_t s, const float *x, float *y, int64_t rows, int M, int k, bool largest, bool indices);
// y[v, i] = act(a[v, i] (op) b[v])   (scalar_left: b[v] (op) a[v, i]) over nvec vectors of E elements
void binary_rowscalar(hipStream_t s, const float *a, const float *b, float *y, int64_t nvec, int64_t E, char op, bool scalar_left, ActParam act);

// ---- preprocessing regions (prep.hip) -----------------------------------------------------------
// y[r, j] = column program j (host/prep.hpp PrepPack: desc, cst, tab of ntab pairs) over x[r, 0:F_in], R rows per block tile; err: the call's failure
// word (plans with a zeros = 0 OneHotEncoder only, else null), set to the encoder's 1-based id on a value outside its categories
void prep(hipStream_t s, const float *x, int F_in, const uint32_t *desc, const float *cst, const float *tab, int ntab, float *y, int F, int64_t rows,
          int R, int *err);

// ---- recurrent layers (rnn.hip) -------------------------------------------------------------------
// LSTM / GRU / RNN over x [rows, T, F] (x_colmajor: ONE column-major chunk [T * F][rows]); tables: host/recurrent.hpp RnnPack (op: RnnOp).
// mode (RnnOut): y = Y [rows, T, D, H], or the last state Y_h / Y_c [rows, D, H].  false: the kernel could not be given its LDS
// lens (null: every row holds T steps): row r holds lens[r * lens_ld + lens_off] valid steps (lens_int: truncated toward zero first) and
// gives what the layer gives on those steps alone: Y is 0 behind them, the states are those after the last of them, what lies behind
// them in x is not read.  A length outside 0 .. T (a NaN included) counts as 0 and sets the call's failure word *err to err_node.
// Never with x_colmajor (false)
bool rnn(hipStream_t s, const float *x, const float *wr, const float *bias, const float *bias2, const float *h0, const float *c0, float *y, int64_t rows,
         int op, int T, int F, int H, int D, bool reverse, bool lbr, bool relu, int mode, bool x_colmajor, const float *lens = nullptr, int64_t lens_ld = 0,
         int lens_off = 0, bool lens_int = false, int *err = nullptr, int err_node = 0);

// ---- Transformer encoders (attention.hip, layernorm.hip) -------------------------------------------------------------------------
// y [rows, T, heads * dh] = softmax(scale . Q K^T + mask) V per row and head; q / k / v: [rows, T, ld[i]] with head g at columns
// off[i] + g * dh of a step (the same pointer three times for a packed projection); mask: [T, T] or null, -inf = no weight.
// rm: null, or the buffer that holds the rows' own key masks ([rows, rm_ld]; no constant mask beside it): key j of a row is kept iff
// rm[row, rm_off + j] (rm_int: truncated toward zero) != rm_cmp; a masked key is excluded like a key beyond T (rm_excl, in rows that keep a
// key) or scored sc + rm_fill / rm_fill (rm_mode: RowMaskMode).
// The operator form: Tk > 0: k / v are [rows, Tk, ld] and mask [T, Tk] (0: Tk = T); kv_heads > 0: query head g reads K / V head
// g / (heads / kv_heads) (0: kv_heads = heads); causal: key j counts for query i iff j <= i, beside either mask.
// false: a size is beyond the caps of host/attention.hpp (the lowering refuses those at load)
bool attention(hipStream_t s, const float *q, const float *k, const float *v, const float *mask, float *y, int64_t rows, int T, int heads, int dh,
               const int64_t ld[3], const int64_t off[3], float scale, const float *rm = nullptr, int64_t rm_ld = 0, int rm_off = 0, float rm_cmp = 0.f,
               float rm_fill = 0.f, int rm_mode = 0, bool rm_excl = false, bool rm_int = false, int Tk = 0, int kv_heads = 0, bool causal = false);
// y = x / sqrtf(mean(x^2) + eps) * gamma over each of nvec vectors of E elements (RMSNormalization); false: E beyond the cap
bool rmsnorm(hipStream_t s, const float *x, const float *gamma, float *y, int64_t nvec, int E, float eps);
// Rotary position embedding (rotary.hip): y [rows, T, heads * dh] dense; x: [rows, T, ld] with head g at columns off + g * dh of a step.
// Column j < rd of a head: y[j] = fl(fl(x[j] * A[t, j]) + fl(x[partner(j)] * B[t, j])), partner(j) = j +- rd / 2, or j ^ 1 (interleaved);
// columns j >= rd are bit copies.  A, B: [T, rd].  false: a size is beyond the caps of host/attention.hpp, rd is odd or the view leaves ld
bool rotary(hipStream_t s, const float *x, int64_t ld, int64_t off, const float *A, const float *B, float *y, int64_t rows, int T, int heads, int dh, int rd,
            bool interleaved);
// y = (x - mean) / sqrt(var + eps) * gamma + beta over each of nvec vectors of E elements (beta may be null); false: E beyond the cap
bool layernorm(hipStream_t s, const float *x, const float *gamma, const float *beta, float *y, int64_t nvec, int E, float eps);
// y[r, e] = mean over t of x[r, t, e]
void mean_time(hipStream_t s, const float *x, float *y, int64_t rows, int T, int E);
// y[r, e] = (sum in order over the kept t of x[r, t, e]) / max(float(kept steps of row r), clip); step t is kept iff rm[r, rm_off + t]
// (rm_int: truncated toward zero) != rm_cmp; a masked step is not read
void mean_time_masked(hipStream_t s, const float *x, float *y, int64_t rows, int T, int E, const float *rm, int64_t rm_ld, int rm_off, float rm_cmp,
                      bool rm_int, float clip);

// ---- dense layer, fp32 MFMA (dense.hip) -------------------------------------------------------
// Y[rows, M] = act(X[rows, K] . W[K, M] + bias[M]); W row-major, bias may be null.
// softmax_fused: apply a row softmax over the M outputs in the epilogue (requires M <= 256).
// x_colmajor: X is ONE column-major chunk [K][rows] (host path staging; only where dense_colmajor_supported(K, M)).
// kernel family that serves a Dense layer (the launcher's own decision function; "" = none carries that epilogue)
const char *dense_kernel_family(int64_t rows, int K, int M, int softmax_mode, bool x_colmajor, bool aligned16);
void dense(hipStream_t s, const float *X, const float *W, const float *bias, float *Y, int64_t rows, int K, int M,
           ActParam act, int softmax_mode /*0 none,1 softmax,2 log-softmax,3 argmax (label only)*/, bool x_colmajor = false);
bool dense_colmajor_supported(int K, int M);
// where a streaming kernel carries the softmax epilogue (wider heads: tiled Dense + the row softmax kernel is faster)
bool dense_can_fuse_softmax(int K, int M);
// softmax_mode 3: Y[rows] = float(index of the first maximum of the M scores) -- only where this returns true
bool dense_can_fuse_argmax(const float *X, int K, int M);

// ---- quantised dense layer, int8 MFMA (qdense.hip) --------------------------------------------
// One QDense step (host/plan.hpp) over `rows` rows.  X: f32 [rows, K], or (in_bytes) the signed bytes xq - x_shift; Y: f32 [rows, M], or
// (out_bytes, y_on only) the signed bytes q - y_shift.  Wp = qdense_pack() of the shifted weights; mult / c0 / wz / bias hold
// qdense_padded_m(M) entries: mult[m] = x_scale * w_scale[m]; c0[m] = every row-independent integer term (qdense.hip; the int32 bias
// included); wz[m] = the shifted weight zero points, null when all are 0; bias = the f32 bias or null.
struct QDenseLaunch {
  const void *X = nullptr;
  void *Y = nullptr;
  const float *Wp = nullptr, *mult = nullptr, *bias = nullptr;
  const int *c0 = nullptr, *wz = nullptr;
  int64_t rows = 0;
  int K = 0, M = 0;
  float x_scale = 1.f;
  int x_zp = 0, x_min = 0, x_max = 255, x_shift = 128;
  int y_on = 0;
  float y_scale = 1.f;
  int y_zp = 0, y_min = 0, y_max = 255, y_shift = 128;
  int act = 0;  // plan.hpp Act: None, Relu or Clip(a, b)
  float act_a = 0.f, act_b = 0.f;
  bool in_bytes = false, out_bytes = false;
  int KT = 0, MTp = 0;  // (set by the launcher)
  bool x_vec = false;
};
int qdense_padded_m(int M);
size_t qdense_packed_floats(int K, int M);
void qdense_pack(int K, int M, const int8_t *W, float *packed);  // W: [K, M] signed bytes
void qdense(hipStream_t s, QDenseLaunch p);

// ---- quantised convolution, int8 MFMA (qconv.hip) -----------------------------------------------
// One QConv2d step (host/plan.hpp) over `rows` images.  X: f32 [rows, C, H, W], or (in_cq) channel-quad planes [rows, C/4, H*W, 4]; Y
// likewise ([rows, M, OH, OW] / out_cq).  Wfrag = qconv_pack() of the shifted weights; mult / c0 / wz / bias as for QDenseLaunch, with
// qconv_padded_m(M) entries and K = C * kh * kw.
struct QConvLaunch {
  const float *X = nullptr;
  float *Y = nullptr;
  const float *Wfrag = nullptr, *mult = nullptr, *bias = nullptr;
  const int *c0 = nullptr, *wz = nullptr;
  int64_t rows = 0;
  int C = 0, H = 0, W = 0, M = 0, OH = 0, OW = 0, kh = 1, kw = 1, sh = 1, sw = 1, pt = 0, pl = 0, dh = 1, dw = 1;
  bool in_cq = false, out_cq = false;
  float x_scale = 1.f;
  int x_zp = 0, x_min = 0, x_max = 255, x_shift = 128;
  int y_on = 0;
  float y_scale = 1.f;
  int y_zp = 0, y_min = 0, y_max = 255;
  int act = 0;  // plan.hpp Act: None, Relu or Clip(a, b)
  float act_a = 0.f, act_b = 0.f;
  bool force_direct = false;  // quantise per tap from global memory even where the staged window fits (A/B, tests)
  int CT = 0, TG = 0, MTp = 0, Hpad = 0, Wpad = 0, lds_entries = 0;  // (set by the launcher)
};
int qconv_padded_m(int M);
size_t qconv_packed_floats(int C, int taps, int M);
void qconv_pack(int C, int taps, int M, const int8_t *W, float *packed);  // W: [K, M] signed bytes, k = (c, tap)
bool qconv_stages_in_lds(QConvLaunch p);  // does the launch stage its quantised input window in LDS (else: per tap from global memory)
void qconv(hipStream_t s, QConvLaunch p);

// ---- float16 dense layer, f16 MFMA (hdense.hip) -----------------------------------------------
// One HDense step (host/plan.hpp) over `rows` rows.  X: f32 [rows, K] (rounded to half on load), or (in_half) halves; Y: f32 [rows, M]
// holding half values, or (out_half) the halves themselves.  Wp = hdense_pack() of the weights' bit patterns; bias = the half bias widened
// to f32, hdense_padded_m(M) entries (bias_mode = plan.hpp HalfBias: 0 none, 1 Gemm, 2 MatMul -> Add).
struct HDenseLaunch {
  const void *X = nullptr;
  void *Y = nullptr;
  const float *Wp = nullptr, *bias = nullptr;
  int64_t rows = 0;
  int K = 0, M = 0;
  int bias_mode = 0;
  int act = 0;  // plan.hpp Act: None, Relu, Sigmoid, Tanh, LeakyRelu(a) or Clip(a, b)
  float act_a = 0.f, act_b = 0.f;
  bool in_half = false, out_half = false;
  int KT = 0, MTp = 0;  // (set by the launcher)
  bool x_vec = false, y_vec = false;
};
int hdense_padded_m(int M);
size_t hdense_packed_floats(int K, int M);
void hdense_pack(int K, int M, const uint16_t *W, float *packed);  // W: [K, M] half bit patterns
void hdense(hipStream_t s, HDenseLaunch p);

// ---- whole-chain fused MLP (mlp_fused.hip) -----------------------------------------------------
// A chain D0 -> D1 -> D2 -> D3 evaluated in one persistent kernel; activations never leave
// registers.  `packed` holds the fragment-major weights produced by mlp3_pack().
struct Mlp3Shape {
  int d0, d1, d2, d3;
  int act1, act2, act3;  // only None/Relu chains are instantiated ahead of time
};
// True if a fused kernel exists for the chain: an ahead-of-time instantiation, or one compiled right now
// by hipRTC from the same device source (needs a visible GPU).  On false, `why` explains and the caller
// keeps the layer-by-layer plan.
bool mlp3_supported(const Mlp3Shape &sh, std::string *why = nullptr);
// Size in floats of the packed weight blob and host-side packing (fragment-major order, see mlp_fused.hip).
size_t mlp3_packed_floats(const Mlp3Shape &sh);
void mlp3_pack(const Mlp3Shape &sh, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
               const float *b3, float *packed);
// x_colmajor: X is a column-major chunk [d0][rows] (the host path's staging of flat DuckDB columns); only for the chains
// mlp3_colmajor_supported() names.
// queue: kMlp3QueueWords zeroed unsigneds in device memory that belong to the launches of stream `s` alone (never to two kernels
// that may run at once): the tile queue of mlp3_split_kernel, which leaves them zero again at the end of every launch.
constexpr size_t kMlp3QueueWords = 2;  // head, done
bool mlp3(hipStream_t s, const Mlp3Shape &sh, const float *X, const float *packed, float *Y, int64_t rows, int num_cus,
          unsigned *queue, std::string *why = nullptr, bool x_colmajor = false);
bool mlp3_colmajor_supported(const Mlp3Shape &sh);
int64_t mlp3_colmajor_max_rows(const Mlp3Shape &sh);  // longest column-major chunk the chain's kernels read themselves (0: none)
std::string mlp3_kernel_name(const Mlp3Shape &sh);

// ---- fused chain of small Dense layers over tables of any width (chain_device.inc, specialised with hipRTC) ----
// k0 table columns; layer l maps dims[l-1] (dims[-1] = k0) -> dims[l] and applies acts[l] (plan.hpp Act 0..5) with
// parameters pa/pb; sm: 0 plain, 1 softmax, 2 log-softmax, 3 argmax (label only) over the last layer's <= 16 outputs.
struct ChainShape {
  int k0 = 0;
  std::vector<int> dims, acts;
  std::vector<float> pa, pb;
  int sm = 0;
};
// True once a kernel for the shape is compiled (first call compiles); `why` otherwise: limits, hipRTC missing, ...
bool chain_supported(const ChainShape &s, std::string *why = nullptr);
size_t chain_packed_floats(const ChainShape &s);
// W[l] is [K_l, M_l] row-major, bias[l] has M_l floats or is null
void chain_pack(const ChainShape &s, const std::vector<const float *> &W, const std::vector<const float *> &bias, float *out);
// x_colmajor: X is one column-major chunk [k0][rows] (the host path's staging layout) instead of the row-major table
bool chain(hipStream_t st, const ChainShape &s, const float *X, const float *packed, float *Y, int64_t rows, int num_cus,
           std::string *why, bool x_colmajor = false);
std::string chain_kernel_name(const ChainShape &s);

// ---- convolution / pooling (conv.hip) ----------------------------------------------------------
struct ConvGeom {
  int C, H, W, M, OH, OW, kh, kw, sh, sw, pt, pl, dh, dw, groups;
  // Dense layers on the tiled kernel (H = W = 1): C and M are the PADDED sizes (multiples of 32, zero weights / bias
  // beyond the real ones); the real row lengths of the input and output matrices.  0 = not a dense layer.
  int kvalid = 0, mvalid = 0;
  // Convolutions whose channel counts are whole quads but no multiples of 32 (MobileNet's 16 / 24 / 144, ...): C and M
  // are the PADDED sizes as above, kvalid / mvalid the real ones (the tensors' plane counts are kvalid/4 and mvalid/4).
  int padc = 0;
};
// the geometry the tiled kernel runs for a convolution step: channels padded to 32 when they are not (padc = 1)
ConvGeom conv2d_tiled_geom(const ConvGeom &real);
// the same for the stem's patch kernel: M padded to whole 32-feature tiles (mvalid = the real count) for stems with 16 / 24 outputs
ConvGeom conv2d_patch_geom(const ConvGeom &real);
// Generic implicit-GEMM convolution: any geometry / groups; Wk = conv2d_generic_pack() of the ONNX
// weights ([group][k][M/g], k = (c, ky, kx)); activations NCHW or channel-quad planes (CQ) per flag.
bool conv2d_generic_supported(const ConvGeom &g);  // (C/g)*kh*kw <= 8192 (the per-k offset table lives in LDS)
void conv2d_generic_pack(const ConvGeom &g, const float *Wt, float *packed);
void conv2d(hipStream_t s, const float *X, const float *Wk, const float *bias, float *Y, int64_t rows, const ConvGeom &g,
            ActParam act, bool in_cq, bool out_cq);
// Patch convolution for the network's first layer: few input channels (C <= 8), NCHW input, CQ output,
// M in {32, 64, 96, 128}, groups == 1; the receptive field of a pixel tile is staged in LDS.
bool conv2d_patch_supported(const ConvGeom &g);
size_t conv2d_patch_packed_floats(const ConvGeom &g);
// ... with the MaxPool 3x3 / stride 2 that follows it in the same kernel (ResNet / DenseNet / SqueezeNet stems): the convolution's
// own output never reaches memory.  pool = pooled extent and the pooling's pads (0 or 1).  Pack with the same PoolTail.
struct PoolTail {
  int OH = 0, OW = 0, pt = 0, pl = 0;
};
bool conv2d_patch_pool_supported(const ConvGeom &g, const PoolTail &pool);
// ... and in the default arithmetic (bf16 x three exact parts, six MFMAs per product: no scales, nothing to track)
bool conv2d_stem_split6_supported(const ConvGeom &g, const PoolTail &pool);
size_t conv2d_stem_split6_packed_floats();
void conv2d_stem_split6_pack(const ConvGeom &g, const float *Wt, float *packed);
void conv2d_stem_split6(hipStream_t s, const float *X, const float *packed, const float *bias, float *Y, int64_t rows, const ConvGeom &g,
                        ActParam act, const PoolTail &pool, int num_cus);
void conv2d_patch_pool(hipStream_t s, const float *X, const float *packed, const float *bias, float *Y, int64_t rows,
                       const ConvGeom &g, ActParam act, const PoolTail &pool, int num_cus);
void conv2d_patch_pack(const ConvGeom &g, const float *Wt, float *packed, const PoolTail *pool = nullptr);
void conv2d_patch(hipStream_t s, const float *X, const float *packed, const float *bias, float *Y, int64_t rows,
                  const ConvGeom &g, ActParam act, int num_cus);
// Depthwise convolution (groups == C == M, C % 4 == 0) in channel-quad planes; packed = [C/4][tap][4].
bool conv2d_depthwise_supported(const ConvGeom &g);
void conv2d_depthwise_pack(const ConvGeom &g, const float *Wt, float *packed);
void conv2d_depthwise(hipStream_t s, const float *X, const float *packed, const float *bias, float *Y, int64_t rows,
                      const ConvGeom &g, ActParam act);
// Tiled CQ-layout convolution (groups == 1, C % 32 == 0, M % 32 == 0) on fragment-major packed weights.
bool conv2d_tiled_supported(const ConvGeom &g);
size_t conv2d_tiled_packed_floats(const ConvGeom &g);
void conv2d_tiled_pack(const ConvGeom &g, const float *Wt, float *packed);
// residual (nullable): CQ tensor of the output's shape added before the activation (fused ResNet Add)
void conv2d_tiled(hipStream_t s, const float *X, const float *packed, const float *bias, const float *residual, float *Y,
                  int64_t rows, const ConvGeom &g, ActParam act);
// The same convolution on the bf16 matrix cores with every fp32 operand cut exactly into three bf16 parts, six partial products per product (the default;
// conv_split.hip): no scales, no maxima,
// no precondition on the data.  M % 64 == 0; packed = conv2d_split6_packed_floats(g) floats' worth of bf16 hi / mid / lo fragments.
bool conv2d_split6_supported(const ConvGeom &g);
size_t conv2d_split6_packed_floats(const ConvGeom &g);
void conv2d_split6_pack(const ConvGeom &g, const float *Wt, float *packed);
// Second input of a split convolution (a ResNet block's projection shortcut folded into the block's second convolution): a channel-quad tensor of C
// channels on an H x W grid, read at (oh * sh, ow * sw) through a 1x1 filter whose C / 32 weight chunks (conv2d_split6_pack of the 1x1 layer) follow
// the main filter's in `packed`; X == nullptr: none.  Only where conv2d_split6_takes_second_input(g).
struct SecondInput {
  const float *X = nullptr;
  int C = 0, H = 0, W = 0, sh = 1, sw = 1;
};
bool conv2d_split6_takes_second_input(const ConvGeom &g);
void conv2d_split6(hipStream_t s, const float *X, const float *packed, const float *bias, const float *residual, float *Y, int64_t rows,
                   const ConvGeom &g, ActParam act, const SecondInput &x2 = SecondInput());
void pool2d(hipStream_t s, const float *X, float *Y, int64_t rows, int C, int H, int W, int OH, int OW, int kh, int kw,
            int sh, int sw, int pt, int pl, int dh, int dw, bool is_max, bool count_pad, bool cq);
// y[n,c,p] = x[n,c,p] / (bias + alpha/size * sum_{c' in window(c)} x[n,c',p]^2)^beta over [rows, C, S] (cq: channel-quad planes)
void lrn(hipStream_t s, const float *X, float *Y, int64_t rows, int C, int S, int size, float alpha, float beta, float bias, bool cq);
// Y[n, j*g + i, p] = X[n, i*(C/g) + j, p]
void channel_shuffle(hipStream_t s, const float *X, float *Y, int64_t rows, int C, int S, int groups, bool cq);
void global_avgpool(hipStream_t s, const float *X, float *Y, int64_t rows, int C, int S, bool cq, bool is_max = false);

// ---- transposed convolution by stride phases (deconv.hip) and Resize (resize.hip) --------------
// C, H, W = the input; M, OH, OW = the output; h_stride / w_stride = ints per row- / column-phase record of `tab` (host/deconv.hpp)
struct ConvTGeom {
  int C, H, W, M, OH, OW, kh, kw, sh, sw, pt, pl, groups, h_stride, w_stride;
};
// Generic kernel: any groups / dilation / layouts; Wg = convt2d_generic_pack() of the ONNX weights [C, M/g, kh, kw] -> [ky][kx][C][M/g]
void convt2d_generic_pack(const ConvTGeom &g, const float *W, float *packed);
void convt2d_generic(hipStream_t s, const float *X, const float *Wg, const float *bias, float *Y, const int *tab, int64_t rows, const ConvTGeom &g,
                     ActParam act, bool in_cq, bool out_cq);
// MFMA phase kernel: groups == 1, channel-quad input (C % 4 == 0), output channel-quad or NCHW per flag.  `tab` on the device = the axis
// tables followed by the sh * sw phase offsets convt2d_phase_pack() fills (units of 256 floats into the packed weights)
bool convt2d_phase_supported(const ConvTGeom &g, const int32_t *tab);
size_t convt2d_phase_packed_floats(const ConvTGeom &g, const int32_t *tab);
void convt2d_phase_pack(const ConvTGeom &g, const int32_t *tab, const float *W, float *packed, int32_t *phase_off);
void convt2d_phase(hipStream_t s, const float *X, const float *Wp, const float *bias, float *Y, const int *tab, int64_t rows, const ConvTGeom &g,
                   int64_t max_phase_pixels, ActParam act, bool out_cq);
// Y[n, c, oh, ow] from the row / column tables: nearest: X[n, c, row_idx[oh], col_idx[ow]]; linear: horizontal interpolation of the rows
// row_idx[2 oh], row_idx[2 oh + 1] with (col_wgt[2 ow], col_wgt[2 ow + 1]) = (1 - w, w), then the vertical one with row_wgt
void resize2d(hipStream_t s, const float *X, float *Y, int64_t rows, int C, int H, int W, int OH, int OW, const int *row_idx, const int *col_idx,
              const float *row_wgt, const float *col_wgt, bool linear, bool cq);

// ---- DepthToSpace / SpaceToDepth (pixelshuffle.hip; the four forms: host/pixelshuffle.hpp) ------
// C, H, W = the input; OC, OH, OW = the output; b = the block size
struct PixelShuffleGeom {
  int b, C, H, W, OC, OH, OW;
  bool to_space, channel_major;
};
// `kernel`: the PixelShuffleKernel the scheduler chose for these layouts; false: it does not serve them (nothing was launched)
bool pixel_shuffle(hipStream_t s, const float *X, float *Y, int64_t rows, const PixelShuffleGeom &g, int kernel, bool in_cq, bool out_cq);

// ---- InstanceNormalization / GroupNormalization (spatialnorm.hip; host/spatialnorm.hpp) --------------
// X, Y: [rows, C, S] in NCHW order or (cq) channel-quad planes; G groups of C / G channels; gamma, beta: [C].  false: beyond the kernel's caps
// fused: where spatialnorm_fused_unit(C, S, G, cq) names a unit -- one pass, y = act(d / sqrtf(var + eps) * gamma + beta)
bool spatialnorm_fused(hipStream_t s, const float *X, const float *gamma, const float *beta, float *Y, int64_t rows, int C, int S, int G, bool cq, float eps,
                       ActParam act);
// general: stats [rows, G, 3] = (mean, resid, 1 / sqrtf(var + eps)), then y = act(((x - mean) - resid) * inv * gamma + beta)
bool spatialnorm_stats(hipStream_t s, const float *X, float *stats, int64_t rows, int C, int S, int G, bool cq, float eps);
bool spatialnorm_apply(hipStream_t s, const float *X, const float *stats, const float *gamma, const float *beta, float *Y, int64_t rows, int C, int S, int G,
                       bool cq, ActParam act);

// ---- Tokens: [rows, C, S] of a convolutional step -> the window [rows, P + S, C] (tokens.hip; host/tokens.hpp) --------------
// X: NCHW order or (cq) channel-quad planes; prefix [P, C] (P = 0: none), pos [P + S, C] or null: added in the store.  false: beyond the caps
bool tokens(hipStream_t s, const float *X, const float *prefix, const float *pos, float *Y, int64_t rows, int C, int S, int P, bool cq);

// ---- Embed: table lookups by runtime indices, column copies and their Concat as one pass (embed.hip; host/embed.hpp) --------------
// x [rows, W] row-major; desc: kEmbedDescInts per piece (P pieces); map: the piece of every output column (map_entries 16-bit entries, a
// multiple of 8) or null: a search; tab: the tables; y [rows, F]; R rows per work group; staged: the source tile goes through LDS; err: the
// call's failure word, set to a piece's node id on an index outside its table (that load goes to row 0); nt: non-temporal stores for the full
// quads.  false: beyond the caps
bool embed(hipStream_t s, const float *x, int W, const int32_t *desc, int P, const uint16_t *map, int map_entries, const float *tab, float *y, int64_t F,
           int64_t rows, int R, bool staged, int *err, bool nt = false);

// ---- Interact: DLRM's pairwise dot products and the FM bi-interaction term of a window T [rows, k, d] (interact.hip; host/interact.hpp) ----
// dot: out [rows, F]; map [F]: per output column >= 0 the entry i * tile + j of Z = T . T^T, < 0: -(column of T's flat row) - 1, a bit copy;
// tile: 16, 32 or 64 >= k.  fm: out [rows, d] = h * ((sum_f T)^2 - sum_f T^2) (has_h = false: no multiply), sum_last: [rows, 1], its sum
// over the d columns (h_after: multiplied by h after the sum, not before).  false: beyond the caps
bool interact_dot(hipStream_t s, const float *T, int k, int d, int tile, const int32_t *map, int64_t F, float *out, int64_t rows);
bool interact_fm(hipStream_t s, const float *T, int k, int d, float h, bool has_h, bool h_after, bool sum_last, float *out, int64_t rows);

// ---- LayerNorm over the channel axis at each pixel (channelnorm.hip; host/channelnorm.hpp) --------------
// X, Y: [rows, C, S] in NCHW order or (cq) channel-quad planes, the same layout; gamma [C], beta [C] or null.  regs: the register form
// (C <= kChannelNormRegsMaxC), else the re-read form.  y = act(d / sqrtf(var + eps) * gamma + beta).  false: beyond the kernel's caps
bool channelnorm(hipStream_t s, const float *X, const float *gamma, const float *beta, float *Y, int64_t rows, int C, int S, bool cq, bool regs, float eps,
                 ActParam act);

}  // namespace infera_hip::kern
