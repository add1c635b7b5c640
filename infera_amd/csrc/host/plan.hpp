// plan.hpp -- the lowered, device-independent execution plan of one model.
//
// infera_load_model turns the ONNX graph into this at load time (the reference does the analogous
// work with Tract's into_optimized()/into_runnable(), engine.rs:52-55).  Every activation is a
// row-major [rows, per_row] f32 matrix whose leading axis is the table-row (batch) axis, so all
// steps are row-independent and a scan shards by row range with no exchange.
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "onnx_model.hpp"

namespace infera_hip {

struct TreePack;  // host/trees.hpp
struct SvmPack;   // host/svm.hpp
struct PrepPack;  // host/prep.hpp
struct RnnPack;   // host/recurrent.hpp
struct NearestPack;  // host/nearest.hpp
struct VotePack;     // host/nearest.hpp
struct DeconvPack;   // host/deconv.hpp
struct EmbedPack;    // host/embed.hpp
struct InteractPack;  // host/interact.hpp

// Kinds 1..5 may be fused into the epilogue of a Dense / Conv2d step (the MFMA kernels resolve them at
// compile time); the rest run in the elementwise kernels (fused into Binary*/AffineChannel or as a Unary step).
enum class Act : int {
  None = 0, Relu = 1, Sigmoid = 2, Tanh = 3, LeakyRelu = 4, Clip = 5,
  Exp = 6, Log = 7, Sqrt = 8, Neg = 9, Abs = 10, Elu = 11, Selu = 12, Softplus = 13, HardSigmoid = 14, HardSwish = 15,
  Erf = 16, Gelu = 17, Reciprocal = 18, Floor = 19, Ceil = 20, Softsign = 21, Trunc = 22, Round = 23,
  Swish = 24,  // x * sigmoid(x): recognised from Mul(x, Sigmoid(x)) (EfficientNet / YOLO exports)
};
constexpr int kMaxMfmaFusedAct = 5;  // the load-time specialised chain kernels resolve kinds 0..5
// what the ahead-of-time MFMA epilogues resolve (device_common.hpp dispatch_act): the above + the mobile-net gates
inline bool mfma_fusable(Act a) { return int(a) <= kMaxMfmaFusedAct || a == Act::HardSigmoid || a == Act::HardSwish || a == Act::Swish; }

enum class StepKind : int {
  Dense = 0,        // Y[rows,M] = act(X[rows,K] . W[K,M] + bias[M])       (MatMul / Gemm [+Add] [+act])
  Unary = 1,        // elementwise activation
  AffineChannel = 2,// y = x*scale[c] + shift[c]  per channel              (unfused BatchNormalization)
  BinaryConst = 3,  // y = x (op) cst[per_row]  (constant pre-broadcast to one row)
  BinaryAct = 4,    // y = a (op) b             (residual adds; S > 1: b is a per-channel gate [rows, C] broadcast over S positions; K > 0: b is one scalar per vector of K elements, [N, K] (op) [N, 1], const_left: the scalar is the left operand)
  Softmax = 5,      // softmax / log-softmax over `sm_len` with (outer, len, inner) strides inside a row
  Conv2d = 6,       // NCHW convolution as implicit GEMM (BatchNormalization folded when adjacent)
  Pool2d = 7,       // MaxPool / AveragePool
  GlobalAvgPool = 8,
  CopyCols = 9,     // out[r, col_off : col_off+len] = in0[r, :]   (one piece of a Concat along the feature/channel axis)
  ArgMax = 10,      // out[r, 0] = float(index of the first maximum of in0[r, 0:len])   (labels as f32 values)
  SliceCols = 11,   // out[r, :] = in0[r, col_off : col_off+K]   (Slice / Split on the feature axis; one input of a multi-input model)
  LRN = 13,         // across-channel local response normalisation: y = x / (act_b' ... see lrn_* fields) over [N,C,S]
  ChannelShuffle = 14,  // out[n, j*g + i, p] = in0[n, i*(C/g) + j, p]   (Reshape [N,g,C/g,..] -> Transpose(0,2,1,..) -> Reshape; groups in `groups`)
  PadCols = 12,     // out[r, 0:K] = in0[r, :], zeros up to M columns   (row length -> multiple of 4 for the 16-byte loads of the MFMA kernels)
  TreeEnsemble = 15,  // ai.onnx.ml tree walk: out = per-slice partial sums, f64 as f32 pairs: [rows][2 * slices * W] of the TreePack (slice-major inside the pass, trees.hip)
  TreeReduce = 16,    // in0 = those partials -> scores [rows, E] (AVERAGE, base_values, binary expansion) or the class label [rows]
  SvmKernel = 17,     // ai.onnx.ml SVM: out = per-slice sums  sum_s coef[q][s] * K(x, s)  over each SV slice: [slices][rows][Q] (SvmPack, svm.hip)
  SvmReduce = 18,     // in0 = those partials -> regressor value / one-class sign, pairwise decisions, label or probabilities (SvmOut)
  Prep = 19,          // ai.onnx.ml preprocessing region: out[r, j] = column program j over in0[r, :] (host/prep.hpp, prep.hip)
  Recurrent = 20,     // ONNX LSTM / GRU / RNN over in0 [rows, T, F]: out = Y [rows, T, D, H] or the last state [rows, D, H] (RnnOut; RnnPack, rnn.hip)
  LayerNorm = 21,     // y = (x - mean) / sqrt(var + eps) * scale[K] + shift[K] over each of the `rep` vectors of K elements of a row (layernorm.hip)
  Attention = 22,     // attention over the T steps of a row: out [rows, T, heads * dh] = softmax(attn_scale . Q K^T + mask) V per head; the Attention operator adds attn_Tk, attn_kv_heads, attn_causal (attention.hip)
  MeanTime = 23,      // out[r, e] = mean over t of in0[r, t, e]   (ReduceMean over the time axis of [rows, T = rep, K])
  FakeQuant = 24,     // y = (sat(rne(x / s) + zp) - zp) * s   (QuantizeLinear -> DequantizeLinear on an activation; Step::qx)
  QDense = 25,        // quantised MatMul / Gemm on the int8 matrix cores, f32 in and out (Step::qx, qy, qW ...; qdense.hip)
  QConv2d = 26,       // quantised convolution (groups == 1): the QDense definition per output pixel, padding = real 0; the Conv2d geometry fields + the QDense quantisation fields (qconv.hip)
  RoundHalf = 27,     // y = float(half_rne(x)): an f32 value rounded once to IEEE binary16 (the float path of a float16 graph)
  RowReduce = 29,     // out[r, v] = reduction `out_mode` (ReduceOp) over the K elements of vector v of in0 [rows, rep, K]   (the ONNX Reduce* family over the last axis; reduce.hip)
  ArgMin = 30,        // out[r, 0] = float(index of the first minimum of in0[r, 0:K])
  TopK = 31,          // the M (<= 16) smallest / largest (is_max) of in0[r, 0:K], sorted, equal values by lower index, NaN last: out [rows, M] = the values (out_mode 0) or the indices as f32 values (1)
  Nearest = 32,       // distances of in0 [rows, F] to a constant set (NearestPack, nearest.hip): out = d2 / sqrt(d2) [rows, set size], or the per-slice best-M lists (out_mode: host/nearest.hpp NearestOut)
  NearestReduce = 33, // in0 = those lists -> the label [rows], the M nearest indices or their distances [rows, M]
  NearestVote = 45,   // in0 = those lists -> the k-NN vote of the M nearest (VotePack, host/nearest.hpp): the class label [rows], the class probabilities [rows, C] or the regression value [rows, 1] (out_mode: VoteOut)
  HDense = 28,        // float16 MatMul / Gemm on the f16 matrix cores: half operands, f32 accumulation, half results served as f32 values (Step::hW, h_bias_mode; hdense.hip)
  ConvTranspose2d = 34,  // transposed convolution by stride phases (the Conv2d geometry fields: C, H, Wd = the input, Mo, OH, OW = the output; W = the ONNX weights [C, M/g, kh, kw]; DeconvPack: the phase tap lists; deconv.hip)
  SpatialNorm = 36,   // InstanceNormalization / GroupNormalization over the (C / groups) * S elements of each of `groups` channel groups of in0 [rows, C, S]: y = act((x - mean) / sqrt(var + ln_eps) * scale[c] + shift[c]); in1 = -1: the fused kernel, else in1 = a SpatialStats result (host/spatialnorm.hpp, spatialnorm.hip)
  SpatialStats = 37,  // out [rows, groups, 3] = (mean, resid, 1 / sqrt(var + ln_eps)) of each group of in0: the first half of the general SpatialNorm plan (the scheduler inserts it, schedule.cpp)
  Tokens = 38,        // out [rows, rep = P + S, K = C] = the window of in0 [rows, C, S] (NCHW or channel quads): out[r, P + s, c] = in0[r, c, s] (+ cst[P + s, c]); rows p < P = prefix[p, c] (+ cst[p, c]) (host/tokens.hpp, tokens.hip)
  ChannelNorm = 39,   // LayerNorm over the C channels at each of the S pixels of in0 [rows, C, S] (NCHW or channel quads, never changed): y = act((x - mean) / sqrt(var + ln_eps) * scale[c] + shift[c]), shift may be empty; out_mode (set by the scheduler): 0 the register form, 1 the re-read form (host/channelnorm.hpp, channelnorm.hip)
  Embed = 40,         // out [rows, F] = pieces in output order: rows of constant tables chosen by index columns of in0 [rows, W] (truncated toward zero, + an offset) and runs of in0's columns as they are; a window [rows, k, d] when the pack says so (EmbedPack, host/embed.hpp, embed.hip)
  Interact = 41,      // feature interactions of in0 [rows, k, d] (rows first, flat): dot mode, out [rows, F] = chosen entries of T . T^T beside bit copies of columns of T; fm mode, out [rows, d] or [rows, 1] = h * ((sum_f T)^2 - sum_f T^2) (InteractPack, host/interact.hpp, interact.hip)
  RmsNorm = 42,       // y = x / sqrt(mean(x^2) + ln_eps) * scale[K] over each of the `rep` vectors of K elements of a row (RMSNormalization; layernorm.hip)
  Rotary = 43,        // rotary position embedding of in0 [rows, attn_T, ld] read through the view (attn_ld[0], attn_off[0]) into a dense [rows, attn_T, attn_heads * attn_dh]: column j < rot_rd of a head, y[j] = fl(fl(x[j] * scale[t, j]) + fl(x[partner(j)] * shift[t, j])), partner(j) = j +- rot_rd / 2 or j ^ 1 (rot_interleaved); the other columns are bit copies (RotaryEmbedding and the rotate_half spelling; rotary.hip)
  PixelShuffle = 44,  // DepthToSpace / SpaceToDepth of in0 [rows, C, H, Wd] to [rows, Mo, OH, OW] with block ps_block: a bit copy of every element, in one of four forms (ps_to_space, ps_channel_major: host/pixelshuffle.hpp); out_mode (set by the scheduler): the PixelShuffleKernel that runs it (pixelshuffle.hip)
  Resize2d = 35,      // nearest / linear Resize (and Upsample) of an [N,C,H,W] tensor to [N,C,OH,OW] from the DeconvPack's row and column tables (resize.hip)
};
// how an HDense step adds its bias: Gemm rounds acc + b once; MatMul -> Add rounds the product first, then the sum
enum HalfBias : int { kHalfBiasNone = 0, kHalfBiasGemm = 1, kHalfBiasMatmulAdd = 2 };

// Constant per-tensor quantisation of an activation: q = sat(rne(x / scale) + zp) in uint8 or int8
struct Quant {
  bool on = false;
  float scale = 1.f;
  int zp = 0;
  bool is_signed = false;  // int8 (else uint8)
  int qmin() const { return is_signed ? -128 : 0; }
  int qmax() const { return is_signed ? 127 : 255; }
  int shift() const { return is_signed ? 0 : 128; }  // q - shift() is the signed byte the matrix instruction reads
  bool operator==(const Quant &o) const { return on == o.on && scale == o.scale && zp == o.zp && is_signed == o.is_signed; }
};
// Largest K of a QDense step with |bias| <= max_bias: K * 255 * 255 + max|bias| stays below 2^31, so the int32 accumulator is exact
inline bool qdense_k_fits(int64_t K, int64_t max_bias) { return K * 255 * 255 + max_bias < (int64_t(1) << 31); }

// RowReduce operators (Step::out_mode)
enum ReduceOp : int {
  kReduceSum = 0, kReduceMean = 1, kReduceMax = 2, kReduceMin = 3, kReduceProd = 4, kReduceL1 = 5, kReduceL2 = 6, kReduceSumSquare = 7,
  kReduceLogSum = 8, kReduceLogSumExp = 9,
};
constexpr int64_t kReduceMaxE = 65536;  // elements per reduced vector

// TreeEnsemble / TreeReduce output modes (Step::out_mode)
enum TreeOut : int { kTreeScores = 0, kTreeLabel = 1, kTreeBinaryScores = 2, kTreeBinaryLabel = 3 };

// SvmKernel / SvmReduce output modes (Step::out_mode): regressor value [rows, 1], one-class +-1 [rows, 1], class label [rows], pairwise
// decisions [rows, P] (binary: [d, -d]), probabilities [rows, C]
enum SvmOut : int { kSvmValue = 0, kSvmOneClass = 1, kSvmLabel = 2, kSvmDecision = 3, kSvmProb = 4 };
// SVM kernel types (SvmPack::kernel)
enum SvmKernelType : int { kSvmLinear = 0, kSvmPoly = 1, kSvmRbf = 2, kSvmSigmoid = 3 };

struct Step {
  StepKind kind = StepKind::Unary;
  int in0 = -1, in1 = -1, out = -1;  // activation buffer ids; 0 is the model input
  Act act = Act::None;               // fused trailing activation
  float act_a = 0.f, act_b = 0.f;    // LeakyRelu alpha / Clip lo,hi
  // Dense
  int64_t K = 0, M = 0;
  // Dense over a window: in0 is [rows, rep, K] and the layer runs on each of its rows * rep vectors (the buffer IS that matrix).
  // LayerNorm / MeanTime: vectors (time steps) per row
  int64_t rep = 1;
  std::vector<float> W;     // [K, M] row-major (Gemm transB / alpha already folded)
  std::vector<float> bias;  // [M] or empty (Gemm beta folded)
  // AffineChannel: scale/shift per channel, S = elements per channel
  std::vector<float> scale, shift;
  int64_t S = 1;
  // BinaryConst / BinaryAct: + - * /  m(in) M(ax) ^(pow)  p(relu: x >= 0 ? x : c*x, BinaryConst only)
  char bop = '+';
  bool const_left = false;
  std::vector<float> cst;  // per_row elements
  std::vector<float> prefix;  // Tokens: the P constant rows in front of the S positions, [P, C] (cst: the position table [P + S, C] or empty)
  // CopyCols: destination column offset (elements inside a row), length = in0's per_row.  SliceCols: SOURCE offset, length K
  int64_t col_off = 0;
  // Softmax
  int64_t sm_outer = 1, sm_len = 1, sm_inner = 1;
  bool log_softmax = false;
  int sm_norm = 0;  // 0: softmax family; row normalisation instead (ai.onnx.ml Normalizer): 1 MAX, 2 L1, 3 L2
  // Conv2d / Pool2d / GlobalAvgPool geometry (per sample)
  int64_t C = 0, H = 0, Wd = 0, Mo = 0, OH = 0, OW = 0;
  int64_t kh = 1, kw = 1, sh = 1, sw = 1, pt = 0, pl = 0, pb = 0, pr = 0, dh = 1, dw = 1, groups = 1;
  bool is_max = false, count_pad = false;
  // LRN: window `lrn_size` channels, y = x / (lrn_bias + lrn_alpha / lrn_size * sum x^2)^lrn_beta
  int64_t lrn_size = 0;
  float lrn_alpha = 1e-4f, lrn_beta = 0.75f, lrn_bias = 1.f;
  // TreeEnsemble / TreeReduce, SvmKernel / SvmReduce, Prep: the packed tables and their sizes (a kernel step and its reduce step share
  // one pack); uploaded table by table into the family's struct of hip/backend.hpp (hip/steps.cpp)
  std::shared_ptr<const TreePack> tree;
  std::shared_ptr<const SvmPack> svm;
  std::shared_ptr<const PrepPack> prep;
  std::shared_ptr<const RnnPack> rnn;
  std::shared_ptr<const NearestPack> nearest;
  std::shared_ptr<const VotePack> vote;  // NearestVote (beside `nearest`, the set whose lists it reads)
  std::shared_ptr<const EmbedPack> embed;
  std::shared_ptr<const InteractPack> interact;
  std::shared_ptr<const DeconvPack> deconv;  // ConvTranspose2d: phase tap lists; Resize2d: source tables
  int out_mode = 0;  // Tree*: TreeOut, Svm*: SvmOut, Recurrent: RnnOut, RowReduce: ReduceOp, TopK: 0 values / 1 indices, Nearest / NearestReduce: NearestOut, NearestVote: VoteOut
  // Attention: Q = in0, K = in1, V = in2 (the same buffer three times when the projections are merged), each [rows, T, ld] with the head
  // block of head g at columns off + g * dh of a step; mask (cst): [T, T] added to the scaled scores, -inf = no weight, empty = none
  int in2 = -1;
  // A row mask (Attention, MeanTime; INTEGRATION.md 2.6 "Padded sequences"): in3 = the buffer that holds the mask's source (the model input;
  // -1: none), step t of a row is kept iff in3[r, rm_off + t] (rm_int: an integer graph input, truncated toward zero) != rm_cmp.
  // Attention: rm_fill reaches a masked key's score by rm_mode (RowMaskMode, host/attention.hpp); rm_excl: the fill excludes the key.
  // MeanTime: the sum over the kept steps is divided by max(count, rm_clip)
  // Recurrent with sequence_lens (INTEGRATION.md 2.6 "Padded windows"): in3 = the same buffer, row r holds in3[r, rm_off] valid steps (rm_int
  // as above); rnn_node = the node's 1-based id in Plan::prep_strict_nodes, the failure word of a length outside 0 .. T
  int in3 = -1;
  int rnn_node = 0;
  int64_t rm_off = 0;
  float rm_cmp = 0.f, rm_fill = 0.f, rm_clip = 0.f;
  int rm_mode = 0;
  bool rm_excl = false, rm_int = false;
  int64_t attn_T = 0, attn_heads = 0, attn_dh = 0, attn_ld[3] = {0, 0, 0}, attn_off[3] = {0, 0, 0};
  // the Attention operator: attn_Tk keys per row (K / V are [rows, attn_Tk, ld], cst [attn_T, attn_Tk]; 0: attn_T),
  // attn_kv_heads heads in K / V (query head g reads head g / (attn_heads / attn_kv_heads); 0: attn_heads), attn_causal: key j counts
  // for query i iff j <= i
  int64_t attn_Tk = 0, attn_kv_heads = 0;
  bool attn_causal = false;
  float attn_scale = 1.f, ln_eps = 1e-5f;
  // Rotary: the window and its view in attn_T, attn_heads, attn_dh, attn_ld[0], attn_off[0]; rot_rd rotated columns per head; the tables
  // A = scale, B = shift, [attn_T, rot_rd] each; rot_const_pos: they were gathered by a constant position_ids (else positions 0 .. T - 1)
  int64_t rot_rd = 0;
  bool rot_interleaved = false, rot_const_pos = false;
  // PixelShuffle: the block size, depth to space (else space to depth), channel-major (CRD / pixel_unshuffle; else block-major: DCR / SpaceToDepth)
  int64_t ps_block = 0;
  bool ps_to_space = false, ps_channel_major = false;
  // FakeQuant: qx.  QDense: qx = how the f32 input is quantised, qy = how the result is (off: the step returns `real`, f32);
  // qW [K, M] = the weights as signed bytes (uint8 data shifted by 128), q_wzp[M] = their zero points shifted the same way, q_mult[M] =
  // x_scale * w_scale[m] in f32, q_bias[M] = the int32 bias added to the accumulator (else `bias`: f32, added after the scaling).
  // QConv2d: the same fields with K = C * kh * kw, M = Mo and row k = (c, ky, kx) of qW in ONNX order
  Quant qx, qy;
  std::vector<int8_t> qW;
  std::vector<int32_t> q_wzp, q_bias;
  std::vector<float> q_mult;
  bool q_w_signed = true, q_per_channel = false;
  // HDense: hW [K, M] = the weights' 16-bit patterns, h_bias [M] = the bias's (empty: none), h_bias_mode = HalfBias
  std::vector<uint16_t> hW, h_bias;
  int h_bias_mode = kHalfBiasNone;
  std::string origin;  // ONNX node names/ops this step came from (diagnostics)
};

struct Plan {
  std::vector<int64_t> input_shape, output_shape;  // -1 = symbolic (engine.rs:64-73)
  std::vector<std::vector<int64_t>> buf_shape;     // per activation buffer, dim0 = -1 or the fixed batch
  std::vector<int64_t> buf_per_row;                // elements per row of each buffer
  std::vector<Step> steps;
  int out_buf = 0;
  int64_t fixed_batch = -1;  // > 0 when the model's leading dim is a constant (e.g. linear.onnx [1,3])
  int64_t opset = 1;
  std::string output_name;         // the served graph output
  std::string output_declared_type;  // "" for f32; "int64" / "int32" / "float16" when the graph declares such an output that is served as f32 VALUES
  std::string input_declared_type;   // "float16" when the graph declares a half input: the f32 values of a call are rounded to half first
  bool output_zipmap = false;        // the served output is a ZipMap's: its input [rows, C] is served, one column per class label
  // the checks a call can fail on the device, by 1-based id (the ids in the Prep and Embed descriptors): a call whose failure word is set
  // fails with `node` + `message` of that entry.  node: "node 'name' (OneHotEncoder)" of a zeros = 0 one-hot encoder, "node 'name' (Gather)"
  // of an embedding lookup, "node 'name' (LSTM)" of a recurrent layer with sequence_lens
  struct StrictNode {
    std::string node, message;
  };
  std::vector<StrictNode> prep_strict_nodes;

  int64_t in_per_row() const { return buf_per_row[0]; }
  int64_t out_per_row() const { return buf_per_row[out_buf]; }
  double flops_per_row() const;  // 2*MACs of Dense/Conv steps (bias/activation excluded)
  std::string describe_json() const;
};

// Throws InferaError::onnx on unsupported graphs.
// output_select: "" = the first graph output (the reference's behaviour), else an output's name or decimal index.
Plan lower_model(const onnx::Model &m, const std::string &output_select = "");

}  // namespace infera_hip
