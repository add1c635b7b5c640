// steps.cpp -- per kernel family, side by side: upload_X fills the family's tables (backend.hpp) from the Step or its pack, in the order its
// kernel walks them, and launch_X hands them to kern::X.  upload_step (load time, model.cpp's loop) and PassRunner::launch_fused /
// launch_plain (every pass, exec.cpp's loop) pick the pair by ExecKind / StepKind.  A new family adds its struct, its pair and its two cases.
#include <cstdlib>

#include "../host/deconv.hpp"
#include "../host/embed.hpp"
#include "../host/interact.hpp"
#include "../host/nearest.hpp"
#include "../host/channelnorm.hpp"
#include "../host/onnx_model.hpp"
#include "../host/pixelshuffle.hpp"
#include "../host/prep.hpp"
#include "../host/recurrent.hpp"
#include "../host/spatialnorm.hpp"
#include "../host/svm.hpp"
#include "../host/tokens.hpp"
#include "../host/trees.hpp"
#include "runtime.hpp"

namespace infera_hip {
namespace rt {

kern::ConvTGeom convt_geom(const Step &s) {
  return kern::ConvTGeom{int(s.C), int(s.H), int(s.Wd), int(s.Mo), int(s.OH), int(s.OW), int(s.kh), int(s.kw), int(s.sh), int(s.sw),
                         int(s.pt), int(s.pl), int(s.groups), s.deconv->h_stride, s.deconv->w_stride};
}

namespace {

// `v` padded with zeros to n floats (channel / feature counts rounded up to what a kernel's tiles need)
std::vector<float> zero_padded(const std::vector<float> &v, size_t n) {
  std::vector<float> out(n, 0.f);
  std::copy(v.begin(), v.end(), out.begin());
  return out;
}

// ---- the whole-chain fused MLP (mlp_fused.hip) and the load-time specialised chain (chain_device.inc) ---------------------------------
void upload_mlp3(const Upload &up, size_t i) {
  const Step &s1 = up.m.plan.steps[i], &s2 = up.m.plan.steps[i + 1], &s3 = up.m.plan.steps[i + 2];
  std::vector<float> packed(kern::mlp3_packed_floats(up.m.mlp3_shape));
  kern::mlp3_pack(up.m.mlp3_shape, s1.W.data(), s1.bias.empty() ? nullptr : s1.bias.data(), s2.W.data(), s2.bias.empty() ? nullptr : s2.bias.data(),
                  s3.W.data(), s3.bias.empty() ? nullptr : s3.bias.data(), packed.data());
  up.dm.mlp3_packed = up(packed);
}
void launch_mlp3(const PassRunner &r, size_t i, bool cm) {
  const Step &x = r.st[i];
  std::string why;
  // (the tile queue of the stream this pass runs on: the context's own, or one of its lanes')
  if (!kern::mlp3(r.stream, r.m.mlp3_shape, r.buf(x.in0), r.dm.mlp3_packed, r.buf(r.st[i + 2].out), r.nr * x.rep, r.dm.num_cus,
                  r.ctx.mlp_queue_of(r.stream), &why, cm))
    throw InferaError::onnx("fused MLP kernel launch failed: " + why);
}

void upload_chain(const Upload &up, size_t i) {
  const LoadedModel::ChainRun &run = *up.m.chain_at(i);
  std::vector<const float *> W, B;
  for (size_t l = 0; l < run.shape.dims.size(); l++) {
    const Step &ls = up.m.plan.steps[i + size_t(run.pad) + l];
    W.push_back(ls.W.data());
    B.push_back(ls.bias.empty() ? nullptr : ls.bias.data());
  }
  std::vector<float> packed(kern::chain_packed_floats(run.shape));
  kern::chain_pack(run.shape, W, B, packed.data());
  up.dm.chain_packed.resize(up.m.chains.size(), nullptr);
  up.dm.chain_packed[size_t(&run - up.m.chains.data())] = up(packed);
}
void launch_chain(const PassRunner &r, size_t i, bool cm) {
  const LoadedModel::ChainRun &run = *r.m.chain_at(i);
  std::string why;
  if (!kern::chain(r.stream, run.shape, r.buf(r.st[i].in0), r.dm.chain_packed[size_t(&run - r.m.chains.data())], r.buf(r.st[i + size_t(run.nsteps) - 1].out),
                   r.nr * r.st[i + size_t(run.pad)].rep, r.dm.num_cus, &why, cm))
    throw InferaError::onnx("fused chain kernel launch failed: " + why);
}

// ---- convolutions on the tiled / split kernels (conv.hip, conv_split.hip): W = the fragment-major filter, bias padded or summed as packed ----
void upload_conv_tiled(const Upload &up, size_t i, PlainTables &t) {
  const Step &s = up.m.plan.steps[i];
  const kern::ConvGeom g = conv_geom(s), gp = kern::conv2d_tiled_geom(g);
  std::vector<float> packed(kern::conv2d_tiled_packed_floats(gp));
  if (gp.padc) {  // channel counts padded to 32: zero weights and zero bias beyond the real ones
    const size_t taps = size_t(g.kh) * g.kw;
    std::vector<float> wt(size_t(gp.M) * gp.C * taps, 0.f);
    for (int mo = 0; mo < g.M; mo++) std::copy_n(s.W.begin() + size_t(mo) * g.C * taps, size_t(g.C) * taps, wt.begin() + size_t(mo) * gp.C * taps);
    kern::conv2d_tiled_pack(gp, wt.data(), packed.data());
    t.W = up(packed);
    if (!s.bias.empty()) t.bias = up(zero_padded(s.bias, size_t(gp.M)));
    return;
  }
  std::vector<float> bias(s.bias);
  if (!up.m.conv_split6[i]) {
    kern::conv2d_tiled_pack(g, s.W.data(), packed.data());
  } else {
    const size_t main_floats = kern::conv2d_split6_packed_floats(g);
    packed.resize(main_floats);
    kern::conv2d_split6_pack(g, s.W.data(), packed.data());
    if (const int fl = up.m.conv_fold[i]; fl >= 0) {  // the folded 1x1 shortcut: its chunks behind the main filter's, its bias added to this layer's
      const Step &q = up.m.plan.steps[size_t(fl)];
      const kern::ConvGeom gq{int(q.C), int(q.H), int(q.Wd), int(q.Mo), int(q.OH), int(q.OW), 1, 1, int(q.sh), int(q.sw), 0, 0, 1, 1, 1};
      packed.resize(main_floats + kern::conv2d_split6_packed_floats(gq));
      kern::conv2d_split6_pack(gq, q.W.data(), packed.data() + main_floats);
      for (size_t k = 0; k < bias.size() && k < q.bias.size(); k++) bias[k] += q.bias[k];
    }
  }
  t.W = up(packed);
  t.bias = up(bias);
}
void launch_conv_tiled(const PassRunner &r, size_t i, const PlainTables &t) {
  const Step &x = r.st[i];
  const int fj = r.m.conv_fused_add[i];
  const kern::ConvGeom gp = kern::conv2d_tiled_geom(conv_geom(x));
  const Step &last = fj >= 0 ? r.st[size_t(fj)] : x;  // whose activation and output the launch carries (a fused residual Add's)
  if (r.m.conv_split6[i] && r.m.conv_fold[i] >= 0) {
    const Step &q = r.st[size_t(r.m.conv_fold[i])];
    const kern::SecondInput x2{r.buf(q.in0), int(q.C), int(q.H), int(q.Wd), int(q.sh), int(q.sw)};
    kern::conv2d_split6(r.stream, r.buf(x.in0), t.W, t.bias, nullptr, r.buf(last.out), r.nr, gp, act_of(last), x2);
    return;
  }
  const float *residual = fj >= 0 ? r.buf(r.m.conv_residual_buf[i]) : nullptr;
  if (r.m.conv_split6[i]) kern::conv2d_split6(r.stream, r.buf(x.in0), t.W, t.bias, residual, r.buf(last.out), r.nr, gp, act_of(last));
  else kern::conv2d_tiled(r.stream, r.buf(x.in0), t.W, t.bias, residual, r.buf(last.out), r.nr, gp, act_of(last));
}

// ---- a Dense layer on the tiled convolution kernel: K and M padded to 32 ----
void upload_dense_tiled(const Step &s, PlainTables &t, const Upload &up) {
  const kern::ConvGeom g = dense_as_conv(s);
  std::vector<float> wt(size_t(g.C) * g.M, 0.f), packed(kern::conv2d_tiled_packed_floats(g));
  for (int64_t k = 0; k < s.K; k++)
    for (int64_t j = 0; j < s.M; j++) wt[size_t(j) * g.C + size_t(k)] = s.W[size_t(k * s.M + j)];  // [K][M] -> conv's [Mp][Cp]
  kern::conv2d_tiled_pack(g, wt.data(), packed.data());
  t.W = up(packed);
  if (!s.bias.empty()) t.bias = up(zero_padded(s.bias, size_t(g.M)));
}
void launch_dense_tiled(const PassRunner &r, const Step &x, const PlainTables &t) {
  kern::conv2d_tiled(r.stream, r.buf(x.in0), t.W, t.bias, nullptr, r.buf(x.out), r.nr * x.rep, dense_as_conv(x), act_of(x));
}

// ---- the stem's patch kernel, alone or with the MaxPool behind it (then, on a split plan, in both arithmetics) ----
void upload_conv_patch(const Upload &up, size_t i, PlainTables &t) {
  const Step &s = up.m.plan.steps[i];
  const kern::ConvGeom g = conv_geom(s), gp = kern::conv2d_patch_geom(g);
  std::vector<float> packed(kern::conv2d_patch_packed_floats(gp));
  if (gp.mvalid > 0) {  // output features padded to whole tiles: zero weights and bias beyond the real ones
    kern::conv2d_patch_pack(gp, zero_padded(s.W, size_t(gp.M) * g.C * g.kh * g.kw).data(), packed.data());
    t.W = up(packed);
    if (!s.bias.empty()) t.bias = up(zero_padded(s.bias, size_t(gp.M)));
    return;
  }
  if (const int fj = up.m.conv_fused_pool[i]; fj >= 0) {
    const kern::PoolTail tail = pool_tail(up.m.plan.steps[size_t(fj)]);
    kern::conv2d_patch_pack(g, s.W.data(), packed.data(), &tail);
    if (up.m.stem_split6[i]) {  // (the exact-fp32 blob stays: INFERA_STEM_SPLIT=0 at run time compares the two)
      std::vector<float> sp(kern::conv2d_stem_split6_packed_floats());
      kern::conv2d_stem_split6_pack(g, s.W.data(), sp.data());
      t.stem_split = up(sp);
    }
  } else {
    kern::conv2d_patch_pack(g, s.W.data(), packed.data());
  }
  t.W = up(packed);
  t.bias = up(s.bias);
}
void launch_conv_patch(const PassRunner &r, size_t i, const PlainTables &t) {
  const Step &x = r.st[i];
  const kern::ConvGeom gp = kern::conv2d_patch_geom(conv_geom(x));
  const int fj = r.m.conv_fused_pool[i];
  if (fj < 0) {
    kern::conv2d_patch(r.stream, r.buf(x.in0), t.W, t.bias, r.buf(x.out), r.nr, gp, act_of(x), r.dm.num_cus);
    return;
  }
  const Step &q = r.st[size_t(fj)];
  const char *sse = getenv("INFERA_STEM_SPLIT");  // 0: the exact-fp32 stem kernels under a split plan (read per launch: tests, A/B)
  if (r.m.stem_split6[i] && t.stem_split && !(sse && atoi(sse) == 0))
    kern::conv2d_stem_split6(r.stream, r.buf(x.in0), t.stem_split, t.bias, r.buf(q.out), r.nr, gp, act_of(x), pool_tail(q), r.dm.num_cus);
  else
    kern::conv2d_patch_pool(r.stream, r.buf(x.in0), t.W, t.bias, r.buf(q.out), r.nr, gp, act_of(x), pool_tail(q), r.dm.num_cus);
}

// ---- depthwise convolutions: W = [C/4][tap][4] ----
void upload_conv_depthwise(const Step &s, PlainTables &t, const Upload &up) {
  std::vector<float> packed(s.W.size());
  kern::conv2d_depthwise_pack(conv_geom(s), s.W.data(), packed.data());
  t.W = up(packed);
  t.bias = up(s.bias);
}
void launch_conv_depthwise(const PassRunner &r, const Step &x, const PlainTables &t) {
  kern::conv2d_depthwise(r.stream, r.buf(x.in0), t.W, t.bias, r.buf(x.out), r.nr, conv_geom(x), act_of(x));
}

// ---- quantised layers (qdense.hip, qconv.hip): mult, c0, wz and the f32 bias, each padded to Mp entries, behind the weight fragments.
// c0[m] = -xz * colsum[m] + K * xz * wz[m] + the int32 bias, mod 2^32; wz = the shifted weight zero points (none when all are 0)
void upload_quant_tables(const Step &s, QuantTables &t, int Mp, const Upload &up) {
  const int K = int(s.K), M = int(s.M);
  t.mult = up(zero_padded(s.q_mult, size_t(Mp)));
  const int64_t xz = int64_t(s.qx.zp) - s.qx.shift();
  std::vector<int> c0(size_t(Mp), 0), wz(size_t(Mp), 0);
  bool any_wz = false;
  for (int j = 0; j < M; j++) {
    int64_t colsum = 0;
    for (int k = 0; k < K; k++) colsum += s.qW[size_t(k) * M + j];
    const int64_t z = s.q_wzp[size_t(j)];
    c0[size_t(j)] = int(uint32_t(uint64_t(-xz * colsum + int64_t(K) * xz * z + (s.q_bias.empty() ? 0 : int64_t(s.q_bias[size_t(j)])))));
    wz[size_t(j)] = int(z);
    any_wz = any_wz || z != 0;
  }
  t.c0 = up(c0);
  if (any_wz) t.wz = up(wz);
  if (!s.bias.empty()) t.bias = up(zero_padded(s.bias, size_t(Mp)));
}
void upload_qdense(const Step &s, QuantTables &t, const Upload &up) {
  const int K = int(s.K), M = int(s.M);
  std::vector<float> packed(kern::qdense_packed_floats(K, M));
  kern::qdense_pack(K, M, s.qW.data(), packed.data());
  t.Wfrag = up(packed);
  upload_quant_tables(s, t, kern::qdense_padded_m(M), up);
}
void launch_qdense(const PassRunner &r, size_t i, const QuantTables &t) {
  const Step &x = r.st[i];
  kern::QDenseLaunch q;
  fill_quant(q, x);
  q.y_shift = x.qy.shift();
  q.X = r.buf(x.in0), q.Y = r.buf(x.out), q.rows = r.nr * x.rep;
  q.Wp = t.Wfrag, q.mult = t.mult, q.bias = t.bias, q.c0 = t.c0, q.wz = t.wz;
  q.K = int(x.K), q.M = int(x.M);
  q.in_bytes = r.m.q_in_bytes[i] != 0, q.out_bytes = r.m.q_out_bytes[i] != 0;
  kern::qdense(r.stream, q);
}
// (the weight fragments in the kernel's (channel chunk, tap, channel) order)
void upload_qconv(const Step &s, QuantTables &t, const Upload &up) {
  const int taps = int(s.kh * s.kw);
  std::vector<float> packed(kern::qconv_packed_floats(int(s.C), taps, int(s.M)));
  kern::qconv_pack(int(s.C), taps, int(s.M), s.qW.data(), packed.data());
  t.Wfrag = up(packed);
  upload_quant_tables(s, t, kern::qconv_padded_m(int(s.M)), up);
}
void launch_qconv(const PassRunner &r, const Step &x, const QuantTables &t) {
  kern::QConvLaunch q = qconv_launch(x);
  q.X = r.buf(x.in0), q.Y = r.buf(x.out), q.rows = r.nr;
  q.Wfrag = t.Wfrag, q.mult = t.mult, q.bias = t.bias, q.c0 = t.c0, q.wz = t.wz;
  q.in_cq = r.cq(x.in0), q.out_cq = r.cq(x.out);
  const char *stage = getenv("INFERA_QCONV_STAGE");  // 0: quantise per tap from global memory, no LDS window (read per launch: tests, A/B)
  q.force_direct = stage && atoi(stage) == 0;
  kern::qconv(r.stream, q);
}

// ---- float16 layers (hdense.hip): the weight fragments (half bit patterns), the half bias widened to f32 and padded ----
void upload_hdense(const Step &s, HalfTables &t, const Upload &up) {
  const int K = int(s.K), M = int(s.M);
  std::vector<float> packed(kern::hdense_packed_floats(K, M));
  kern::hdense_pack(K, M, s.hW.data(), packed.data());
  t.Wp = up(packed);
  if (s.h_bias_mode != kHalfBiasNone) {
    std::vector<float> b(size_t(kern::hdense_padded_m(M)), 0.f);
    for (size_t j = 0; j < s.h_bias.size(); j++) b[j] = onnx::half_to_float(s.h_bias[j]);
    t.bias = up(b);
  }
}
void launch_hdense(const PassRunner &r, size_t i, const HalfTables &t) {
  const Step &x = r.st[i];
  kern::HDenseLaunch h;
  h.X = r.buf(x.in0), h.Y = r.buf(x.out), h.rows = r.nr * x.rep;
  h.Wp = t.Wp, h.bias = t.bias, h.bias_mode = x.h_bias_mode;
  h.K = int(x.K), h.M = int(x.M);
  h.act = int(x.act), h.act_a = x.act_a, h.act_b = x.act_b;
  h.in_half = r.m.h_in_half[i] != 0, h.out_half = r.m.h_out_half[i] != 0;
  kern::hdense(r.stream, h);
}

// ---- tree ensembles (host/trees.hpp TreePack, trees.hip) ----
void upload_tree_walk(const Step &s, TreeWalkTables &t, const Upload &up) {
  t.tab = up(s.tree->tab);
  t.leaves = up(s.tree->leaves);
}
void launch_tree_walk(const PassRunner &r, const Step &x, const TreeWalkTables &t) {
  const TreePack &k = *x.tree;
  kern::tree_walk(r.stream, r.buf(x.in0), int(r.p.buf_per_row[size_t(x.in0)]), t.tab, k.nodes, k.trees, t.leaves, int(k.W), int(k.slices), r.buf(x.out), r.nr);
}
void upload_tree_reduce(const Step &s, TreeReduceTables &t, const Upload &up) {
  t.base = up(s.tree->base);
  t.labels = up(s.tree->labels);
}
void launch_tree_reduce(const PassRunner &r, const Step &x, const TreeReduceTables &t) {
  const TreePack &k = *x.tree;
  kern::tree_reduce(r.stream, r.buf(x.in0), t.base, t.labels, r.buf(x.out), r.nr, int(k.W), int(k.slices), k.trees, k.average, x.out_mode, k.is_signed);
}

// ---- support-vector machines (host/svm.hpp SvmPack, svm.hip) ----
void upload_svm_kernel(const Step &s, SvmKernelTables &t, const Upload &up) {
  t.sv = up(s.svm->sv);
  t.coef = up(s.svm->coef);
  t.sv_norm = up(s.svm->sv_norm);
  t.center = up(s.svm->center);
  t.slice_tile = up(s.svm->slice_tile);
}
void launch_svm_kernel(const PassRunner &r, const Step &x, const SvmKernelTables &t) {
  const SvmPack &v = *x.svm;
  if (!kern::svm_kernel(r.stream, r.buf(x.in0), int(r.p.buf_per_row[size_t(x.in0)]), int(v.F_pad), v.kernel, t.center, t.sv, t.sv_norm, t.coef,
                        t.slice_tile, r.buf(x.out), r.nr, int(v.slices), int(v.Q), int(v.QW), v.gamma, v.coef0, v.degree))
    throw InferaError::onnx("SVM kernel launch failed: '" + x.origin + "' (F = " + std::to_string(v.F) + ") could not be given its LDS");
}
void upload_svm_reduce(const Step &s, SvmReduceTables &t, const Upload &up) {
  t.rho = up(s.svm->rho);
  t.labels = up(s.svm->labels);
  t.prob_a = up(s.svm->prob_a);
  t.prob_b = up(s.svm->prob_b);
  t.class_slice = up(s.svm->class_slice);
}
void launch_svm_reduce(const PassRunner &r, const Step &x, const SvmReduceTables &t) {
  kern::svm_reduce(r.stream, r.buf(x.in0), t.class_slice, t.rho, t.labels, t.prob_a, t.prob_b, r.buf(x.out), r.nr, int(x.svm->Q), int(x.svm->classes), x.out_mode);
}

// ---- distance models (host/nearest.hpp NearestPack, nearest.hip; NearestReduce has no tables) ----
void upload_nearest(const Step &s, NearestTables &t, const Upload &up) {
  t.ref = up(s.nearest->ref);
  t.ref_norm = up(s.nearest->ref_norm);
  t.center = up(s.nearest->center);
  t.slice_tile = up(s.nearest->slice_tile);
}
void launch_nearest(const PassRunner &r, const Step &x, const NearestTables &t) {
  const NearestPack &q = *x.nearest;
  if (!kern::nearest(r.stream, r.buf(x.in0), int(q.F), int(q.F_pad), t.center, t.ref, t.ref_norm, t.slice_tile, r.buf(x.out), r.nr, int(q.slices), int(q.M),
                     int(x.M), x.out_mode))
    throw InferaError::onnx("nearest kernel launch failed: '" + x.origin + "' could not be given its LDS");
}

// the k-NN vote over a Nearest step's lists (host/nearest.hpp VotePack)
void upload_nearest_vote(const Step &s, NearestVoteTables &t, const Upload &up) {
  t.cls = up(s.vote->cls);
  t.target = up(s.vote->target);
  t.class_value = up(s.vote->class_value);
}
void launch_nearest_vote(const PassRunner &r, const Step &x, const NearestVoteTables &t) {
  const VotePack &v = *x.vote;
  if (!kern::nearest_vote(r.stream, r.buf(x.in0), t.cls, t.target, t.class_value, r.buf(x.out), r.nr, int(x.nearest->slices), int(x.nearest->M), int(x.M),
                          int(v.classes), x.out_mode, v.weighted, v.rooted, v.eps))
    throw InferaError::onnx("nearest vote kernel launch failed: '" + x.origin + "' is beyond the kernel's caps");
}

// ---- preprocessing regions (host/prep.hpp PrepPack, prep.hip) ----
void upload_prep(const Step &s, PrepTables &t, const Upload &up) {
  t.desc = up(s.prep->desc);
  t.cst = up(s.prep->cst);
  t.tab = up(s.prep->tab);
}
void launch_prep(const PassRunner &r, const Step &x, const PrepTables &t) {
  const PrepPack &q = *x.prep;
  kern::prep(r.stream, r.buf(x.in0), int(q.F_in), t.desc, t.cst, t.tab, int(q.tab.size() / 2), r.buf(x.out), int(q.F), r.nr, int(q.R),
             q.strict ? r.ctx.prep_err : nullptr);
}

// ---- recurrent layers (host/recurrent.hpp RnnPack, rnn.hip) ----
void upload_rnn(const Step &s, RnnTables &t, const Upload &up) {
  t.wr = up(s.rnn->wr);
  t.bias = up(s.rnn->bias);
  t.bias2 = up(s.rnn->bias2);
  t.h0 = up(s.rnn->h0);
  t.c0 = up(s.rnn->c0);
}
void launch_rnn(const PassRunner &r, const Step &x, const RnnTables &t) {
  const RnnPack &k = *x.rnn;
  const bool lens = x.in3 >= 0;  // per-row sequence lengths: a column of the input buffer, which such plans take row-major (schedule.cpp)
  if (lens && r.in_colmajor) throw InferaError::onnx("internal: '" + x.origin + "' reads sequence_lens from a column-major chunk");
  if (!kern::rnn(r.stream, r.buf(x.in0), t.wr, t.bias, t.bias2, t.h0, t.c0, r.buf(x.out), r.nr, k.op, int(k.T), int(k.F), int(k.H), int(k.D), k.reverse, k.lbr,
                 k.relu, x.out_mode, r.in_colmajor && x.in0 == 0, lens ? r.buf(x.in3) : nullptr, lens ? r.p.buf_per_row[size_t(x.in3)] : 0, int(x.rm_off),
                 x.rm_int, lens ? r.ctx.prep_err : nullptr, x.rnn_node))
    throw InferaError::onnx("recurrent kernel launch failed: '" + x.origin + "' could not be given its LDS");
}

// ---- transposed convolutions (host/deconv.hpp DeconvPack, deconv.hip): the MFMA phase kernel's fragments and phase offsets, or the
// generic kernel's [tap][C][M/g] weights; both read the pack's axis tables ----
void upload_convt(const Upload &up, size_t i, ConvTKernelTables &t) {
  const Step &s = up.m.plan.steps[i];
  const kern::ConvTGeom g = convt_geom(s);
  std::vector<int32_t> tab = s.deconv->tab;
  if (up.m.exec[i] == ExecKind::ConvTPhase) {
    std::vector<float> packed(kern::convt2d_phase_packed_floats(g, tab.data()));
    std::vector<int32_t> off(size_t(g.sh) * g.sw, 0);
    kern::convt2d_phase_pack(g, tab.data(), s.W.data(), packed.data(), off.data());
    tab.insert(tab.end(), off.begin(), off.end());
    t.W = up(packed);
  } else {
    std::vector<float> packed(s.W.size());
    kern::convt2d_generic_pack(g, s.W.data(), packed.data());
    t.W = up(packed);
  }
  t.bias = up(s.bias);
  t.tab = up(tab);
}
void launch_convt(const PassRunner &r, size_t i, const ConvTKernelTables &t) {
  const Step &x = r.st[i];
  if (r.m.exec[i] == ExecKind::ConvTPhase)
    kern::convt2d_phase(r.stream, r.buf(x.in0), t.W, t.bias, r.buf(x.out), t.tab, r.nr, convt_geom(x), x.deconv->max_phase_pixels, act_of(x), r.cq(x.out));
  else
    kern::convt2d_generic(r.stream, r.buf(x.in0), t.W, t.bias, r.buf(x.out), t.tab, r.nr, convt_geom(x), act_of(x), r.cq(x.in0), r.cq(x.out));
}

// ---- Resize / Upsample (resize.hip): the row and column source tables ----
void upload_resize(const Step &s, ResizeTables &t, const Upload &up) {
  t.row_idx = up(s.deconv->row_idx);
  t.col_idx = up(s.deconv->col_idx);
  t.row_wgt = up(s.deconv->row_wgt);
  t.col_wgt = up(s.deconv->col_wgt);
}
void launch_resize(const PassRunner &r, const Step &x, const ResizeTables &t) {
  kern::resize2d(r.stream, r.buf(x.in0), r.buf(x.out), r.nr, int(x.C), int(x.H), int(x.Wd), int(x.OH), int(x.OW), t.row_idx, t.col_idx, t.row_wgt, t.col_wgt,
                 x.deconv->linear, r.cq(x.in0));
}

// ---- InstanceNormalization / GroupNormalization (host/spatialnorm.hpp, spatialnorm.hip): gamma and beta per channel; SpatialStats has no tables ----
void upload_spatialnorm(const Step &s, SpatialNormTables &t, const Upload &up) {
  t.gamma = up(s.scale);
  t.beta = up(s.shift);
}
void launch_spatialnorm(const PassRunner &r, const Step &x, const SpatialNormTables &t) {
  if (r.cq(x.in0) != r.cq(x.out)) throw InferaError::onnx("SpatialNorm '" + x.origin + "' would have to change the tensor's layout; there is no such kernel");
  const bool ok = x.in1 < 0 ? kern::spatialnorm_fused(r.stream, r.buf(x.in0), t.gamma, t.beta, r.buf(x.out), r.nr, int(x.C), int(x.S), int(x.groups), r.cq(x.in0), x.ln_eps, act_of(x))
                            : kern::spatialnorm_apply(r.stream, r.buf(x.in0), r.buf(x.in1), t.gamma, t.beta, r.buf(x.out), r.nr, int(x.C), int(x.S), int(x.groups), r.cq(x.in0), act_of(x));
  if (!ok) throw InferaError::onnx("SpatialNorm kernel launch failed: '" + x.origin + "' is beyond the kernel's caps");
}
void launch_spatialstats(const PassRunner &r, const Step &x) {
  if (!kern::spatialnorm_stats(r.stream, r.buf(x.in0), r.buf(x.out), r.nr, int(x.C), int(x.S), int(x.groups), r.cq(x.in0), x.ln_eps))
    throw InferaError::onnx("SpatialStats kernel launch failed: '" + x.origin + "' is beyond the kernel's caps");
}

// ---- ChannelNorm (host/channelnorm.hpp, channelnorm.hip): gamma and, where the layer has one, beta per channel ----
void upload_channelnorm(const Step &s, ChannelNormTables &t, const Upload &up) {
  t.gamma = up(s.scale);
  t.beta = s.shift.empty() ? nullptr : up(s.shift);
}
void launch_channelnorm(const PassRunner &r, const Step &x, const ChannelNormTables &t) {
  if (r.cq(x.in0) != r.cq(x.out)) throw InferaError::onnx("ChannelNorm '" + x.origin + "' would have to change the tensor's layout; there is no such kernel");
  const bool cq = r.cq(x.in0) && x.S > 1;  // (an [N,C,1,1] tensor is the same floats in either layout)
  if (!kern::channelnorm(r.stream, r.buf(x.in0), t.gamma, t.beta, r.buf(x.out), r.nr, int(x.C), int(x.S), cq, x.out_mode == 0, x.ln_eps, act_of(x)))
    throw InferaError::onnx("ChannelNorm kernel launch failed: '" + x.origin + "' is beyond the kernel's caps");
}

// ---- Tokens (host/tokens.hpp, tokens.hip): the constant rows and the position table, either may be absent ----
void upload_tokens(const Step &s, TokensTables &t, const Upload &up) {
  t.prefix = s.prefix.empty() ? nullptr : up(s.prefix);
  t.pos = s.cst.empty() ? nullptr : up(s.cst);
}
void launch_tokens(const PassRunner &r, const Step &x, const TokensTables &t) {
  const bool cq = r.cq(x.in0) && x.S > 1;  // (an [N,C,1,1] tensor is the same floats in either layout)
  if (!kern::tokens(r.stream, r.buf(x.in0), t.prefix, t.pos, r.buf(x.out), r.nr, int(x.C), int(x.S), int(x.rep - x.S), cq))
    throw InferaError::onnx("Tokens kernel launch failed: '" + x.origin + "' is beyond the kernel's caps");
}

// ---- Embed (host/embed.hpp EmbedPack, embed.hip): the piece descriptors, the column -> piece map (short rows) and the tables ----
void upload_embed(const Step &s, EmbedTables &t, const Upload &up) {
  t.desc = up(s.embed->desc);
  t.map = s.embed->map.empty() ? nullptr : up(s.embed->map);
  t.tab = up(s.embed->tab);
}
void launch_embed(const PassRunner &r, const Step &x, const EmbedTables &t) {
  const EmbedPack &q = *x.embed;
  if (r.in_colmajor && x.in0 == 0) throw InferaError::onnx("internal: an Embed step reads its input row-major");
  // non-temporal stores: 4-8 % off an Embed -> Relu model where a pass writes more than the caches hold, no difference where it does not
  // (profiles/r19_embed.txt); INFERA_EMBED_NT=0: plain stores, the same bits (A/B: tools/embed_time.py)
  static const bool nt = !(getenv("INFERA_EMBED_NT") && atoi(getenv("INFERA_EMBED_NT")) == 0);
  if (!kern::embed(r.stream, r.buf(x.in0), int(q.W), t.desc, int(q.pieces.size()), t.map, int(q.map.size()), t.tab, r.buf(x.out), q.F, r.nr, q.R, q.staged,
                   r.ctx.prep_err, nt))
    throw InferaError::onnx("Embed kernel launch failed: '" + x.origin + "' is beyond the kernel's caps");
}

// ---- Interact (host/interact.hpp InteractPack, interact.hip): dot mode's output column map; fm mode has no tables ----
void upload_interact(const Step &s, InteractTables &t, const Upload &up) {
  if (s.interact->mode == kInteractDot) t.map = up(s.interact->map);
}
void launch_interact(const PassRunner &r, const Step &x, const InteractTables &t) {
  const InteractPack &q = *x.interact;
  if (r.in_colmajor && x.in0 == 0) throw InferaError::onnx("internal: an Interact step reads its input row-major");
  const bool ok = q.mode == kInteractDot ? kern::interact_dot(r.stream, r.buf(x.in0), int(q.k), int(q.d), q.tile, t.map, q.F, r.buf(x.out), r.nr)
                                         : kern::interact_fm(r.stream, r.buf(x.in0), int(q.k), int(q.d), q.h, q.has_h, q.h_after, q.sum_last, r.buf(x.out), r.nr);
  if (!ok) throw InferaError::onnx("Interact kernel launch failed: '" + x.origin + "' is beyond the kernel's caps");
}

// ---- Rotary (rotary.hip): the two [T, rd] factor tables, as the lowering built them ----
void upload_rotary(const Step &s, RotaryTables &t, const Upload &up) {
  t.A = up(s.scale);
  t.B = up(s.shift);
}
void launch_rotary(const PassRunner &r, const Step &x, const RotaryTables &t) {
  if (r.in_colmajor && x.in0 == 0) throw InferaError::onnx("internal: a Rotary step reads its input row-major");
  if (!kern::rotary(r.stream, r.buf(x.in0), x.attn_ld[0], x.attn_off[0], t.A, t.B, r.buf(x.out), r.nr, int(x.attn_T), int(x.attn_heads), int(x.attn_dh), int(x.rot_rd),
                    x.rot_interleaved))
    throw InferaError::onnx("Rotary kernel launch failed: '" + x.origin + "' is beyond the kernel's caps");
}

// ---- PixelShuffle (pixelshuffle.hip): no tables; the scheduler chose the form for the two layouts (Step::out_mode) ----
void launch_pixelshuffle(const PassRunner &r, const Step &x) {
  if (r.in_colmajor && x.in0 == 0) throw InferaError::onnx("internal: a PixelShuffle step reads its input row-major");
  const kern::PixelShuffleGeom g{int(x.ps_block), int(x.C), int(x.H), int(x.Wd), int(x.Mo), int(x.OH), int(x.OW), x.ps_to_space, x.ps_channel_major};
  if (!kern::pixel_shuffle(r.stream, r.buf(x.in0), r.buf(x.out), r.nr, g, x.out_mode, r.cq(x.in0), r.cq(x.out)))
    throw InferaError::onnx("PixelShuffle kernel launch failed: '" + x.origin + "' was scheduled as " + pixelshuffle_kernel_name(x.out_mode) + " for other layouts than it meets");
}

// ---- the plain family: the step's constants as the lowering left them (Conv2d: packed for the generic kernel); its launches are the head
// of PassRunner::launch_plain, right below ----
void upload_plain(const Step &s, PlainTables &t, const Upload &up) {
  if (s.kind == StepKind::Conv2d) {
    const kern::ConvGeom g = conv_geom(s);
    if (!kern::conv2d_generic_supported(g))
      throw InferaError::onnx("Conv with (C/group)*kh*kw = " + std::to_string(s.K) + " > 8192 is not supported by the generic kernel");
    std::vector<float> packed(s.W.size());
    kern::conv2d_generic_pack(g, s.W.data(), packed.data());
    t.W = up(packed);
  } else {
    t.W = up(s.W);
  }
  t.bias = up(s.bias);
  t.cst = up(s.cst);
  t.scale = up(s.scale);
  t.shift = up(s.shift);
}

}  // namespace

void PassRunner::launch_plain(size_t i) {
  const Step &x = st[i];
  const DeviceStep &d = dm.steps[i];
  const PlainTables &t = d.plain;
  switch (x.kind) {
    // (a window Dense, rep > 1: its [rows, rep, K] buffer is the [rows * rep, K] matrix; Dense with an epilogue: launch_fused)
    case StepKind::Dense: kern::dense(stream, buf(x.in0), t.W, t.bias, buf(x.out), nr * x.rep, int(x.K), int(x.M), act_of(x), 0, in_colmajor && x.in0 == 0); break;
    case StepKind::Conv2d: kern::conv2d(stream, buf(x.in0), t.W, t.bias, buf(x.out), nr, conv_geom(x), act_of(x), cq(x.in0), cq(x.out)); break;
    case StepKind::AffineChannel: kern::affine_channel(stream, buf(x.in0), t.scale, t.shift, buf(x.out), nr, x.C, x.S, act_of(x), cq(x.in0)); break;
    case StepKind::BinaryConst: kern::binary_const(stream, buf(x.in0), t.cst, buf(x.out), nr, p.buf_per_row[size_t(x.out)], x.bop, x.const_left, act_of(x)); break;
    case StepKind::LayerNorm:
      if (!kern::layernorm(stream, buf(x.in0), t.scale, t.shift, buf(x.out), nr * x.rep, int(x.K), x.ln_eps))
        throw InferaError::onnx("LayerNorm kernel launch failed: '" + x.origin + "' is beyond the kernel's caps");
      break;
    case StepKind::RmsNorm:
      if (!kern::rmsnorm(stream, buf(x.in0), t.scale, buf(x.out), nr * x.rep, int(x.K), x.ln_eps))
        throw InferaError::onnx("RmsNorm kernel launch failed: '" + x.origin + "' is beyond the kernel's caps");
      break;
    case StepKind::Attention:
      if (!kern::attention(stream, buf(x.in0), buf(x.in1), buf(x.in2), t.cst, buf(x.out), nr, int(x.attn_T), int(x.attn_heads), int(x.attn_dh), x.attn_ld,
                           x.attn_off, x.attn_scale, x.in3 >= 0 ? buf(x.in3) : nullptr, x.in3 >= 0 ? p.buf_per_row[size_t(x.in3)] : 0, int(x.rm_off), x.rm_cmp,
                           x.rm_fill, x.rm_mode, x.rm_excl, x.rm_int, int(x.attn_Tk), int(x.attn_kv_heads), x.attn_causal))
        throw InferaError::onnx("attention kernel launch failed: '" + x.origin + "' is beyond the kernel's caps");
      break;
    // the other families: their pairs above
    case StepKind::QDense: launch_qdense(*this, i, d.quant); break;
    case StepKind::QConv2d: launch_qconv(*this, x, d.quant); break;
    case StepKind::HDense: launch_hdense(*this, i, d.half); break;
    case StepKind::TreeEnsemble: launch_tree_walk(*this, x, d.tree_walk); break;
    case StepKind::TreeReduce: launch_tree_reduce(*this, x, d.tree_reduce); break;
    case StepKind::SvmKernel: launch_svm_kernel(*this, x, d.svm_kernel); break;
    case StepKind::SvmReduce: launch_svm_reduce(*this, x, d.svm_reduce); break;
    case StepKind::Nearest: launch_nearest(*this, x, d.nearest); break;
    case StepKind::NearestVote: launch_nearest_vote(*this, x, d.nearest_vote); break;
    case StepKind::Prep: launch_prep(*this, x, d.prep); break;
    case StepKind::Recurrent: launch_rnn(*this, x, d.rnn); break;
    case StepKind::ConvTranspose2d: launch_convt(*this, i, d.convt); break;
    case StepKind::Resize2d: launch_resize(*this, x, d.resize); break;
    case StepKind::SpatialNorm: launch_spatialnorm(*this, x, d.spatialnorm); break;
    case StepKind::SpatialStats: launch_spatialstats(*this, x); break;
    case StepKind::Tokens: launch_tokens(*this, x, d.tokens); break;
    case StepKind::ChannelNorm: launch_channelnorm(*this, x, d.channelnorm); break;
    case StepKind::Embed: launch_embed(*this, x, d.embed); break;
    case StepKind::Interact: launch_interact(*this, x, d.interact); break;
    case StepKind::Rotary: launch_rotary(*this, x, d.rotary); break;
    case StepKind::PixelShuffle: launch_pixelshuffle(*this, x); break;
    // the steps without tables
    case StepKind::Unary: kern::unary(stream, buf(x.in0), buf(x.out), nr * p.buf_per_row[size_t(x.out)], act_of(x)); break;
    case StepKind::BinaryAct:
      if (x.K > 0) kern::binary_rowscalar(stream, buf(x.in0), buf(x.in1), buf(x.out), nr * x.rep, x.K, x.bop, x.const_left, act_of(x));
      else if (x.S > 1) kern::binary_gate(stream, buf(x.in0), buf(x.in1), buf(x.out), nr, x.C, x.S, x.bop, act_of(x), cq(x.in0));
      else kern::binary_act(stream, buf(x.in0), buf(x.in1), buf(x.out), nr * p.buf_per_row[size_t(x.out)], x.bop, act_of(x));
      break;
    case StepKind::Softmax: kern::softmax(stream, buf(x.in0), buf(x.out), nr, x.sm_outer, x.sm_len, x.sm_inner, x.sm_norm ? 1 + x.sm_norm : int(x.log_softmax)); break;
    case StepKind::Pool2d:
      kern::pool2d(stream, buf(x.in0), buf(x.out), nr, int(x.C), int(x.H), int(x.Wd), int(x.OH), int(x.OW), int(x.kh), int(x.kw), int(x.sh), int(x.sw),
                   int(x.pt), int(x.pl), int(x.dh), int(x.dw), x.is_max, x.count_pad, cq(x.in0));
      break;
    case StepKind::GlobalAvgPool: kern::global_avgpool(stream, buf(x.in0), buf(x.out), nr, int(x.C), int(x.S), cq(x.in0), x.is_max); break;
    case StepKind::CopyCols:
      kern::copy_cols(stream, buf(x.in0), buf(x.out), nr, p.buf_per_row[size_t(x.in0)], p.buf_per_row[size_t(x.in0)], 0, p.buf_per_row[size_t(x.out)], x.col_off);
      break;
    case StepKind::PadCols: kern::pad_cols(stream, buf(x.in0), buf(x.out), nr * x.rep, x.K, x.M); break;
    case StepKind::LRN:
      kern::lrn(stream, buf(x.in0), buf(x.out), nr, int(x.C), int(x.S), int(x.lrn_size), x.lrn_alpha, x.lrn_beta, x.lrn_bias, cq(x.in0));
      break;
    case StepKind::ChannelShuffle: kern::channel_shuffle(stream, buf(x.in0), buf(x.out), nr, int(x.C), int(x.S), int(x.groups), cq(x.in0)); break;
    case StepKind::SliceCols: kern::copy_cols(stream, buf(x.in0), buf(x.out), nr, x.K, p.buf_per_row[size_t(x.in0)], x.col_off, x.K, 0); break;
    case StepKind::ArgMax: kern::argmax_rows(stream, buf(x.in0), buf(x.out), nr, x.K); break;
    case StepKind::MeanTime:
      if (x.in3 >= 0)
        kern::mean_time_masked(stream, buf(x.in0), buf(x.out), nr, int(x.rep), int(x.K), buf(x.in3), p.buf_per_row[size_t(x.in3)], int(x.rm_off), x.rm_cmp, x.rm_int,
                               x.rm_clip);
      else kern::mean_time(stream, buf(x.in0), buf(x.out), nr, int(x.rep), int(x.K));
      break;
    case StepKind::FakeQuant:
      kern::fake_quant(stream, buf(x.in0), buf(x.out), nr * p.buf_per_row[size_t(x.out)], x.qx.scale, x.qx.zp, x.qx.qmin(), x.qx.qmax());
      break;
    case StepKind::RowReduce: kern::row_reduce(stream, buf(x.in0), buf(x.out), nr * x.rep, int(x.K), x.out_mode); break;
    case StepKind::ArgMin: kern::argmin_rows(stream, buf(x.in0), buf(x.out), nr, x.K); break;
    case StepKind::TopK: kern::topk_rows(stream, buf(x.in0), buf(x.out), nr, int(x.K), int(x.M), x.is_max, x.out_mode == 1); break;
    case StepKind::NearestReduce: kern::nearest_reduce(stream, buf(x.in0), buf(x.out), nr, int(x.nearest->slices), int(x.M), x.out_mode); break;
    case StepKind::RoundHalf: kern::round_half(stream, buf(x.in0), buf(x.out), nr * p.buf_per_row[size_t(x.out)]); break;
  }
}

void upload_step(const Upload &up, size_t i) {
  const Step &s = up.m.plan.steps[i];
  DeviceStep &d = up.dm.steps[i];
  switch (up.m.exec[i]) {
    case ExecKind::Skipped: return;
    case ExecKind::Mlp3Head: return upload_mlp3(up, i);
    case ExecKind::ChainHead: return upload_chain(up, i);
    case ExecKind::ConvTiled: return upload_conv_tiled(up, i, d.plain);
    case ExecKind::DenseTiled: return upload_dense_tiled(s, d.plain, up);
    case ExecKind::ConvPatch: return upload_conv_patch(up, i, d.plain);
    case ExecKind::ConvDepthwise: return upload_conv_depthwise(s, d.plain, up);
    default: break;
  }
  switch (s.kind) {
    case StepKind::Dense: case StepKind::Conv2d: case StepKind::AffineChannel: case StepKind::BinaryConst: case StepKind::LayerNorm:
    case StepKind::Attention: case StepKind::RmsNorm: return upload_plain(s, d.plain, up);
    case StepKind::QDense: return upload_qdense(s, d.quant, up);
    case StepKind::QConv2d: return upload_qconv(s, d.quant, up);
    case StepKind::HDense: return upload_hdense(s, d.half, up);
    case StepKind::TreeEnsemble: return upload_tree_walk(s, d.tree_walk, up);
    case StepKind::TreeReduce: return upload_tree_reduce(s, d.tree_reduce, up);
    case StepKind::SvmKernel: return upload_svm_kernel(s, d.svm_kernel, up);
    case StepKind::SvmReduce: return upload_svm_reduce(s, d.svm_reduce, up);
    case StepKind::Nearest: return upload_nearest(s, d.nearest, up);
    case StepKind::NearestVote: return upload_nearest_vote(s, d.nearest_vote, up);
    case StepKind::Prep: return upload_prep(s, d.prep, up);
    case StepKind::Recurrent: return upload_rnn(s, d.rnn, up);
    case StepKind::ConvTranspose2d: return upload_convt(up, i, d.convt);
    case StepKind::Resize2d: return upload_resize(s, d.resize, up);
    case StepKind::SpatialNorm: return upload_spatialnorm(s, d.spatialnorm, up);
    case StepKind::Tokens: return upload_tokens(s, d.tokens, up);
    case StepKind::ChannelNorm: return upload_channelnorm(s, d.channelnorm, up);
    case StepKind::Embed: return upload_embed(s, d.embed, up);
    case StepKind::Interact: return upload_interact(s, d.interact, up);
    case StepKind::Rotary: return upload_rotary(s, d.rotary, up);
    case StepKind::PixelShuffle: return;  // (a copy by index arithmetic: no tables)
    default: return;  // (no tables)
  }
}

bool PassRunner::launch_fused(size_t i, size_t *skip) {
  const Step &x = st[i];
  const PlainTables &t = dm.steps[i].plain;
  const bool cm = in_colmajor && x.in0 == 0;  // this step reads the caller's column-major chunk
  switch (m.exec[i]) {
    case ExecKind::Skipped: return true;
    case ExecKind::Mlp3Head: launch_mlp3(*this, i, cm); return true;
    case ExecKind::ChainHead: launch_chain(*this, i, cm); return true;
    case ExecKind::DenseArgMax:
      if (cm || kern::dense_can_fuse_argmax(buf(x.in0), int(x.K), int(x.M))) {  // (both column-major kernels have the epilogue)
        kern::dense(stream, buf(x.in0), t.W, t.bias, buf(st[i + 1].out), nr, int(x.K), int(x.M), act_of(x), 3, cm);
        *skip = 1;  // the ArgMax step is done
        return true;
      }
      return false;  // as two kernels
    case ExecKind::DenseSoftmax:
      kern::dense(stream, buf(x.in0), t.W, t.bias, buf(st[i + 1].out), nr, int(x.K), int(x.M), act_of(x), st[i + 1].log_softmax ? 2 : 1, cm);
      return true;
    case ExecKind::ConvTiled: launch_conv_tiled(*this, i, t); return true;
    case ExecKind::DenseTiled: launch_dense_tiled(*this, x, t); return true;
    case ExecKind::ConvDepthwise: launch_conv_depthwise(*this, x, t); return true;
    case ExecKind::ConvPatch: launch_conv_patch(*this, i, t); return true;
    default: return false;
  }
}

}  // namespace rt
}  // namespace infera_hip
