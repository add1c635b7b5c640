// plan.cpp -- what a Plan says about itself: its work per row and the JSON infera_hip_get_plan reports.
#include <cmath>
#include <iomanip>
#include <sstream>

#include "attention.hpp"
#include "channelnorm.hpp"
#include "common.hpp"
#include "deconv.hpp"
#include "embed.hpp"
#include "interact.hpp"
#include "spatialnorm.hpp"
#include "tokens.hpp"
#include "nearest.hpp"
#include "pixelshuffle.hpp"
#include "plan.hpp"
#include "prep.hpp"
#include "recurrent.hpp"
#include "svm.hpp"
#include "trees.hpp"

namespace infera_hip {

double Plan::flops_per_row() const {
  double f = 0;
  for (const auto &s : steps) {
    if (s.kind == StepKind::Dense || s.kind == StepKind::QDense || s.kind == StepKind::HDense) f += 2.0 * double(s.rep) * double(s.K) * double(s.M);
    else if (s.kind == StepKind::Attention) f += 4.0 * double(s.attn_T) * double(s.attn_Tk > 0 ? s.attn_Tk : s.attn_T) * double(s.attn_heads * s.attn_dh);  // (an upper bound under attn_causal, as for padded rows)
    else if (s.kind == StepKind::Conv2d || s.kind == StepKind::QConv2d) f += 2.0 * double(s.K) * double(s.Mo) * double(s.OH) * double(s.OW);
    else if (s.kind == StepKind::ConvTranspose2d) f += 2.0 * double(s.K) * double(s.Mo) * double(s.H) * double(s.Wd);  // (C/g) kh kw taps per input pixel and output channel
    else if (s.kind == StepKind::SvmKernel) f += 2.0 * double(s.svm->n_sv) * double(s.svm->F + s.svm->Q);  // X . S^T, then the coefficients
    else if (s.kind == StepKind::Nearest) f += 2.0 * double(s.nearest->F) * double(s.nearest->M);
    else if (s.kind == StepKind::NearestVote) f += 2.0 * double(s.M);  // a weight and an add per neighbour
    else if (s.kind == StepKind::Interact) f += s.interact->mode == kInteractDot ? 2.0 * double(s.interact->k * s.interact->k * s.interact->d) : 4.0 * double(s.interact->k * s.interact->d);
    else if (s.kind == StepKind::Rotary) f += 3.0 * double(s.attn_T * s.attn_heads * s.rot_rd);  // two products and a sum per rotated column
    else if (s.kind == StepKind::Recurrent) f += 2.0 * double(s.rnn->T * s.rnn->D * s.rnn->G * s.rnn->H) * double(s.rnn->F + s.rnn->H);
  }
  return f;
}

std::string Plan::describe_json() const {
  static const char *kinds[] = {"Dense", "Unary", "AffineChannel", "BinaryConst", "BinaryAct", "Softmax", "Conv2d", "Pool2d", "GlobalAvgPool", "CopyCols", "ArgMax", "SliceCols", "PadCols", "LRN", "ChannelShuffle", "TreeEnsemble", "TreeReduce", "SvmKernel", "SvmReduce", "Prep", "Recurrent", "LayerNorm", "Attention", "MeanTime", "FakeQuant", "QDense", "QConv2d", "RoundHalf", "HDense", "RowReduce", "ArgMin", "TopK", "Nearest", "NearestReduce", "ConvTranspose2d", "Resize2d", "SpatialNorm", "SpatialStats", "Tokens", "ChannelNorm", "Embed", "Interact", "RmsNorm", "Rotary", "PixelShuffle", "NearestVote"};
  static const char *acts[] = {"", "Relu", "Sigmoid", "Tanh", "LeakyRelu", "Clip", "Exp", "Log", "Sqrt", "Neg", "Abs", "Elu", "Selu", "Softplus",
                               "HardSigmoid", "HardSwish", "Erf", "Gelu", "Reciprocal", "Floor", "Ceil", "Softsign", "Trunc", "Round", "Swish"};
  std::ostringstream o;
  o << "{\"input_shape\":" << json_int_array(input_shape) << ",\"output_shape\":" << json_int_array(output_shape)
    << ",\"flops_per_row\":" << (long long)flops_per_row();
  if (!input_declared_type.empty()) o << ",\"input_type\":" << json_str(input_declared_type);
  if (output_declared_type == "float16") o << ",\"output_type\":" << json_str(output_declared_type);  // (integer outputs: infera_get_model_info says so)
  o << ",\"steps\":[";
  for (size_t i = 0; i < steps.size(); i++) {
    const Step &s = steps[i];
    if (i) o << ",";
    o << "{\"kind\":\"" << kinds[int(s.kind)] << "\",\"in\":" << s.in0 << ",\"out\":" << s.out;
    if (s.in1 >= 0) o << ",\"in1\":" << s.in1;
    if (s.in2 >= 0) o << ",\"in2\":" << s.in2;
    if (s.kind == StepKind::Dense) o << ",\"K\":" << s.K << ",\"M\":" << s.M << ",\"bias\":" << (s.bias.empty() ? "false" : "true");
    if (s.kind == StepKind::Dense && s.rep > 1) o << ",\"T\":" << s.rep;
    auto qtype = [](const Quant &q) { return !q.on ? "f32" : q.is_signed ? "int8" : "uint8"; };
    if (s.kind == StepKind::FakeQuant) o << ",\"type\":\"" << qtype(s.qx) << "\",\"scale\":" << double(s.qx.scale) << ",\"zero_point\":" << s.qx.zp;
    if (s.kind == StepKind::QDense || s.kind == StepKind::QConv2d) {
      o << ",\"K\":" << s.K << ",\"M\":" << s.M << ",\"bias\":\"" << (!s.q_bias.empty() ? "int32" : !s.bias.empty() ? "f32" : "none") << "\",\"x_type\":\"" << qtype(s.qx)
        << "\",\"w_type\":\"" << (s.q_w_signed ? "int8" : "uint8") << "\",\"y_type\":\"" << qtype(s.qy) << "\",\"per_channel\":" << (s.q_per_channel ? "true" : "false");
      if (s.rep > 1) o << ",\"T\":" << s.rep;
      // what the parser read, for checks without a GPU: sums over the weights in their own type and over the int32 bias
      long long wsum = 0, whash = 0, bsum = 0;
      for (size_t k = 0; k < s.qW.size(); k++) {
        const long long w = s.qW[k] + (s.q_w_signed ? 0 : 128);
        wsum += w;
        whash += w * (long long)(k % 251 + 1);
      }
      for (int32_t b : s.q_bias) bsum += b;
      o << ",\"w_sum\":" << wsum << ",\"w_hash\":" << whash << ",\"bias_sum\":" << bsum << ",\"x_zero_point\":" << s.qx.zp;
    }
    if (s.kind == StepKind::HDense) {
      static const char *modes[] = {"none", "gemm", "matmul_add"};
      o << ",\"K\":" << s.K << ",\"M\":" << s.M << ",\"bias\":\"" << modes[s.h_bias_mode] << "\"";
      if (s.rep > 1) o << ",\"T\":" << s.rep;
      long long wsum = 0, whash = 0, bsum = 0;  // over the 16-bit patterns the parser read
      for (size_t k = 0; k < s.hW.size(); k++) {
        wsum += s.hW[k];
        whash += (long long)(s.hW[k]) * (long long)(k % 251 + 1);
      }
      for (uint16_t b : s.h_bias) bsum += b;
      o << ",\"w_sum\":" << wsum << ",\"w_hash\":" << whash << ",\"bias_sum\":" << bsum;
    }
    if (s.kind == StepKind::LayerNorm) o << ",\"E\":" << s.K << ",\"T\":" << s.rep << ",\"epsilon\":" << double(s.ln_eps) << ",\"bias\":" << (s.shift.empty() ? "false" : "true");
    if (s.kind == StepKind::RmsNorm) o << ",\"E\":" << s.K << ",\"T\":" << s.rep << ",\"eps\":" << double(s.ln_eps);
    if (s.kind == StepKind::MeanTime) o << ",\"E\":" << s.K << ",\"T\":" << s.rep;
    if (s.kind == StepKind::Rotary) {  // the tables as one hash over their f32 bit patterns: equal spellings give equal plans
      uint64_t h = 1469598103934665603ull;
      for (const auto *v : {&s.scale, &s.shift})
        for (float f : *v) {
          uint32_t b;
          std::memcpy(&b, &f, sizeof b);
          h = (h ^ b) * 1099511628211ull;
        }
      o << ",\"T\":" << s.attn_T << ",\"heads\":" << s.attn_heads << ",\"dh\":" << s.attn_dh << ",\"rd\":" << s.rot_rd << ",\"interleaved\":" << (s.rot_interleaved ? "true" : "false")
        << ",\"positions\":\"" << (s.rot_const_pos ? "constant" : "arange") << "\",\"ld\":" << s.attn_ld[0] << ",\"off\":" << s.attn_off[0] << ",\"form\":\""
        << (rotary_vec4(s.attn_ld[0], s.attn_off[0], s.attn_dh, s.rot_rd, s.rot_interleaved) ? "vec4" : "scalar") << "\",\"tables_hash\":" << (h >> 11);
    }
    auto json_f32 = [](float f) { return std::isnan(f) ? std::string("NaN") : std::isinf(f) ? std::string(f < 0 ? "-Infinity" : "Infinity") : ([&] { std::ostringstream q; q << std::setprecision(9) << double(f); return q.str(); })(); };
    if (s.kind == StepKind::MeanTime && s.in3 >= 0)
      o << ",\"row_mask\":{\"src_col\":" << s.rm_off << ",\"cmp\":" << json_f32(s.rm_cmp) << ",\"clip\":" << json_f32(s.rm_clip) << "}";
    if (s.kind == StepKind::RowReduce) {
      static const char *ops[] = {"Sum", "Mean", "Max", "Min", "Prod", "L1", "L2", "SumSquare", "LogSum", "LogSumExp"};
      o << ",\"op\":\"" << ops[s.out_mode] << "\",\"E\":" << s.K << ",\"T\":" << s.rep;
    }
    if (s.kind == StepKind::ArgMin) o << ",\"K\":" << s.K;
    if (s.kind == StepKind::TopK) o << ",\"M\":" << s.K << ",\"k\":" << s.M << ",\"largest\":" << (s.is_max ? "true" : "false") << ",\"output\":\"" << (s.out_mode ? "indices" : "values") << "\"";
    if (s.kind == StepKind::BinaryAct && s.K > 0) o << ",\"row_scalar\":\"" << (s.const_left ? "left" : "right") << "\",\"E\":" << s.K << ",\"T\":" << s.rep;
    if (s.kind == StepKind::Nearest || s.kind == StepKind::NearestReduce) {
      static const char *modes[] = {"lists", "d2", "sqrt_d2", "label", "indices", "values", "sqrt_values"};
      const NearestPack &q = *s.nearest;
      o << ",\"nearest\":{\"F\":" << q.F << ",\"M\":" << q.M << ",\"k\":" << s.M << ",\"outputs\":\"" << modes[s.out_mode] << "\",\"slices\":" << q.slices
        << ",\"slice_tile\":" << json_int_array(std::vector<int64_t>(q.slice_tile.begin(), q.slice_tile.end())) << ",\"spelling\":\"" << q.spelling << "\",\"centred\":true}";
    }
    if (s.kind == StepKind::NearestVote) {
      static const char *outs[] = {"label", "probabilities", "value"};
      o << ",\"k\":" << s.M << ",\"classes\":" << s.vote->classes << ",\"weights\":\"" << (s.vote->weighted ? "distance" : "uniform") << "\",\"outputs\":\"" << outs[s.out_mode]
        << "\",\"rooted\":" << (s.vote->rooted ? "true" : "false") << ",\"M\":" << s.nearest->M << ",\"slices\":" << s.nearest->slices;
      if (s.vote->weighted) o << ",\"eps\":" << json_f32(s.vote->eps);
    }
    if (s.kind == StepKind::Attention)
      o << ",\"T\":" << s.attn_T << ",\"heads\":" << s.attn_heads << ",\"dh\":" << s.attn_dh << ",\"scale\":" << double(s.attn_scale) << ",\"mask\":" << (s.cst.empty() ? "false" : "true")
        << ",\"packed_qkv\":" << (s.in0 == s.in1 && s.in1 == s.in2 ? "true" : "false");
    if (s.kind == StepKind::Attention && s.attn_Tk > 0 && s.attn_Tk != s.attn_T) o << ",\"Tk\":" << s.attn_Tk;
    if (s.kind == StepKind::Attention && s.attn_kv_heads > 0 && s.attn_kv_heads != s.attn_heads) o << ",\"kv_heads\":" << s.attn_kv_heads;
    if (s.kind == StepKind::Attention && s.attn_causal) o << ",\"causal\":true";
    if (s.kind == StepKind::Attention && s.in3 >= 0)
      o << ",\"row_mask\":{\"src_col\":" << s.rm_off << ",\"cmp\":" << json_f32(s.rm_cmp) << ",\"fill\":" << json_f32(s.rm_fill) << ",\"mode\":\""
        << (s.rm_mode == kRowMaskAdd ? "add" : "replace") << "\",\"excluding\":" << (s.rm_excl ? "true" : "false") << "}";
    if (s.kind == StepKind::Conv2d) o << ",\"C\":" << s.C << ",\"M\":" << s.Mo << ",\"k\":[" << s.kh << "," << s.kw << "],\"out_hw\":[" << s.OH << "," << s.OW << "]";
    if (s.kind == StepKind::ConvTranspose2d) {
      const DeconvPack &q = *s.deconv;
      o << ",\"C\":" << s.C << ",\"M\":" << s.Mo << ",\"group\":" << s.groups << ",\"k\":[" << s.kh << "," << s.kw << "],\"strides\":[" << s.sh << "," << s.sw << "],\"pads\":[" << s.pt
        << "," << s.pl << "," << s.pb << "," << s.pr << "],\"dilations\":[" << s.dh << "," << s.dw << "],\"output_padding\":[" << q.out_pad_h << "," << q.out_pad_w
        << "],\"in_hw\":[" << s.H << "," << s.Wd << "],\"out_hw\":[" << s.OH << "," << s.OW << "],\"bias\":" << (s.bias.empty() ? "false" : "true") << ",\"phases\":[";
      for (size_t a = 0; a < q.hphase.size(); a++)
        for (size_t b = 0; b < q.wphase.size(); b++) {
          const ConvTAxisPhase &hp = q.hphase[a], &wp = q.wphase[b];
          o << (a + b ? "," : "") << "{\"phase\":[" << a << "," << b << "],\"first\":[" << hp.out0 << "," << wp.out0 << "],\"pixels\":[" << hp.count << "," << wp.count << "],\"taps\":[";
          for (size_t i = 0; i < hp.tap.size(); i++)
            for (size_t j = 0; j < wp.tap.size(); j++) o << (i + j ? "," : "") << "[" << hp.tap[i] << "," << wp.tap[j] << "]";
          o << "],\"source_offsets\":[";  // per tap: the input pixel of the phase's pixel (j, i) is (j, i) + this
          for (size_t i = 0; i < hp.tap.size(); i++)
            for (size_t j = 0; j < wp.tap.size(); j++) o << (i + j ? "," : "") << "[" << hp.q[i] << "," << wp.q[j] << "]";
          o << "]}";
        }
      o << "]";
    }
    if (s.kind == StepKind::Resize2d)
      o << ",\"C\":" << s.C << ",\"mode\":\"" << (s.deconv->linear ? "linear" : "nearest") << "\",\"coordinate_transformation_mode\":\"" << s.deconv->coord_mode << "\""
        << (s.deconv->linear ? std::string() : ",\"nearest_mode\":\"" + s.deconv->nearest_mode + "\"") << ",\"in_hw\":[" << s.H << "," << s.Wd << "],\"out_hw\":[" << s.OH << "," << s.OW << "]";
    if (s.kind == StepKind::PixelShuffle)  // (a copy: no flops; every element is read once and written once)
      o << ",\"form\":\"" << pixelshuffle_form_name(s.ps_to_space, s.ps_channel_major) << "\",\"block\":" << s.ps_block << ",\"C\":" << s.C << ",\"M\":" << s.Mo << ",\"in_hw\":[" << s.H << "," << s.Wd
        << "],\"out_hw\":[" << s.OH << "," << s.OW << "],\"bytes_per_row\":" << 8 * s.C * s.H * s.Wd;
    if (s.kind == StepKind::SpatialNorm || s.kind == StepKind::SpatialStats)
      o << ",\"C\":" << s.C << ",\"groups\":" << s.groups << ",\"E\":" << (s.C / s.groups) * s.S << ",\"hw\":[" << (s.H > 0 ? s.H : 1) << "," << (s.H > 0 ? s.Wd : s.S)
        << "],\"epsilon\":" << double(s.ln_eps);
    if (s.kind == StepKind::SpatialNorm) {  // gamma and beta as their f32 bit patterns: what the lowering folded, for checks without a GPU
      auto bits = [](const std::vector<float> &v) {
        std::vector<uint32_t> b(v.size());
        if (!v.empty()) std::memcpy(b.data(), v.data(), v.size() * sizeof(float));
        return json_int_array(b);
      };
      o << ",\"scale_bits\":" << bits(s.scale) << ",\"shift_bits\":" << bits(s.shift);
    }
    if (s.kind == StepKind::ChannelNorm) {  // gamma and beta as their f32 bit patterns, as for SpatialNorm
      auto bits = [](const std::vector<float> &v) {
        std::vector<uint32_t> b(v.size());
        if (!v.empty()) std::memcpy(b.data(), v.data(), v.size() * sizeof(float));
        return json_int_array(b);
      };
      o << ",\"C\":" << s.C << ",\"hw\":[" << s.H << "," << s.Wd << "],\"epsilon\":" << double(s.ln_eps) << ",\"scale_bits\":" << bits(s.scale) << ",\"shift_bits\":" << bits(s.shift);
    }
    if (s.kind == StepKind::Tokens) {  // the tables as one hash over their f32 bit patterns: equal spellings give equal plans
      uint64_t h = 1469598103934665603ull;
      for (const auto *v : {&s.prefix, &s.cst})
        for (float f : *v) {
          uint32_t b;
          std::memcpy(&b, &f, sizeof b);
          h = (h ^ b) * 1099511628211ull;
        }
      o << ",\"C\":" << s.C << ",\"S\":" << s.S << ",\"prefix\":" << s.rep - s.S << ",\"pos\":" << (s.cst.empty() ? "false" : "true") << ",\"T\":" << s.rep << ",\"E\":" << s.K
        << ",\"tables_hash\":" << (h >> 11);
    }
    if (s.kind == StepKind::Embed) {
      const EmbedPack &q = *s.embed;
      o << ",\"W\":" << q.W << ",\"out_cols\":" << q.F << ",\"window\":";
      if (q.win_k > 0) o << "[" << q.win_k << "," << q.win_d << "]";
      else o << "null";
      o << ",\"tables\":" << q.n_tables << ",\"rows_per_tile\":" << q.R << ",\"staged\":" << (q.staged ? "true" : "false") << ",\"bytes_per_row\":" << q.bytes_per_row()
        << ",\"pieces\":[";
      for (size_t k = 0; k < q.pieces.size(); k++) {
        const EmbedPiece &e = q.pieces[k];
        o << (k ? "," : "");
        if (e.table >= 0)
          o << "{\"table\":" << e.table << ",\"src\":" << e.src << ",\"V\":" << e.V << ",\"d\":" << e.d << ",\"offset\":" << e.offset << ",\"out\":" << e.out << "}";
        else if (e.table == -2)
          o << "{\"gap\":" << e.d << ",\"out\":" << e.out << "}";
        else
          o << "{\"copy\":" << e.d << ",\"src\":" << e.src << ",\"out\":" << e.out << "}";
      }
      o << "]";
    }
    if (s.kind == StepKind::Interact) {
      const InteractPack &q = *s.interact;
      o << ",\"mode\":\"" << (q.mode == kInteractDot ? "dot" : "fm") << "\",\"k\":" << q.k << ",\"d\":" << q.d << ",\"P\":" << q.P << ",\"out_cols\":" << q.F
        << ",\"bytes_per_row\":" << q.bytes_per_row();
      if (q.mode == kInteractDot) {
        o << ",\"whole\":" << (q.whole ? "true" : "false") << ",\"tile\":" << q.tile << ",\"selection_out\":" << q.sel_out << ",\"selection\":" << json_int_array(q.sel) << ",\"pass_through\":[";
        for (size_t k = 0; k < q.passes.size(); k++)
          o << (k ? "," : "") << "{\"src\":" << q.passes[k].src << ",\"len\":" << q.passes[k].len << ",\"out\":" << q.passes[k].out << "}";
        o << "]";
      } else {
        o << ",\"h\":";
        if (q.has_h) o << json_f32(q.h);
        else o << "null";
        o << ",\"sum_last\":" << (q.sum_last ? "true" : "false") << ",\"h_after_sum\":" << (q.h_after ? "true" : "false");
      }
    }
    if (s.kind == StepKind::QConv2d)
      o << ",\"C\":" << s.C << ",\"k\":[" << s.kh << "," << s.kw << "],\"strides\":[" << s.sh << "," << s.sw << "],\"pads\":[" << s.pt << "," << s.pl << "," << s.pb << "," << s.pr
        << "],\"dilations\":[" << s.dh << "," << s.dw << "],\"in_hw\":[" << s.H << "," << s.Wd << "],\"out_hw\":[" << s.OH << "," << s.OW << "]";
    if (s.kind == StepKind::TreeEnsemble || s.kind == StepKind::TreeReduce) {
      static const char *modes[] = {"scores", "label", "binary_scores", "binary_label"};
      const TreePack &t = *s.tree;
      o << ",\"E\":" << t.E << ",\"slices\":" << t.slices << ",\"output\":\"" << modes[s.out_mode] << "\"";
      if (s.kind == StepKind::TreeEnsemble)
        o << ",\"trees\":" << t.trees << ",\"nodes\":" << t.nodes << ",\"max_depth\":" << t.max_depth << ",\"walk_width\":" << t.W
          << ",\"aggregate\":\"" << (t.average ? "AVERAGE" : "SUM") << "\"";
    }
    if (s.kind == StepKind::SvmKernel || s.kind == StepKind::SvmReduce) {
      static const char *kernels[] = {"LINEAR", "POLY", "RBF", "SIGMOID"}, *modes[] = {"value", "one_class", "label", "decision", "probabilities"};
      const SvmPack &v = *s.svm;
      o << ",\"kernel\":\"" << kernels[v.kernel] << "\",\"support_vectors\":" << v.n_sv << ",\"F\":" << v.F << ",\"classes\":" << v.classes
        << ",\"slices\":" << v.slices << ",\"output\":\"" << modes[s.out_mode] << "\",\"probabilities\":" << (v.probabilities ? "true" : "false");
    }
    if (s.kind == StepKind::Prep)
      o << ",\"F_in\":" << s.prep->F_in << ",\"F\":" << s.prep->F << ",\"onehot_cols\":" << s.prep->onehot << ",\"lookup_cols\":" << s.prep->lookup
        << ",\"rows_per_tile\":" << s.prep->R << ",\"strict\":" << (s.prep->strict ? "true" : "false");
    if (s.kind == StepKind::Recurrent) {
      static const char *ops[] = {"LSTM", "GRU", "RNN"}, *modes[] = {"Y", "Y_h", "Y_c"};
      const RnnPack &r = *s.rnn;
      o << ",\"op\":\"" << ops[r.op] << "\",\"T\":" << r.T << ",\"F\":" << r.F << ",\"H\":" << r.H << ",\"D\":" << r.D << ",\"direction\":\""
        << (r.D == 2 ? "bidirectional" : r.reverse ? "reverse" : "forward") << "\",\"output\":\"" << modes[s.out_mode] << "\"";
      if (r.op == kRnnGru) o << ",\"linear_before_reset\":" << (r.lbr ? 1 : 0);
      if (r.op == kRnnPlain) o << ",\"activation\":\"" << (r.relu ? "Relu" : "Tanh") << "\"";
      if (s.in3 >= 0) o << ",\"seq_lens\":{\"src_col\":" << s.rm_off << "}";
    }
    if (s.act != Act::None) o << ",\"act\":\"" << acts[int(s.act)] << "\"";
    o << ",\"origin\":" << json_str(s.origin) << "}";
  }
  o << "]}";
  return o.str();
}

}  // namespace infera_hip
