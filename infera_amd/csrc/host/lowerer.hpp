// lowerer.hpp -- struct Lowerer, the ONNX graph -> Plan lowering (lowering.cpp), declared once so that its member functions can be defined
// per model family in lower_<family>.cpp.  Private to the lowering: only lowering.cpp and the lower_*.cpp files include it; the entry
// point is lower_model (plan.hpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "attention.hpp"
#include "common.hpp"
#include "interact.hpp"
#include "plan.hpp"  // Plan, Step, Quant; it forward-declares NearestPack (host/nearest.hpp), held here by pointer only
#include "prep.hpp"

namespace infera_hip {

// (hidden: none of this is part of the library's dynamic symbol table)
namespace lowering __attribute__((visibility("hidden"))) {

using onnx::NodeDef;
using onnx::TensorData;

// A value inside a preprocessing region (host/prep.hpp): not computed yet -- one column program per column over the rows of buffer
// `src`.  It becomes a buffer (one Prep step, a SliceCols, or the source itself) where something outside the region reads it.
struct PrepVal {
  int src = -1;
  std::vector<PrepCol> cols;
  std::vector<std::string> origin;  // the ONNX nodes absorbed so far
  void add_origin(const std::string &o) {
    if (std::find(origin.begin(), origin.end(), o) == origin.end()) origin.push_back(o);
  }
  // q's columns after these (q reads the same source)
  void append(const PrepVal &q) {
    cols.insert(cols.end(), q.cols.begin(), q.cols.end());
    for (const auto &o : q.origin) add_origin(o);
  }
};

struct NearestPending {
  std::shared_ptr<const NearestPack> pack;
  int in_buf = -1;
  int64_t rows = -1;  // the row extent of the input's shape
  bool rooted = false;
  std::string origin;
  std::map<int64_t, int> part_of_k;  // k -> the buffer of the best-k lists already emitted
};

struct Val {
  bool is_const = false;
  std::shared_ptr<const PrepVal> pv;  // set: a preprocessing-region value (buf = -1)
  std::shared_ptr<TensorData> c;
  int buf = -1;
  std::vector<int64_t> shape;  // activations: dim[ra] = -1 (symbolic rows) or fixed batch
  // row-axis tag: where the row axis stands in `shape`.  The buffer is always [rows, the other axes in the order of `shape`]; 0 for
  // everything but the time-major values around a recurrent layer ([T, rows, F], Y [T, D, rows, H], Y_h [D, rows, H])
  int ra = 0;
  // zero padding (top, left, bottom, right) a Pad node asked for and the consuming Conv still has to apply; `shape`
  // is the UNPADDED tensor that `buf` holds
  int64_t pend[4] = {0, 0, 0, 0};
  // set: the value is a QUANTISED activation (uint8 / int8 in the graph).  q_done: `buf` holds the dequantised values (q - zp) * s (a
  // QLinearMatMul's result); else `buf` is the f32 tensor a QuantizeLinear read and the rounding is still to be done by whoever reads this
  std::shared_ptr<const Quant> q;
  bool q_done = false;
  // an ACTIVATION the graph types float16: `buf` holds f32 values that are halves once the plan's RoundHalf steps
  // have run (insert_half_roundings).  A constant is half when its tensor says so (TensorData::elem)
  bool half = false;
  // set: the distances of the rows to a constant set (buf = -1), not computed yet -- whoever reads the value decides what the Nearest step
  // serves (a label, the best k, the matrix); `rooted`: this value is sqrt(d2)
  std::shared_ptr<struct NearestPending> nn;
  // set: a CHANNELS-LAST VIEW: `shape` is [N,H,W,C] and `buf` is the [N,C,H,W] tensor a step wrote, untouched -- what a
  // Transpose(0,2,3,1) of that tensor yields.  Only the operators lower_on_view lists read it
  bool cl = false;
  bool padded() const { return pend[0] || pend[1] || pend[2] || pend[3]; }
};

inline int64_t prod(const std::vector<int64_t> &v, size_t from = 0, size_t to = SIZE_MAX) {
  // Shapes come from a model file: a product that leaves int64 is an error, not a wrapped number.
  int64_t p = 1;
  for (size_t i = from; i < std::min(to, v.size()); i++)
    if (__builtin_mul_overflow(p, v[i], &p)) throw InferaError::onnx("tensor shape too large");
  return p;
}

// Largest activation row the planner accepts (elements): 2^31 floats = 8 GiB per table row is beyond anything the
// staging or scratch sizing could serve, and keeping per-row counts in 31 bits keeps rows*per_row inside int64.
constexpr int64_t kMaxPerRow = int64_t(1) << 31;

inline std::string shape_str(const std::vector<int64_t> &s) {
  std::string o = "[";
  for (size_t i = 0; i < s.size(); i++) o += (i ? "," : "") + std::to_string(s[i]);
  return o + "]";
}

[[noreturn]] inline void unsupported(const NodeDef &n, const std::string &why) {
  throw InferaError::onnx("node '" + (n.name.empty() ? n.op : n.name) + "' (" + n.op + "): " + why);
}

// "Op:name" (or "Op"): how a step's origin names a node
inline std::string node_label(const NodeDef &n) { return n.op + (n.name.empty() ? "" : ":" + n.name); }

inline Val const_val(std::shared_ptr<TensorData> t) {
  Val v;
  v.is_const = true;
  v.c = std::move(t);
  v.shape = v.c->dims;
  return v;
}
inline Val const_f32(std::vector<float> f, std::vector<int64_t> dims) {
  auto t = std::make_shared<TensorData>();
  t->dtype = onnx::kFloat;
  t->dims = std::move(dims);
  t->f32 = std::move(f);
  return const_val(std::move(t));
}
inline Val const_i64(std::vector<int64_t> i, std::vector<int64_t> dims) {
  auto t = std::make_shared<TensorData>();
  t->dtype = onnx::kInt64;
  t->dims = std::move(dims);
  t->i64 = std::move(i);
  return const_val(std::move(t));
}

// What the matchers that run before the walk (Lowerer::find_*) read of the graph: built once, for the served output, and never changed.
// Only live nodes are indexed.  (A live node's inputs have live producers and ONNX names are assigned once, so a lookup that starts at a
// live node finds what a map over all nodes would.)
struct GraphIndex {
  const onnx::Model &m;
  std::vector<char> live;  // node index -> it feeds the served output
  std::map<std::string, size_t> producer_of;
  std::map<std::string, std::vector<size_t>> consumers_of;  // live consumers of every value, one entry per input that reads it
  std::set<std::string> row_data;    // values that hold row data: computed from a graph input (Shape's result is not); everything else folds to a constant
  std::set<std::string> graph_outs;  // the names of all graph outputs, served or not

  GraphIndex(const onnx::Model &model, const std::string &served) : m(model), live(model.nodes.size(), 0) {
    const size_t N = m.nodes.size();
    {
      // Only one output is served (engine.rs:146-149): nodes that do not feed it are dead -- a second
      // output (e.g. the probabilities next to a label) must neither cost kernels nor block loading.
      std::map<std::string, size_t> any_producer;
      for (size_t i = 0; i < N; i++)
        for (const auto &o : m.nodes[i].outputs) any_producer[o] = i;
      std::vector<std::string> work{served};
      while (!work.empty()) {
        const std::string v = work.back();
        work.pop_back();
        auto it = any_producer.find(v);
        if (it == any_producer.end() || live[it->second]) continue;
        live[it->second] = 1;
        for (const auto &i : m.nodes[it->second].inputs) work.push_back(i);
      }
    }
    for (size_t i = 0; i < N; i++) {
      if (!live[i]) continue;
      for (const auto &o : m.nodes[i].outputs) producer_of[o] = i;
      for (const auto &in : m.nodes[i].inputs) consumers_of[in].push_back(i);
    }
    for (const auto &o : m.outputs) graph_outs.insert(o.name);
    for (const auto &v : m.inputs) row_data.insert(v.name);
    for (size_t i = 0; i < N; i++) {
      if (!live[i] || m.nodes[i].op == "Shape") continue;
      bool any = false;
      for (const auto &in : m.nodes[i].inputs) any = any || row_data.count(in);
      if (any)
        for (const auto &o : m.nodes[i].outputs) row_data.insert(o);
    }
  }

  // the node that computes `v` (null: a graph input, an initializer, or nothing)
  const NodeDef *producer(const std::string &v, size_t *idx = nullptr) const {
    auto pi = producer_of.find(v);
    if (pi == producer_of.end()) return nullptr;
    if (idx) *idx = pi->second;
    return &m.nodes[pi->second];
  }
  // the node that alone reads `v` (null: several readers, none, or a graph output); allow_repeat: it may read `v` twice, as in Mul(d, d)
  const NodeDef *sole_reader(const std::string &v, bool allow_repeat) const {
    auto it = consumers_of.find(v);
    if (it == consumers_of.end() || it->second.empty() || graph_outs.count(v)) return nullptr;
    if (!allow_repeat && it->second.size() != 1) return nullptr;
    for (size_t c : it->second)
      if (c != it->second[0]) return nullptr;
    return &m.nodes[it->second[0]];
  }
  static bool std_dom(const NodeDef &n) { return n.domain.empty() || n.domain == "ai.onnx"; }
  // A constant known before the walk: an initializer, or the result of a Constant node -- the tensor of its `value`, or the node
  // itself where the value stands in another attribute (value_int, value_float, value_ints).  Neither: `v` is no such constant.
  struct Const {
    std::shared_ptr<TensorData> t;
    const NodeDef *node = nullptr;
    explicit operator bool() const { return t || node; }
  };
  Const constant(const std::string &v) const {
    Const c;
    if (auto ci = m.initializers.find(v); ci != m.initializers.end()) {
      c.t = ci->second;
    } else if (const NodeDef *p = producer(v); p && p->op == "Constant") {
      if (auto *a = p->attr("value"); a && a->t) c.t = a->t;
      else c.node = p;
    }
    return c;
  }
};

struct Lowerer {
  const onnx::Model &m;
  Plan plan;
  std::map<std::string, Val> vals;
  std::map<std::string, int> uses;
  std::map<int, int> producer;  // buffer id -> index of the step that wrote it
  std::map<int, std::vector<std::string>> buf_names;  // value names that denote each buffer
  std::map<int, int> alias_edges;  // nodes folded away whose input AND output denote the buffer
  std::set<int> half_bufs;  // buffers written by float16-typed nodes: their steps' results are rounded to half (insert_half_roundings)
  bool cur_half = false;    // the node being lowered is float16-typed
  // INFERA_HDENSE=0 (read when a model is loaded): float16 MatMul / Gemm layers stay on the float path (Dense + RoundHalf) -- the
  // switch the bit-identity tests compare the HDense kernel against
  const bool hdense_enabled = ScheduleKnobs::read().hdense;
  // INFERA_NEAREST=0 (read when a model is loaded): distance sub-graphs lower operator by operator (RowReduce, Dense, BinaryAct ...), the
  // plan the bit-identity tests compare the Nearest kernel against
  const bool nearest_enabled = ScheduleKnobs::read().nearest;
  std::set<int> int_bufs;  // buffers whose f32 values are whole numbers by construction (ArgMax, integer Cast, label arithmetic)
  size_t out_index = 0;
  std::unique_ptr<const GraphIndex> graph;  // the graph as the served output sees it (run)

  // ---- Instance / Group norm, the channels-last view, Tokens, LayerNorm ----
  // The exporter's spelling of nn.GroupNorm below opset 18: Reshape(x, [0, G, -1]) -> InstanceNormalization(scale[G], B[G]) -> Reshape(back to
  // x's shape, a constant or the folded Shape(x)) [-> Mul(gamma [C,1,1])] [-> Add(beta)].  The chain is found structurally before the walk
  // (find_group_norms: operators and sole readers), anchored at the first Reshape; shapes and constants are checked when the walk reaches
  // the anchor (false: every node lowers by its own rule), and the nodes behind it emit nothing.
  struct GnMatch {
    size_t inorm = 0, back = 0;
  };
  std::map<size_t, GnMatch> gn_at;  // index of the first Reshape -> the chain behind it
  // ---- sub-pixel layers (lower_shuffle.cpp; INTEGRATION.md 2.6 "Sub-pixel layers") ----
  // Reshape(x, 6-D) -> Transpose(one of four perms) -> Reshape(4-D) with sole readers in between: DepthToSpace / SpaceToDepth spelled out.
  // Found structurally before the walk (find_pixel_shuffles), anchored at the LAST Reshape -- both targets are constants by then; the first
  // two nodes emit nothing.  Shapes are checked at the anchor (false: the three nodes lower by their own rules, as without the matcher)
  struct ShuffleMatch {
    size_t first = 0, transpose = 0;
    int form = 0;  // index into lower_shuffle.cpp's table of spellings
  };
  std::map<size_t, ShuffleMatch> shuffle_at;  // index of the last Reshape -> the two nodes in front of it
  int view_consts = 0;
  std::map<std::string, int64_t> expanded_lead;  // results of Expand over constants -> the leading entry of the target shape as the graph had it

  // ---- self-attention ----------------------------------------------------------------------------
  // The batch-first graph exporters write is matched structurally before the walk (find_attention: by operator, perm and which operands
  // are constants), anchored at the merge Reshape; the nodes inside emit nothing, and the anchor validates shapes and constants and emits
  // ONE Attention step (lower_attention).  A MatMul of two activations that starts no such pattern is rejected with the reason kept here.
  struct AttnScale {
    char op;  // '*' or '/'
    std::string cst;
  };
  // ---- rotary position embeddings (lower_rotary.cpp; INTEGRATION.md 2.6 "Rotary position embeddings") -------------------------------------
  // A rotary embedding on a head-major value [N, h, T, dh], recognised by structure before the walk (match_rotary) where an attention front
  // end walks an operand back to its head split: the RotaryEmbedding operator, or the rotate_half spelling Add(Mul(x, cos), Mul(Concat(Neg(x2),
  // x1), sin)) with x1, x2 the two halves of x's last axis (two Slices or one Split).  Its nodes emit nothing; lower_attention emits one Rotary
  // step per rotated operand in front of the Attention step (rotary_step: constants and shapes are checked there, refusals name `at`).
  struct RotaryMatch {
    const NodeDef *at = nullptr;   // the RotaryEmbedding node, or the Add that closes the spelling
    std::string x;                 // the value it rotates
    std::string cos, sin, pos;     // the constants' names (pos: position_ids or "")
    bool spelling = false;         // rotate_half: cos / sin are whole [T, dh] factor tables, the pairing is `half`
    std::vector<size_t> nodes;
  };
  struct AttnSide {
    std::string src, shape;   // the [N, T, E] value the head split reads (behind an absorbed Split / Slice: its input) and the Reshape's target
    const NodeDef *cut = nullptr;  // that Split / Slice on the last axis
    size_t cut_out = 0;
    std::shared_ptr<const RotaryMatch> rot;  // the rotary embedding between the head split and the attention (null: none)
  };
  // A row's own key mask (INTEGRATION.md 2.6 "Padded sequences"): T consecutive columns of the input buffer and a compare value, traced
  // back from where it meets the scores (or the masked mean) through Cast / Unsqueeze / Reshape / Expand / Equal / Not to a graph input
  struct RowMask {
    int64_t src0 = 0, k = 0;     // columns [src0, src0 + k) of the input buffer
    bool is_int = false;         // the graph sees them as integers: truncated toward zero before the comparison
    float cmp = 0.f;             // kept iff value != cmp
    int state = 0;               // the traced value: 0 the source's own values (kept iff != 0), 1 a bool true = masked, 2 a bool true = kept
    std::vector<int64_t> shape;  // of the traced value in front of any Expand; shape[0] = -1, the rows
    std::vector<size_t> nodes, aux;  // the nodes between the graph input and the value; aux: the Shape sub-graph that sizes an Expand
    float fill = 0.f;            // Attention: the negative constant of masked keys, and how it reaches the score (RowMaskMode)
    int mode = kRowMaskAdd;
    const NodeDef *at = nullptr;  // the Add / Where on the scores
  };
  struct AttnMatch {
    AttnSide side[3];  // Q, K, V
    std::vector<AttnScale> scales;
    std::string mask;
    std::shared_ptr<RowMask> rm;
    const NodeDef *qk = nullptr;
    std::vector<size_t> nodes;
    // the standard-domain Attention operator (lower_attention_op.cpp): `op` is the node (= qk: what refusals name); form3: Q, K, V are
    // [N, T, h dh] values and the node is its own anchor, else each comes through a head split and the anchor is the merge Reshape
    const NodeDef *op = nullptr;
    bool form3 = false;
  };
  std::map<size_t, AttnMatch> attn_at;            // anchor node index -> the pattern it closes
  std::vector<char> absorbed;                // nodes inside a recognised pattern (attention, or the decomposed LayerNorm): they emit nothing
  std::map<const NodeDef *, std::string> attn_fail;  // MatMul(activation, activation) nodes outside one: why
  struct MaskedMean {
    std::string x;  // the window [N, T, E]
    RowMask rm;
    float clip = 0.f;
    size_t mul = 0;
  };
  std::map<size_t, MaskedMean> mmean_at;  // the Div that closes a masked mean over time -> the pattern

  // ---- quantised and float16 graphs ----
  // the constant scale / zero point inputs (`si`, `zi`) of a quantisation node: one scale per tensor, or one per index of an axis
  struct QArgs {
    std::vector<float> scale;
    std::vector<int64_t> zp;
    int elem = onnx::kUint8;  // the quantised element type (the zero point's; uint8 without one)
  };
  std::map<std::string, const NodeDef *> quant_node;  // quantised value -> the node that made it

  // ---- per-row sequence lengths (INTEGRATION.md 2.6 "Padded windows") ----------------------------------------------------------------
  // Input 4 of LSTM / GRU / RNN, sequence_lens, traced back to ONE column of a graph input before the walk: an [N] integer input, an
  // [N, 1] one through Squeeze / Reshape([-1]) / Flatten, a column of a wider input picked by Slice / Gather(axis = 1), with or without
  // Cast (PyTorch: Cast(lengths, INT32)).  The tracing nodes emit nothing and the value may feed every layer of a stack; the steps read the
  // column from the input buffer (Step::in3, rm_off, rm_int).  A constant sequence_lens is left to pack_recurrent, which refuses it.
  struct SeqLens {
    int64_t col = 0;
    bool is_int = false;
    int node = 0;  // 1-based id in plan.prep_strict_nodes
  };
  std::map<size_t, SeqLens> seq_lens_at;  // recurrent node -> its lengths

  // ---- ai.onnx.ml preprocessing regions (host/prep.hpp).  A region is a connected set of Imputer / Scaler / Binarizer / OneHotEncoder /
  // LabelEncoder / FeatureVectorizer / ArrayFeatureExtractor (constant indices) / Cast / Reshape / Flatten / Squeeze / Concat / Identity
  // nodes and graph inputs that holds at least one thing nothing else serves: one of the five encoder nodes, a non-contiguous
  // ArrayFeatureExtractor or an integer graph input.  Graphs without one lower exactly as before.  Inside a region every value is a
  // list of column programs over one source buffer (PrepVal); where anything else reads a region value it becomes ONE Prep step.
  std::vector<char> region;                           // node index -> lowered as part of a region
  std::vector<std::shared_ptr<PrepTable>> prep_tables;  // LabelEncoder tables and strict one-hot category sets, by id
  int64_t prep_cats = 0, prep_keys = 0;                 // one-hot categories / LabelEncoder keys in all (caps)

  // ---- distance models: |x - c|^2 of each row against a constant set C [M, F] ----------------------------
  // Recognised before the walk (find_nearest) in the spellings exporters write,
  //   rs = ReduceSumSquare(X, axes = [1], keepdims = 1);  g = Gemm(X, C, alpha = -2 [, transB]) | Mul(MatMul(X, C^T), -2);
  //   D2 = Add(Add(rs, g), C2) | Add(rs, Add(g, C2))     (either operand order; C2[m] = |C[m]|^2 within rounding)
  // when no intermediate has another reader; the contrib operator CDist(X, C) is the same value in one node.  The nodes emit nothing: the
  // last one binds D2 to a pending value (Val::nn), and what reads it decides what the Nearest step serves -- ArgMin the label, TopK the
  // best k, Sqrt the rooted distances, anything else (the graph output included) the [rows, M] matrix.
  struct NearestMatch {
    std::string x, d2, spelling;
    std::shared_ptr<TensorData> c;
    bool c_fm = false;  // C is stored [F, M]
    std::vector<size_t> nodes;  // ascending; the last is the anchor
  };
  std::map<size_t, NearestMatch> nearest_at;  // anchor node index -> the pattern it closes
  // The k-NN vote (KNeighborsClassifier / KNeighborsRegressor; INTEGRATION.md 2.6 "The k-NN vote"): behind TopK(largest = 0) over such a
  // distance value, the neighbours' labels / targets looked up in a constant table (ArrayFeatureExtractor | Gather, [Reshape] [Cast]
  // [Squeeze]), the weights Reciprocal | Div(1, .) of Max(values, eps), and
  //   classifier: per class c, Equal(lab, c) -> Cast -> [Mul(., wei)] -> ReduceSum(axes = [1]) [-> Unsqueeze], joined by Concat(axis = 1)
  //               (or Concat(axis = 0) -> Transpose); closed by ArgMax (-> the class table lookup [-> Reshape / Cast]) or by
  //               Div(all, ReduceSum(all, axes = [1], keepdims = 1));
  //   regressor:  ReduceMean(lab, axes = [1]) | Div(ReduceSum(Mul(lab, wei)), ReduceSum(wei)) [-> Reshape([-1, 1])].
  // Found structurally before the walk (find_votes: operators, constants and sole readers), anchored at the closing node.  The nodes
  // inside emit nothing.  When the walk reaches the TopK and its input is a pending distance value, the vote is taken (vote_begin: Values
  // / Indices keep only their readers outside the pattern); otherwise the nodes are given back and lower by their own rules, as without
  // the matcher.  The anchor checks the constants and emits ONE NearestVote step on the best-k lists (lower_vote).
  struct VoteMatch {
    size_t topk = 0, anchor = 0, lookup = 0;
    size_t reshape = SIZE_MAX, clamp = SIZE_MAX, concat = SIZE_MAX, class_lookup = SIZE_MAX;  // nodes the checks name (SIZE_MAX: absent)
    int mode = 0;  // VoteOut
    bool weighted = false, sqrt_values = false;  // sqrt_values: a Sqrt stands on the TopK values
    std::string table, eps, classes;             // constants: the lookup's table, Max's bound, the class values ("": 0 .. C - 1)
    std::vector<size_t> equals;                  // the Equal node of each branch, in Concat order
    std::vector<std::string> equal_consts;
    std::string out;                             // the value the step is bound to
    bool out_col = false;                        // ... has shape [N, 1] (else [N]; probabilities: [N, C])
    std::vector<size_t> nodes;                   // the nodes that emit nothing (neither the TopK nor the anchor)
    // set by vote_begin
    std::shared_ptr<NearestPending> np;
    int lists = -1;
    int64_t k = 0;
  };
  std::map<size_t, VoteMatch> vote_at;      // anchor node index -> the pattern it closes
  std::map<size_t, size_t> vote_of_topk;    // TopK node index -> that anchor
  std::vector<char> vote_inside;            // nodes inside a vote pattern

  // ---- embedding lookups (host/embed.hpp; INTEGRATION.md 2.6 "Embedding lookups") ------------------------------------------------------
  // Gather(axis = 0) of a constant f32 table [V, d] / [V] by indices that are columns of a graph input: the column picks (Gather(axis = 1) /
  // Slice / Squeeze), Casts and constant offset Adds in front of it, the Reshape / Flatten of [N, k, d] to [N, k * d] and the feature-axis
  // Concat that alone reads the lookups (with numeric columns of a graph input beside them) become ONE Embed step that reads the input
  // buffer.  Found before the walk (find_embeds): a graph without such a Gather is lowered exactly as before.
  struct EmbedCols {  // a value that is columns [src0, src0 + k) of the input buffer: [N, k] (rank2) or [N]
    int64_t src0 = 0, k = 0;
    bool rank2 = true, truncated = false, int_input = false;
    std::vector<int64_t> off;   // the constant added to each column (empty: none)
    std::vector<size_t> chain;  // the nodes between the graph input and the value
  };
  struct EmbedLookup {
    size_t gather = 0;
    std::shared_ptr<TensorData> table;
    EmbedCols ix;
    int64_t V = 0, d = 0;
    std::vector<size_t> tail;  // the Reshape / Flatten behind it
    std::string out;
    std::vector<int64_t> shape;
  };
  struct EmbedGroup {
    std::vector<EmbedLookup> lookups;
    std::vector<std::pair<int, EmbedCols>> parts;  // in output order: (lookup, -) or (-1, columns to copy)
    std::vector<size_t> nodes;                     // every node the step stands for, ascending (filled by find_embeds)
  };
  std::map<size_t, EmbedGroup> embed_at;  // anchor node (the last of the group) -> the group
  int64_t embed_elems = 0;                // table elements of the model so far
  std::map<size_t, int> embed_node_id;    // Gather node -> its 1-based id in plan.prep_strict_nodes

  // ---- feature interactions (host/interact.hpp; INTEGRATION.md 2.6 "Feature interactions") ---------------------------------------------
  // dot: MatMul(T, Transpose(T, perm = [0,2,1])) of ONE value T [N, k, d], read whole or through Flatten / Reshape -> Gather(axis = 1) by a
  // constant list; the axis-1 Concat that alone reads the selection beside inputs of the Concat that built T joins the step (pass-through).
  // fm: Sub(square(ReduceSum(T, [1])), ReduceSum(square(T), [1])), the constant scalar Mul and the last-axis ReduceSum behind it.
  // Found before the walk by structure (find_interactions); shapes are known, and the caps checked, where the step is emitted
  // (lower_interact).  A graph without either pattern is lowered exactly as before.
  struct InteractView {
    size_t node = 0;
    std::vector<int64_t> target;  // Reshape: its constant target; Flatten: {axis}; Identity: empty
    bool back = false;            // the advanced-index form: behind its Transpose(1,0), where the value is [N, P] (else [P, N])
  };
  struct InteractMatch {
    int mode = kInteractDot;
    std::string T;
    std::vector<size_t> nodes;  // every node the step stands for but the anchor
    size_t product = 0;         // dot: the MatMul; fm: the Sub
    // dot
    std::vector<InteractView> views;  // between the product and the Gather
    size_t gather = SIZE_MAX;         // SIZE_MAX: the whole matrix
    std::vector<int64_t> idx;
    // TorchScript's advanced-index form: Gather(axis = 0) of the transposed, flattened matrix by `index_value` (evaluated once k is known)
    bool advanced = false;
    std::string index_value, selection_value;  // selection_value: the name of the selection [N, P] a pass-through Concat reads
    std::vector<InteractView> views_after;     // behind its Gather: in front of the Transpose(1,0) and behind it (InteractView::back)
    size_t out_concat = SIZE_MAX, t_concat = SIZE_MAX;  // pass-through: the Concat that reads the selection, the Concat that built T
    // fm
    bool keep = false;  // keepdims of the two field sums
    double h = 1.0;
    bool has_h = false, h_after = false;
    size_t last_sum = SIZE_MAX;  // the trailing ReduceSum
  };
  std::map<size_t, InteractMatch> interact_at;  // anchor (the last node of the pattern) -> the pattern

  // ---- lowering.cpp: buffers, values, the walk ----
  Lowerer(const onnx::Model &model, const std::string &output_select_in);
  int new_buf(const std::vector<int64_t> &shape);
  // input i of n; a preprocessing-region value is materialised first (get_raw: as it is)
  const Val &get(const NodeDef &n, size_t i);
  const Val &get_raw(const NodeDef &n, size_t i);
  bool has_input(const NodeDef &n, size_t i) const;
  const std::vector<float> &cf32(const NodeDef &n, const Val &v);
  void set_act(const NodeDef &n, int buf, const std::vector<int64_t> &shape, bool folded = false, int ra = 0);
  // Number of not-yet-folded consumers (incl. graph outputs) of a buffer across all its names.
  int live_uses(int buf);
  // The step that produced `v` if it can still absorb a trailing op: sole consumer is this node.
  Step *fusable_producer(const NodeDef &n, size_t in_idx);
  // The last step, if it wrote `buf` and nothing but this node reads `buf`: it can be folded into this node and removed (drop_tail)
  const Step *sole_tail(int buf);
  void drop_tail();
  // Appends `s` writing a new buffer of `shape`; returns the buffer.
  int push_step(Step s, const std::vector<int64_t> &shape);
  Step &emit(Step s, const NodeDef &n, const std::vector<int64_t> &out_shape);
  static std::vector<int64_t> flat_shape(const std::vector<int64_t> &shape);
  // ... the same for a step whose output is a window by construction
  void emit_window(Step s, const NodeDef &n, const std::vector<int64_t> &out_shape);
  // binds output o of n to a new buffer written by step s
  int bind_output(const NodeDef &n, size_t o, Step s, const std::vector<int64_t> &shape, bool whole);
  [[noreturn]] void bad_form(const NodeDef &n, const std::string &why);
  void lower_node(const NodeDef &n);
  // every operator but the few that understand the row-axis tag reads rows-first values only
  void check_row_axis(const NodeDef &n, bool understands);
  void constant_fill(const NodeDef &n);
  // the columns an input of a multi-input model takes in the input buffer: k of [rows, k]; a rank-1 [rows] integer input is one column
  static int64_t input_cols(const onnx::ValueDef &v);
  Plan run();
  void drop_unread_fake_quants();

  // ---- lowering.cpp: MatMul / Gemm, elementwise operators, Softmax, Sum ----
  void dense(const NodeDef &n, bool gemm);
  void dense_window(const NodeDef &n);
  // Broadcast a constant against an activation's per-row shape; returns per_row floats.
  std::vector<float> broadcast_const(const NodeDef &n, const Val &c, const std::vector<int64_t> &act_shape);
  static float fold_bop(char op, float u, float v);
  void binary(const NodeDef &n, char op);
  void unary(const NodeDef &n);
  void apply_unary(const NodeDef &n, size_t idx, Act act, float pa, float pb, const std::string &label);
  void softmax(const NodeDef &n, bool logsm);
  // Sum of any number of equal-shaped activations: a chain of residual adds
  void sum(const NodeDef &n);

  // ---- lowering.cpp: integer constant folding, Gather, Slice, Split, Cast, Concat, reductions, ArgMax / TopK, Reshape, Transpose ----
  void set_const_i64(const NodeDef &n, std::vector<int64_t> v, std::vector<int64_t> dims);
  void fold_int_binary(const NodeDef &n, char op, const Val &a, const Val &b);
  void shape_op(const NodeDef &n);
  std::vector<int64_t> const_ints(const NodeDef &n, size_t i, const char *what);
  void gather(const NodeDef &n);
  bool time_steppable(const Val &a) const;
  void time_step(const NodeDef &n, const Val &a, int64_t t, bool drop_axis);
  void emit_slice_cols(const std::string &origin, const Val &a, int64_t b, int64_t e, const std::string &out_name);
  void split(const NodeDef &n);
  void slice(const NodeDef &n);
  void cast(const NodeDef &n);
  void concat(const NodeDef &n);
  void reduce_mean(const NodeDef &n);
  // The Reduce* family over the last axis of [rows, F] or of a window [rows, T, E]: one RowReduce step (hip/reduce.hip)
  void row_reduce(const NodeDef &n);
  // ArgMin: the twin of ArgMax
  void argmin(const NodeDef &n);
  // k of a TopK node (a constant input from opset 10 on, an attribute before); -1: not a constant
  int64_t topk_k(const NodeDef &n);
  // TopK over the last axis of [rows, M]: one step per output that is read (Values, Indices as f32 values)
  void topk(const NodeDef &n);
  void argmax(const NodeDef &n);
  void alias(const NodeDef &n, const std::vector<int64_t> &new_shape);
  void reshape_like(const NodeDef &n);
  void reshape_tagged(const NodeDef &n);
  void transpose(const NodeDef &n);

  // ---- lowering.cpp: Conv, ConvTranspose, Resize, BatchNormalization, pooling, Pad, LRN ----
  void spatial(const NodeDef &n, Step &s, int64_t H, int64_t W, const int64_t *extra_pad = nullptr);
  void conv(const NodeDef &n);
  // the geometry fields of a Conv / QLinearConv node over activation `a` with a kernel of shape `ws` ([M,C/g,kh,kw], or [M,C/g,k]: Conv1d)
  void conv_geometry(const NodeDef &n, Step &s, const Val &a, const std::vector<int64_t> &ws);
  static std::vector<int64_t> conv_out_shape(const Step &s, const Val &a);
  static void convt_fold_affine(Step &p, const std::vector<double> &sc, const std::vector<double> &sh, const std::string &label);
  void conv_transpose(const NodeDef &n);
  void resize(const NodeDef &n);
  void batchnorm(const NodeDef &n);
  void pool(const NodeDef &n, bool is_max);
  void pad(const NodeDef &n);
  void lrn(const NodeDef &n);
  void global_avgpool(const NodeDef &n, bool is_max);

  // ---- lowering.cpp: Instance / Group norm, the channels-last view, Tokens, LayerNorm ----
  void spatial_norm_step(const NodeDef &n, const Val &a, int64_t G, std::vector<float> scale, std::vector<float> shift, float eps, const std::string &origin,
                         const std::string &out_name);
  // the activation input of a normalisation node and its constant scale / B
  Val spatial_norm_input(const NodeDef &n, std::vector<float> *scale, std::vector<float> *bias);
  void instance_norm(const NodeDef &n);
  void group_norm(const NodeDef &n);
  void find_group_norms();
  // a constant that multiplies / shifts x [N,C,...] per channel: C values shaped [C,1,1] / [1,C,1,1] (one spatial axis: [C,1] / [1,C,1])
  const std::vector<float> *per_channel_const(const Val *c, const std::vector<int64_t> &x_shape);
  bool exporter_group_norm(const GnMatch &gm, const NodeDef &first);
  bool nchw_tensor(const Val &a) const;
  bool reads_view(const NodeDef &n) const;
  // lowers `n` (by `body`) with every view among its inputs presented as the [N,C,H,W] tensor it names; the result is a view again
  template <class F>
  void as_nchw(const NodeDef &n, F body) {
    std::map<std::string, std::vector<int64_t>> was;
    for (const auto &in_name : n.inputs) {
      auto it = vals.find(in_name);
      if (it == vals.end() || !it->second.cl) continue;
      Val &v = it->second;
      was[in_name] = v.shape;
      v.shape = {v.shape[0], v.shape[3], v.shape[1], v.shape[2]};
      v.cl = false;
    }
    body();
    for (const auto &w : was) {
      Val &v = vals[w.first];
      v.shape = w.second;
      v.cl = true;
    }
    auto it = vals.find(n.outputs[0]);
    if (it == vals.end() || it->second.is_const || it->second.shape.size() != 4) bad_form(n, "its result on a channels-last view is not an [N,C,H,W] tensor");
    Val &o = it->second;
    o.shape = {o.shape[0], o.shape[2], o.shape[3], o.shape[1]};
    o.cl = true;
  }
  // a copy of `n` whose input `i` is the constant `c`
  NodeDef with_const_input(const NodeDef &n, size_t i, Val c);
  // the constant `c` with the dims `dims` (the same elements: type and half tag kept)
  static Val redimensioned(const Val &c, std::vector<int64_t> dims, std::vector<float> f32);
  void lower_on_view(const NodeDef &n);
  // ONE ChannelNorm step on the [N,C,H,W] tensor `x`; the result is bound to `out_name`, as a view or not
  void channel_norm_step(const NodeDef &n, const Val &x, std::vector<float> scale, std::vector<float> shift, bool has_shift, float eps, const std::string &origin,
                         const std::string &out_name, bool as_view);
  // LayerNormalization(axis = -1) on a view: over the channels at each pixel
  void channel_norm_node(const NodeDef &n);
  // MatMul of a view by a constant [C, M]: the 1x1 convolution [M, C, 1, 1] it is, through the path a Conv node takes
  void view_matmul(const NodeDef &n);
  bool channel_axis_mean(const NodeDef &n);
  bool channels_first_norm(const NodeDef &mean, const Val &x);
  bool conv_tensor_view(const Val &a) const;
  bool token_view_of_flatten(const NodeDef &n, const Val &a) const;
  void tokens_step(const NodeDef &n, const Val &a);
  // the Tokens step whose result `v` is, as that step left it
  Step *tokens_producer(const Val &v);
  // Concat with a token value among its operands: constants per row in front of it become the step's prefix rows.  false: no operand is one
  bool tokens_concat(const NodeDef &n);
  const NodeDef *only_reader(const std::string &v) const;
  bool last_axis_mean(const NodeDef &n, int64_t rank);
  // the f32 constant other operand of a two-input node reading `v`, or null
  const Val *const_operand(const NodeDef &n, const std::string &v, bool second_only = false);
  bool decomposed_layer_norm(const NodeDef &mean, const Val &x);
  // LayerNormalization (opset 17) over the last axis of [rows, E] / [rows, T, E]: one LayerNorm step (hip/layernorm.hip)
  void layer_norm(const NodeDef &n);

  // ---- lowering.cpp: row masks, self-attention, masked means ----
  // a constant known before the walk (an initializer or a Constant node): its first element and its element count
  bool graph_const_scalar(const std::string &name, double *v, size_t *count = nullptr) const;
  std::string trace_row_mask(const std::string &v0, RowMask *rm, bool lens = false) const;
  // the negative constant scalar b of masked keys
  float row_mask_fill(const NodeDef &n, const std::string &name, bool add);
  // Add(scores, other): other = Mul(Sub(1, float(mask [N,1,1,T])), b) (BERT); false: no such form
  bool match_add_row_mask(const NodeDef &add, const std::string &other, AttnMatch &am);
  // Where(masked, b, scores) or Where(kept, scores, b) (masked_fill)
  void match_where_row_mask(const NodeDef &wh, const std::string &scores, AttnMatch &am);
  void find_attention();
  void find_masked_means();
  void lower_masked_mean(const MaskedMean &mm, const NodeDef &div);
  const Val *find_value(const std::string &name);
  void lower_attention(const AttnMatch &am, const NodeDef &anchor);

  // ---- lower_attention_op.cpp: the opset-23 Attention and RMSNormalization operators ----
  void find_attention_ops();
  // RMSNormalization over the last axis of [rows, E] / [rows, T, E]: one RmsNorm step (hip/layernorm.hip)
  void rms_norm(const NodeDef &n);

  // ---- lower_rotary.cpp: RotaryEmbedding and the rotate_half spelling ----
  // `v` [N, h, T, dh] as a rotary embedding of another value; null: it is none (nothing is claimed).  Only structure is looked at
  std::shared_ptr<const RotaryMatch> match_rotary(const std::string &v) const;
  // every reader of the rotated value `rm.x` is a node of the match
  bool rotary_reads_alone(const RotaryMatch &rm) const;
  // the Rotary step of `rm` over [N, T, h * dh] (in0 and the view are the caller's); refusals name rm.at
  Step rotary_step(const RotaryMatch &rm, int64_t T, int64_t h, int64_t dh);
  // `v` behind a rotary embedding, for an attention front end that walks an operand back: returns the rotated value (and sets *rot), or `v`
  // itself where match_rotary finds none or the spelling's x has other readers.  An operator whose X is no head split is refused by name
  std::string behind_rotary(const std::string &v, std::shared_ptr<const RotaryMatch> *rot) const;
  // refuses, by name, the head-major RotaryEmbedding nodes that no attention front end absorbed (run: after find_attention)
  void check_rotary_ops();
  // RotaryEmbedding met by the walk: the 3-D form, one window step
  void rotary_embedding(const NodeDef &n);

  // ---- lower_shuffle.cpp: DepthToSpace, SpaceToDepth and their Reshape -> Transpose -> Reshape spellings ----
  void find_pixel_shuffles();
  // a live DepthToSpace / SpaceToDepth node that reads the rank-4 graph input `in` whose C, H or W is symbolic: refused by its name (run: before
  // the general rule that only the row axis of an input may be symbolic)
  void check_shuffle_extents(const onnx::ValueDef &in) const;
  // the spelling closed by the Reshape `last`: ONE PixelShuffle step (or, with b = 1, an alias); false: not exactly a spelling, nothing was done
  bool pixel_shuffle_spelling(const ShuffleMatch &sm, const NodeDef &last);
  void depth_space(const NodeDef &n);
  // the step over the [N,C,H,W] activation `a`, bound to out_node's first output; refusals name `at`
  void pixel_shuffle_step(const NodeDef &at, const NodeDef &out_node, const Val &a, int64_t b, bool to_space, bool channel_major, const std::string &origin);

  // ---- lowering.cpp: quantised and float16 graphs ----
  QArgs quant_args(const NodeDef &n, size_t si, size_t zi, const char *what);
  Quant act_quant(const NodeDef &n, const QArgs &qa, const char *what);
  void set_quant(const NodeDef &n, int buf, const std::vector<int64_t> &shape, int ra, const Quant &q, bool done, bool folded);
  void quantize_linear(const NodeDef &n);
  void dequantize_linear(const NodeDef &n);
  // QDense and QConv2d share their quantisation fields and the helpers below
  static bool quantised_layer(const Step &s);
  static void qdense_canonical_act(Step &s);
  void qdense_check_k(const NodeDef &n, const Step &s);
  void qdense_take_bias(const NodeDef &n, Step &s, const Val &c);
  Step make_qdense(const NodeDef &n, int in_buf, int64_t rep, const TensorData &w, bool trans, const std::vector<float> &ws, const std::vector<int64_t> &wz,
                   const Quant &xq);
  void take_quant_weights(const NodeDef &n, Step &s, const TensorData &w, bool trans, const std::vector<float> &ws, const std::vector<int64_t> &wz, const Quant &xq);
  bool qdense_from_qdq(const NodeDef &n, bool gemm);
  // QLinearMatMul(a, a_scale, a_zp, b, b_scale, b_zp, y_scale, y_zp): the same step, spelled in one node; its result stays a quantised value
  void qlinear_matmul(const NodeDef &n);
  // A QConv2d step over activation `a` (read from in_buf, quantised as xq) with the integer kernel `w` [M, C, kh, kw] (or [M, C, k])
  Step make_qconv(const NodeDef &n, const Val &a, int in_buf, const TensorData &w, const std::vector<float> &ws, const std::vector<int64_t> &wz, const Quant &xq);
  bool qconv_from_qdq(const NodeDef &n);
  void qlinear_conv(const NodeDef &n);
  static std::vector<uint16_t> half_bits(const std::vector<float> &v);
  void mark_half(const std::string &name);
  // lowers one node (by `body`) under the float16 typing rules: a node whose floating inputs are half yields half values
  template <class F>
  void lower_typed(const NodeDef &n, F body) {
    int n_half = 0, n_float_act = 0;
    for (const auto &in_name : n.inputs) {
      if (in_name.empty()) continue;
      const Val *v = nullptr;
      Val from_init;
      if (auto it = vals.find(in_name); it != vals.end()) v = &it->second;
      else if (auto ci = m.initializers.find(in_name); ci != m.initializers.end()) v = &(from_init = const_val(ci->second));
      if (!v) continue;
      if (v->is_const) n_half += v->c->dtype == onnx::kFloat && v->c->elem == onnx::kFloat16;
      else if (v->half) n_half++;
      else if (!int_bufs.count(v->buf) && !v->q) n_float_act++;
    }
    if (n_half && n_float_act) bad_form(n, "it mixes float16 and float activations; cast one side (Cast) so that the operator has one type");
    static const std::set<std::string> own_type = {"Cast", "ArgMax", "ArgMin", "Shape", "Size"};  // (their result type is not their input's)
    cur_half = n_half > 0 && !own_type.count(n.op);
    body();
    if (cur_half)
      for (const auto &o : n.outputs) mark_half(o);
    cur_half = false;
  }
  // does the result of this step need a rounding to be a half value, given half inputs?  Not when it only selects, moves or negates them
  static bool half_exact(const Step &s);
  void insert_half_roundings();
  bool hdense(const NodeDef &n, bool gemm);

  // ---- lower_recurrent.cpp: LSTM / GRU / RNN and their sequence lengths ----
  void find_seq_lens();
  void recurrent(const NodeDef &n);

  // ---- lower_ml.cpp: ai.onnx.ml linear heads, tree ensembles, SVM, ZipMap ----
  static NodeDef std_node(const NodeDef &from, const char *op, std::vector<std::string> in, std::string out);
  static void set_i(NodeDef &d, const char *k, int64_t v);
  bool wanted(const NodeDef &n, size_t i) const;
  std::vector<float> ml_floats(const NodeDef &n, const char *k, int64_t want, float dflt, bool allow_scalar);
  // post_transform over raw scores `raw` -> value `out`
  void ml_post_transform(const NodeDef &n, const std::string &raw, const std::string &out);
  void label_from_index(const NodeDef &n, std::string index, double a0, double step);
  void array_feature_extractor(const NodeDef &n);
  void ml_head(const NodeDef &n, bool cls, Step k, int64_t part_cols, Step r, int label_mode, int score_mode, int64_t score_cols);
  void tree_ensemble(const NodeDef &n);
  void svm(const NodeDef &n);
  void zipmap(const NodeDef &n);
  void ml_node(const NodeDef &n);

  // ---- lower_prep.cpp: ai.onnx.ml preprocessing regions ----
  static bool prep_encoder(const std::string &op);
  // marks `region`; returns the graph inputs that start inside a region
  std::set<std::string> find_regions();
  // identity columns over buffer `buf` (a region value's source); is_int: whole numbers already
  static PrepVal prep_identity(int buf, int64_t off, int64_t width, bool trunc, bool is_int);
  void set_prep(const std::string &name, PrepVal p, std::vector<int64_t> shape);
  PrepVal prep_in(const NodeDef &n, size_t i, int stage);
  // the region value `name` becomes a buffer: the source itself, a SliceCols, or one Prep step
  void materialize(const std::string &name, const NodeDef *at);
  std::vector<int64_t> afe_indices(const NodeDef &n);
  bool prep_side_by_side(const NodeDef &n, PrepVal *out);
  // columns of region values with one source side by side (Concat / FeatureVectorizer); false: the sources differ
  bool prep_concat(const NodeDef &n, std::vector<int64_t> out_shape);
  void prep_node(const NodeDef &n);

  // ---- lower_nearest.cpp: distance models ----
  // a constant f32 tensor known before the walk: an initializer or a Constant node's value
  std::shared_ptr<TensorData> const_tensor(const std::string &name) const;
  // g = -2 X C^T read by one node: the set (and its orientation) and the nodes of the chain
  bool match_minus_two_dot(const std::string &g, const std::string &x, NearestMatch *mt);
  void find_nearest();
  // the pending value of a recognised set; a form the kernel does not take (a time-major, half or quantised X, another width) returns false
  bool bind_nearest(const NodeDef &anchor, const std::string &x_name, const std::string &out, const float *C, int64_t M, int64_t F, const std::string &spelling,
                    bool rooted, const std::string &origin);
  void lower_nearest(const NearestMatch &mt);
  static void set_f(NodeDef &d, const char *k, float v);
  // com.microsoft CDist(X, C, metric): the distances in one node (what skl2onnx writes for neighbour models under optim = 'cdist')
  void cdist(const NodeDef &n);
  // the [rows, M] matrix of a pending distance value, for a reader that takes it as it is
  void materialize_nearest(const std::string &name);
  // the best-k lists of a pending distance value (one Nearest step per k)
  int nearest_lists(NearestPending &np, int64_t k);
  bool nearest_reader(const NodeDef &n);
  // the k-NN vote: the matcher, the decision at the TopK (take the pattern or give its nodes back) and the step at the anchor
  bool vote_axis1(const NodeDef &n) const;
  bool match_vote_lookup(const std::string &lab, VoteMatch *vm) const;
  bool match_vote_weights(const std::string &wei, VoteMatch *vm) const;
  bool match_vote_tally(const std::string &all, VoteMatch *vm, std::string *wei) const;
  void find_votes();
  void vote_begin(size_t anchor);
  void lower_vote(const VoteMatch &vm);

  // ---- lower_embed.cpp: embedding lookups ----
  // an integer constant known before the walk: an initializer or a Constant node
  bool graph_const_ints(const std::string &name, std::vector<int64_t> *v, std::vector<int64_t> *dims) const;
  // the integer list input `i` (or, in older opsets, attribute `attr`) of n; false: not constant
  bool graph_ints_arg(const NodeDef &n, size_t i, const char *attr, std::vector<int64_t> *v) const;
  // `v` as columns of the input buffer; "" or why it is none
  std::string embed_cols(const std::string &v, EmbedCols *c, int depth = 0) const;
  void find_embeds();
  void lower_embed(const EmbedGroup &g, const NodeDef &anchor);

  // ---- lowering.cpp: feature interactions ----
  // lax: a Reshape whose target is computed (from Shape nodes) counts too; lower_interact evaluates it
  bool interact_is_view(const NodeDef &r, const std::string &cur, InteractView *v, bool lax = false) const;
  // x * x or x ^ 2: the value squared ("" = n is no square)
  std::string interact_squared(const NodeDef &n) const;
  // ReduceSum over exactly `axis_a` or `axis_b`
  bool interact_sum_over(const NodeDef &n, int64_t axis_a, int64_t axis_b) const;
  // the node that alone reads the DATA of `v`: Shape nodes read its shape only and do not count (null: several, none, a graph output)
  const NodeDef *interact_data_reader(const std::string &v) const;
  bool interact_shape_closure(InteractMatch &im, size_t anchor) const;
  static constexpr int64_t kInteractDyn = INT64_MIN;
  bool interact_eval(const std::string &v, const std::string &z, int64_t k, std::vector<int64_t> *out, int depth = 0) const;
  void find_interactions();
  bool interact_released(const InteractMatch &im) const;
  void lower_interact(const InteractMatch &im, const NodeDef &anchor);
};

}  // namespace lowering

}  // namespace infera_hip
