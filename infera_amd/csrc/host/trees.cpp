// trees.cpp -- TreeEnsembleRegressor / TreeEnsembleClassifier: validation, child renumbering, mode normalisation, leaf tables.
#include "trees.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <utility>

namespace infera_hip {

namespace {

[[noreturn]] void fail(const std::string &why) { throw TreeError(why); }

std::vector<int64_t> ints_of(const onnx::NodeDef &n, const char *k) {
  const auto *p = n.attr_ints(k);
  return p ? *p : std::vector<int64_t>{};
}

// `k` as doubles: the float list, or `k`_as_tensor (opset 3; double tensors keep their exact values)
bool doubles_of(const onnx::NodeDef &n, const std::string &k, std::vector<double> &out) {
  const onnx::Attribute *a = n.attr(k), *t = n.attr(k + "_as_tensor");
  if (a && t) fail("both " + k + " and " + k + "_as_tensor are given");
  out.clear();
  if (t) {
    if (!t->t || (t->t->dtype != onnx::kFloat)) fail(k + "_as_tensor must be a float or double tensor");
    if (!t->t->f64.empty()) out = t->t->f64;
    else out.assign(t->t->f32.begin(), t->t->f32.end());
    return true;
  }
  if (a) {
    out.assign(a->floats.begin(), a->floats.end());
    return true;
  }
  return false;
}

enum Mode { kLeq, kLt, kGte, kGt, kEq, kNeq, kLeafMode };

Mode mode_of(const std::string &s) {
  if (s == "BRANCH_LEQ") return kLeq;
  if (s == "BRANCH_LT") return kLt;
  if (s == "BRANCH_GTE") return kGte;
  if (s == "BRANCH_GT") return kGt;
  if (s == "BRANCH_EQ") return kEq;
  if (s == "BRANCH_NEQ") return kNeq;
  if (s == "LEAF") return kLeafMode;
  fail("unknown node mode '" + s + "'");
}

std::string where(int64_t tree, int64_t node) { return "node " + std::to_string(node) + " of tree " + std::to_string(tree); }

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

}  // namespace

float tree_threshold_f32(double d, int dir) {
  if (std::isnan(d)) return NAN;
  const float f = float(d);  // round to nearest (overflow: +-inf)
  if (dir == 0) return double(f) > d ? std::nextafter(f, -INFINITY) : f;
  if (dir == 1) return double(f) < d ? std::nextafter(f, INFINITY) : f;
  return double(f) == d ? f : NAN;
}

TreePack pack_tree_ensemble(const onnx::NodeDef &n, int64_t F) {
  TreePack p;
  p.classifier = n.op == "TreeEnsembleClassifier";
  const std::vector<int64_t> tids = ints_of(n, "nodes_treeids");
  const size_t N = tids.size();
  if (N == 0) fail("unsupported operator form: the ensemble has no nodes");
  const std::vector<int64_t> nids = ints_of(n, "nodes_nodeids"), feats = ints_of(n, "nodes_featureids"),
                             tchild = ints_of(n, "nodes_truenodeids"), fchild = ints_of(n, "nodes_falsenodeids");
  std::vector<int64_t> mtt = ints_of(n, "nodes_missing_value_tracks_true");
  const onnx::Attribute *ma = n.attr("nodes_modes");
  const std::vector<std::string> modes_s = ma ? ma->strings : std::vector<std::string>{};
  std::vector<double> thr;
  const bool have_thr = doubles_of(n, "nodes_values", thr);
  const bool thr_f32 = have_thr && !n.attr("nodes_values_as_tensor");
  auto same_len = [&](const char *k, size_t len, bool optional) {
    if (optional && len == 0) return;
    if (len != N) fail("attribute arrays of different lengths: " + std::string(k) + " holds " + std::to_string(len) + " entries, nodes_treeids " + std::to_string(N));
  };
  same_len("nodes_nodeids", nids.size(), false);
  same_len("nodes_featureids", feats.size(), false);
  same_len("nodes_modes", modes_s.size(), false);
  same_len("nodes_truenodeids", tchild.size(), false);
  same_len("nodes_falsenodeids", fchild.size(), false);
  same_len("nodes_values", thr.size(), true);
  same_len("nodes_missing_value_tracks_true", mtt.size(), true);
  if (thr.empty()) thr.assign(N, 0.0);
  if (mtt.empty()) mtt.assign(N, 0);
  if (int64_t(N) > kTreeMaxNodes) fail("the ensemble has " + std::to_string(N) + " nodes, above the cap of " + std::to_string(kTreeMaxNodes));

  // ---- aggregation, post_transform, outputs
  const std::string agg = n.attr_s("aggregate_function", "SUM");
  if (agg == "AVERAGE") p.average = true;
  else if (agg != "SUM") fail("aggregate_function " + agg + " (only SUM and AVERAGE)");
  const std::string pt = n.attr_s("post_transform", "NONE");
  if (pt != "NONE" && pt != "LOGISTIC" && pt != "SOFTMAX") fail("post_transform " + pt);
  if (p.classifier) {
    if (n.attr("classlabels_strings")) fail("string class labels cannot be returned as numbers");
    const std::vector<int64_t> lab = ints_of(n, "classlabels_int64s");
    if (lab.size() < 2) fail("needs at least two classlabels_int64s");
    for (int64_t v : lab) p.labels.push_back(float(v));
    p.E = int64_t(lab.size());
  } else {
    p.E = n.attr_i("n_targets", 1);
    if (p.E < 1) fail("n_targets must be positive");
  }
  if (p.E > kTreeMaxTargets) fail("E = " + std::to_string(p.E) + " outputs, above the cap of " + std::to_string(kTreeMaxTargets));

  // ---- nodes: index by (tree, node id), children, roots
  std::map<std::pair<int64_t, int64_t>, size_t> at;
  std::vector<int64_t> tree_order;  // tree ids in order of first appearance
  std::map<int64_t, std::vector<size_t>> members;
  std::vector<Mode> mode(N);
  for (size_t i = 0; i < N; i++) {
    mode[i] = mode_of(modes_s[i]);
    if (!at.emplace(std::make_pair(tids[i], nids[i]), i).second) fail("duplicate " + where(tids[i], nids[i]));
    auto &mem = members[tids[i]];
    if (mem.empty()) tree_order.push_back(tids[i]);
    mem.push_back(i);
  }
  std::vector<int64_t> tix(N, -1), fix(N, -1);
  std::vector<int> parents(N, 0);
  for (size_t i = 0; i < N; i++) {
    if (mode[i] == kLeafMode) continue;
    if (feats[i] < 0 || feats[i] >= F) fail(where(tids[i], nids[i]) + ": feature id " + std::to_string(feats[i]) + " is not below the input width " + std::to_string(F));
    if (feats[i] >= kTreeMaxFeature) fail(where(tids[i], nids[i]) + ": feature id " + std::to_string(feats[i]) + " is above the cap of " + std::to_string(kTreeMaxFeature - 1));
    for (int side = 0; side < 2; side++) {
      const int64_t c = side ? fchild[i] : tchild[i];
      auto it = at.find({tids[i], c});
      if (it == at.end()) fail(where(tids[i], nids[i]) + " names child " + std::to_string(c) + ", which does not exist in its tree");
      (side ? fix : tix)[i] = int64_t(it->second);
      if (++parents[it->second] > 1) fail(where(tids[i], c) + " is the child of more than one branch (not a tree)");
    }
  }

  // ---- leaf weights
  const bool cls = p.classifier;
  const std::vector<int64_t> lt = ints_of(n, cls ? "class_treeids" : "target_treeids"), ln = ints_of(n, cls ? "class_nodeids" : "target_nodeids"),
                             lid = ints_of(n, cls ? "class_ids" : "target_ids");
  std::vector<double> lw;
  doubles_of(n, cls ? "class_weights" : "target_weights", lw);
  const char *wname = cls ? "class_weights" : "target_weights";
  if (ln.size() != lt.size() || lid.size() != lt.size() || lw.size() != lt.size())
    fail(std::string("attribute arrays of different lengths: ") + (cls ? "class_" : "target_") + "treeids / nodeids / ids / " + wname + " hold " +
         std::to_string(lt.size()) + " / " + std::to_string(ln.size()) + " / " + std::to_string(lid.size()) + " / " + std::to_string(lw.size()) + " entries");
  // binary single-column form (GBDT / XGBoost binary exports): two classes, every weight names the same class
  if (cls && p.E == 2 && !lid.empty()) {
    bool one = true;
    for (int64_t v : lid) one = one && v == lid[0];
    p.binary = one;
  }
  p.W = p.binary ? 1 : p.E;
  for (size_t k = 0; k < lid.size(); k++) {
    if (lid[k] < 0 || lid[k] >= p.E) fail(std::string(cls ? "class id " : "target id ") + std::to_string(lid[k]) + " is not below E = " + std::to_string(p.E));
    if (lw[k] < 0) p.is_signed = true;
  }
  if (p.binary && !p.is_signed && pt != "NONE")
    fail("binary single-column form with non-negative weights and post_transform " + pt + " (ambiguous; only NONE)");
  std::vector<double> base;
  doubles_of(n, "base_values", base);
  if (p.binary) {
    if (base.size() > 1) fail("the binary single-column form takes at most one base_values entry, got " + std::to_string(base.size()));
  } else if (!base.empty() && int64_t(base.size()) != p.E) {
    fail("base_values holds " + std::to_string(base.size()) + " values, expected " + std::to_string(p.E));
  }
  for (double b : base) p.base.push_back(float(b));
  std::map<size_t, std::vector<double>> leafw;  // node index -> W sums
  for (size_t k = 0; k < lt.size(); k++) {
    auto it = at.find({lt[k], ln[k]});
    if (it == at.end()) fail(std::string(wname) + " entry " + std::to_string(k) + " names " + where(lt[k], ln[k]) + ", which does not exist");
    if (mode[it->second] != kLeafMode) fail(std::string(wname) + " entry " + std::to_string(k) + " names " + where(lt[k], ln[k]) + ", which is not a leaf");
    auto &v = leafw[it->second];
    if (v.empty()) v.assign(size_t(p.W), 0.0);
    v[p.binary ? 0 : size_t(lid[k])] += lw[k];
  }

  // ---- pack: per tree, pair-DFS order (a node's two children adjacent)
  p.trees = int64_t(tree_order.size());
  p.nodes = int64_t(N);
  std::vector<uint32_t> rec;
  rec.reserve(2 * N);
  std::vector<uint32_t> roots;
  int64_t leaf_rows = 0;
  for (int64_t t : tree_order) {
    const auto &mem = members[t];
    if (int64_t(mem.size()) > kTreeMaxNodesPerTree)
      fail("tree " + std::to_string(t) + " has " + std::to_string(mem.size()) + " nodes, above the cap of " + std::to_string(kTreeMaxNodesPerTree));
    int64_t root = -1;
    for (size_t i : mem)
      if (parents[i] == 0) {
        if (root >= 0) fail("tree " + std::to_string(t) + " has more than one root (nodes " + std::to_string(nids[size_t(root)]) + " and " + std::to_string(nids[i]) + ")");
        root = int64_t(i);
      }
    if (root < 0) fail("tree " + std::to_string(t) + " has no root: its nodes form a cycle");
    const size_t base_pos = rec.size() / 2;
    roots.push_back(uint32_t(base_pos));
    rec.resize(rec.size() + 2 * mem.size(), 0);
    size_t next = base_pos + 1, placed = 1;
    std::vector<std::pair<size_t, std::pair<size_t, int64_t>>> stack{{size_t(root), {base_pos, 0}}};  // node, (position, depth)
    while (!stack.empty()) {
      const size_t i = stack.back().first, pos = stack.back().second.first;
      const int64_t depth = stack.back().second.second;
      stack.pop_back();
      uint32_t *r = rec.data() + 2 * pos;
      if (mode[i] == kLeafMode) {
        p.max_depth = std::max(p.max_depth, depth);
        auto it = leafw.find(i);
        if (p.W == 1) {
          r[0] = bits(it == leafw.end() ? 0.f : float(it->second[0]));
          r[1] = kTreeLeaf << 30;
        } else {
          if ((leaf_rows + 1) * p.W > kTreeMaxLeafFloats) fail("leaf table above the cap of " + std::to_string(kTreeMaxLeafFloats) + " values");
          for (int64_t j = 0; j < p.W; j++) p.leaves.push_back(it == leafw.end() ? 0.f : float(it->second[size_t(j)]));
          r[0] = 0;
          r[1] = kTreeLeaf << 30 | uint32_t(leaf_rows++);
        }
        continue;
      }
      // normalise: kind 0 (<=), 1 (<), 2 (==); `left` is taken when the compare holds
      const double d = thr[i];
      const size_t T = size_t(tix[i]), Fc = size_t(fix[i]);
      uint32_t kind;
      float th;
      size_t left, right;
      const Mode md = mode[i];
      const int dir = (md == kLeq || md == kGt) ? 0 : (md == kLt || md == kGte) ? 1 : 2;
      th = thr_f32 ? float(d) : tree_threshold_f32(d, dir);
      if (std::isnan(th)) {  // the compare never holds (NaN threshold, or == / != a double with no f32 value): constant outcome
        kind = 2;
        right = md == kNeq ? T : Fc;
        left = md == kNeq ? Fc : T;
      } else {
        kind = dir;
        const bool swap = md == kGte || md == kGt || md == kNeq;
        left = swap ? Fc : T;
        right = swap ? T : Fc;
      }
      const size_t nan_to = (mtt[i] != 0 || md == kNeq) ? T : Fc;  // NaN: tracks-true, else the IEEE result (false except for !=)
      const size_t q = next;
      next += 2;
      placed += 2;
      if (placed > mem.size()) fail("tree " + std::to_string(t) + " is not a tree (a cycle)");
      r[0] = bits(th);
      r[1] = kind << 30 | (nan_to == right ? kTreeNanRight : 0u) | uint32_t(feats[i]) << kTreeFeatureShift | uint32_t(q - pos);
      stack.push_back({right, {q + 1, depth + 1}});
      stack.push_back({left, {q, depth + 1}});
    }
    if (placed != mem.size()) fail("tree " + std::to_string(t) + " has nodes its root does not reach: they form a cycle");
  }
  p.slices = std::min<int64_t>(kTreeMaxSlices, (p.trees + kTreeSliceTrees - 1) / kTreeSliceTrees);
  p.tab = std::move(rec);
  p.tab.insert(p.tab.end(), roots.begin(), roots.end());
  for (int64_t s = 0; s <= p.slices; s++) p.tab.push_back(uint32_t(s * p.trees / p.slices));
  return p;
}

}  // namespace infera_hip
