// prep.cpp -- ai.onnx.ml preprocessing nodes: validation against INTEGRATION.md section 2.6 and the tables of a Prep step (prep.hpp).
#include "prep.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>

namespace infera_hip {

namespace {

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

float exact_int(int64_t v, const char *what) {
  if (v > kPrepMaxExact || v < -kPrepMaxExact)
    throw PrepError(std::string(what) + " value " + std::to_string(v) + " is beyond 2^24 and cannot be held exactly as f32");
  return float(v);
}

// the numbers of a tensor attribute (keys_tensor / values_tensor / default_tensor); *is_int: its type
std::vector<float> tensor_values(const onnx::Attribute &a, const char *what, bool *is_int) {
  if (!a.t || (a.t->dtype != onnx::kFloat && a.t->dtype != onnx::kInt64))
    throw PrepError(std::string(what) + ": only numeric tensors are supported (string keys and values cannot be served as f32)");
  *is_int = a.t->dtype == onnx::kInt64;
  if (!*is_int) return a.t->f32;
  std::vector<float> o;
  for (int64_t v : a.t->i64) o.push_back(exact_int(v, what));
  return o;
}

}  // namespace

ImputerSpec parse_imputer(const onnx::NodeDef &n, int64_t F) {
  ImputerSpec s;
  const onnx::Attribute *fl = n.attr("imputed_value_floats"), *in = n.attr("imputed_value_int64s");
  const bool has_f = fl && !fl->floats.empty(), has_i = in && !in->ints.empty();
  if (has_f == has_i) throw PrepError("needs exactly one of imputed_value_floats / imputed_value_int64s");
  if (has_f) {
    s.imputed = fl->floats;
    s.replaced = n.attr_f("replaced_value_float", 0.f);
  } else {
    for (int64_t v : in->ints) s.imputed.push_back(exact_int(v, "imputed_value_int64s"));
    s.replaced = exact_int(n.attr_i("replaced_value_int64", 0), "replaced_value_int64");
  }
  if (s.imputed.size() != 1 && int64_t(s.imputed.size()) != F)
    throw PrepError(std::string(has_f ? "imputed_value_floats" : "imputed_value_int64s") + " holds " + std::to_string(s.imputed.size()) +
                    " values, expected 1 or " + std::to_string(F));
  if (s.imputed.size() == 1) s.imputed.assign(size_t(F), s.imputed[0]);
  return s;
}

float parse_binarizer(const onnx::NodeDef &n) { return n.attr_f("threshold", 0.f); }

OneHotSpec parse_onehot(const onnx::NodeDef &n) {
  if (n.attr("cats_strings")) throw PrepError("cats_strings: string categories are not supported (the C ABI carries f32 only)");
  const std::vector<int64_t> *c = n.attr_ints("cats_int64s");
  if (!c || c->empty()) throw PrepError("needs cats_int64s");
  OneHotSpec s;
  for (int64_t v : *c) s.cats.push_back(exact_int(v, "cats_int64s"));
  s.zeros = n.attr_i("zeros", 1) != 0;
  return s;
}

PrepTable onehot_table(const std::vector<float> &cats) {
  PrepTable t;
  t.int_keys = true;
  t.keys = cats;
  std::sort(t.keys.begin(), t.keys.end());
  t.keys.erase(std::unique(t.keys.begin(), t.keys.end()), t.keys.end());
  t.vals.assign(t.keys.size(), 1.f);
  return t;
}

PrepTable parse_label_encoder(const onnx::NodeDef &n, bool *int_values) {
  for (const char *k : {"classes_strings", "keys_strings", "values_strings"})
    if (n.attr(k)) throw PrepError(std::string(k) + ": string keys and values are not supported (the C ABI carries f32 only)");
  std::vector<float> keys, vals;
  bool int_keys = false, ivals = false;
  int nk = 0, nv = 0;
  if (const onnx::Attribute *a = n.attr("keys_int64s")) {
    for (int64_t v : a->ints) keys.push_back(exact_int(v, "keys_int64s"));
    int_keys = true, nk++;
  }
  if (const onnx::Attribute *a = n.attr("keys_floats")) keys = a->floats, nk++;
  if (const onnx::Attribute *a = n.attr("keys_tensor")) keys = tensor_values(*a, "keys_tensor", &int_keys), nk++;
  if (const onnx::Attribute *a = n.attr("values_int64s")) {
    for (int64_t v : a->ints) vals.push_back(exact_int(v, "values_int64s"));
    ivals = true, nv++;
  }
  if (const onnx::Attribute *a = n.attr("values_floats")) vals = a->floats, nv++;
  if (const onnx::Attribute *a = n.attr("values_tensor")) vals = tensor_values(*a, "values_tensor", &ivals), nv++;
  if (nk != 1 || nv != 1) throw PrepError("needs exactly one numeric keys_* and one numeric values_* attribute");
  if (keys.empty()) throw PrepError("no keys");
  if (keys.size() != vals.size())
    throw PrepError("keys and values differ in length (" + std::to_string(keys.size()) + " vs " + std::to_string(vals.size()) + ")");
  float dflt = ivals ? -1.f : -0.f;  // the specification's defaults
  if (const onnx::Attribute *a = n.attr("default_tensor")) {
    bool di = false;
    std::vector<float> d = tensor_values(*a, "default_tensor", &di);
    if (d.size() != 1) throw PrepError("default_tensor must hold one value");
    dflt = d[0];
  } else if (ivals) {
    if (n.attr("default_int64")) dflt = exact_int(n.attr_i("default_int64", -1), "default_int64");
  } else if (n.attr("default_float")) {
    dflt = n.attr_f("default_float", -0.f);
  }
  PrepTable t;
  t.int_keys = int_keys;
  std::vector<size_t> order;
  for (size_t i = 0; i < keys.size(); i++) {
    if (std::isnan(keys[i])) {
      if (t.has_nan) throw PrepError("duplicate key nan");
      t.has_nan = true;
      t.nan_val = vals[i];
      continue;
    }
    if (keys[i] == 0.f) keys[i] = 0.f;  // -0 matches 0
    order.push_back(i);
  }
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return keys[a] < keys[b]; });
  for (size_t j = 0; j < order.size(); j++) {
    if (j && keys[order[j]] == keys[order[j - 1]]) {
      char buf[48];
      std::snprintf(buf, sizeof buf, "%.9g", double(keys[order[j]]));
      throw PrepError(std::string("duplicate key ") + buf);
    }
    t.keys.push_back(keys[order[j]]);
    t.vals.push_back(vals[order[j]]);
  }
  *int_values = ivals && std::nearbyint(dflt) == dflt;
  t.dflt = dflt;
  return t;
}

PrepPack pack_prep(const std::vector<PrepCol> &cols, const std::vector<std::shared_ptr<PrepTable>> &tables, int64_t F_in) {
  PrepPack p;
  p.F_in = F_in;
  p.F = int64_t(cols.size());
  if (F_in > kPrepMaxSource) throw PrepError("reads " + std::to_string(F_in) + " source columns; at most " + std::to_string(kPrepMaxSource));
  if (p.F > kPrepMaxOut)
    throw PrepError("writes " + std::to_string(p.F) + " columns; at most " + std::to_string(kPrepMaxOut) + " per preprocessing step");
  p.R = std::max<int64_t>(1, std::min(kPrepStageBytes / (4 * std::max<int64_t>(F_in, 1)), kPrepMaxTileOut / std::max<int64_t>(p.F, 1)));
  std::map<int, uint32_t> at;  // table id -> first pair
  for (const PrepCol &c : cols) {
    if (c.table < 0 || at.count(c.table)) continue;
    const PrepTable &t = *tables[size_t(c.table)];
    at[c.table] = uint32_t(p.tab.size() / 2);
    for (size_t i = 0; i < t.keys.size(); i++) {
      p.tab.push_back(t.keys[i]);
      p.tab.push_back(t.vals[i]);
    }
    p.tab.push_back(NAN);
    p.tab.push_back(t.nan_val);
  }
  for (const PrepCol &c : cols) {
    uint32_t w = uint32_t(c.src) | (c.kind << kPrepKindShift);
    if (c.trunc) w |= kPrepTrunc;
    if (c.impute) w |= kPrepImpute | (c.imp_nan ? kPrepImputeNan : 0u);
    if (c.affine) w |= kPrepAffine;
    uint32_t off = 0, cnt = 0;
    if (c.table >= 0) {
      const PrepTable &t = *tables[size_t(c.table)];
      off = at[c.table];
      cnt = uint32_t(t.keys.size());
      if (t.int_keys) w |= kPrepIntKey;
      if (t.has_nan) w |= kPrepNanKey;
      if (c.kind == kPrepOneHot) w |= kPrepStrict | (uint32_t(std::min(c.strict, kPrepMaxStrictIds)) << kPrepStrictShift);
    }
    p.onehot += c.kind == kPrepOneHot;
    p.lookup += c.kind == kPrepLookup;
    p.strict = p.strict || (w & kPrepStrict);
    p.desc.insert(p.desc.end(), {w, off, bits(c.c), cnt});
    p.cst.insert(p.cst.end(), {c.repl, c.imp, c.off, c.scale});
  }
  if (p.tab.empty()) p.tab = {0.f, 0.f};  // (the kernel always has a table pointer)
  return p;
}

}  // namespace infera_hip
