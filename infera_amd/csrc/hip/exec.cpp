// exec.cpp -- the plan executor: one model, one context, rows already on the device.  Cuts the rows into device passes (activation scratch),
// long convolutional passes into two lanes, and walks the plan step by step (PassRunner::run; what each step launches, with which of its
// device tables: steps.cpp).  Replaces `SimplePlan::run` (engine.rs:142-145).  Also the strict-prep failure word and the device-resident
// entry points (infera_hip_predict_device).
#include <cstdlib>

#include "runtime.hpp"

namespace infera_hip {
namespace rt {

// Rows per device pass for plans that need activation scratch (pure: no allocation).
int64_t rows_per_pass(const LoadedModel &m, int64_t rows) {
  if (m.scratch_per_row <= 0 || m.plan.out_buf == 0) return rows;
  int64_t by_budget = int64_t(kScratchBudgetBytes / (size_t(m.scratch_per_row) * 4));
  // INFERA_MAX_ROWS_PER_PASS (2^18) bounds the scratch of plans with wide intermediates; plans whose intermediates are a
  // few floats per row (a linear model + Softmax + Normalizer) take passes of up to 256 MB of scratch instead -- 77 passes
  // of 262k rows over a 20M-row table were launch-bound (three ~10 us kernels each)
  const int64_t by_size = int64_t((256ull << 20) / (size_t(m.scratch_per_row) * 4));
  const int64_t cap = std::max<int64_t>(int64_t(Config::get().max_rows_per_pass), by_size);
  int64_t rows_pass = std::min<int64_t>(rows, std::max<int64_t>(1, std::min<int64_t>(by_budget, cap)));
  // equal passes (2000 images at 1783 per pass run as 1000 + 1000, not 1783 + 217: the short tail would leave the chip half empty)
  const int64_t npass = (rows + rows_pass - 1) / rows_pass;
  return (rows + npass - 1) / npass;
}

// ... and grows the scratch for it (never inside a stream capture: callers that capture call this first).
int64_t prepare_scratch(const LoadedModel &m, ThreadCtx &ctx, int64_t rows) {
  const int64_t rows_pass = rows_per_pass(m, rows);
  // (+ 1 row: a pass cut into two lanes of ceil(n / 2) rows each)
  if (m.scratch_per_row > 0 && m.plan.out_buf != 0)
    ctx.ensure_dev(ctx.scratch, ctx.scratch_cap, size_t(rows_pass + ThreadCtx::kMaxLanes) * size_t(m.scratch_per_row) * 4);
  return rows_pass;
}

// A long pass of a convolutional plan runs as TWO LANES: its rows in two halves, each through all the plan's kernels on its own stream, with
// its own half of the scratch.  Every launch of such a plan ends in a partial round of workgroups (ResNet-18 at 1024 images: 12.25 / 6.125 /
// 3.06 rounds for its 128 / 256 / 512-channel layers -- 3.2 % of the pass, profiles/r04_tail_rounds.txt); with two independent kernel
// sequences in flight the other lane's workgroups fill those rounds (and the stem of one lane runs beside the matrix-bound layers of the
// other).  Same kernels, same per-row arithmetic: results are bit-identical (tests/test_conv_split_gpu.py).  ResNet-18, 1024 images: 18.42 ->
// 17.94 ms (-2.6 %); three or four lanes: no gain (profiles/r04_conv_lanes_ab.txt).  With the lanes a 1024-image pass is within 0.2 % of the per-image
// time of a 1003-image one (whole rounds everywhere), and splitting the last round finer only costs (round 5, profiles/r05_tail_split_ab.txt).  Not under a stream capture (INFERA_HIPGRAPH=1), not
// for the short passes of the host path (many contexts already overlap there).
constexpr int64_t kLaneMinRows = 512;
int lanes_of(const LoadedModel &m, int64_t nr) {
  // (INFERA_CONV_LANES=1: one lane -- for counter passes, which serialise kernels: per-kernel figures of full-size launches; tools/profile_bench.sh)
  static const bool one = getenv("INFERA_CONV_LANES") && atoi(getenv("INFERA_CONV_LANES")) == 1;
  if (one || nr < kLaneMinRows || Config::get().use_hipgraph || m.scratch_per_row <= 0) return 1;
  for (const ExecKind k : m.exec)
    if (k == ExecKind::ConvTiled) return ThreadCtx::kMaxLanes;
  return 1;
}

void PassRunner::run(hipStream_t s, int64_t first_row, int64_t rows, int64_t slot_rows, int64_t scratch_off) {
  stream = s;
  r0 = first_row;
  nr = rows;
  int64_t off = scratch_off;
  for (size_t i = 0; i < m.slot_per_row.size(); i++) {
    slot_base[i] = off;
    off += m.slot_per_row[i] * slot_rows;
  }
  for (size_t i = 0; i < st.size(); i++) {
    size_t skip = 0;
    if (!launch_fused(i, &skip)) launch_plain(i);
    i += skip;
  }
  HIP_TRY(hipGetLastError());
}

// in_colmajor: d_in is one column-major chunk [in_per_row][rows] (only with m.in_colmajor_ok, which implies a single pass)
void exec_plan(const LoadedModel &m, const DeviceModel &dm, ThreadCtx &ctx, const float *d_in, float *d_out, int64_t rows, bool in_colmajor) {
  const Plan &p = m.plan;
  if (rows <= 0) return;
  if (p.out_buf == 0) {  // pure alias / Identity graph
    HIP_TRY(hipMemcpyAsync(d_out, d_in, size_t(rows) * size_t(p.in_per_row()) * 4, hipMemcpyDeviceToDevice, ctx.stream));
    return;
  }
  const int64_t rows_pass = prepare_scratch(m, ctx, rows);
  // a plan with a zeros = 0 OneHotEncoder or an embedding lookup: the call's failure word, cleared on the call's stream and read back with
  // the result
  const bool strict = !p.prep_strict_nodes.empty();
  if (strict) {
    ctx.ensure_prep_err();
    HIP_TRY(hipMemsetAsync(ctx.prep_err, 0, sizeof(int), ctx.stream));
  }
  // a column-major chunk [K][rows] cannot be cut into row passes (pass r0 would start at a row-major offset with stride nr):
  // callers check single_pass() first and stage such calls row-major instead; this guards every kernel family at once
  if (in_colmajor && rows_pass != rows) throw InferaError::onnx("internal: column-major input needs a single pass");
  PassRunner runner(m, dm, ctx, d_in, d_out, in_colmajor);
  for (int64_t r0 = 0; r0 < rows; r0 += rows_pass) {
    const int64_t nr = std::min(rows_pass, rows - r0);
    const int nl = in_colmajor ? 1 : lanes_of(m, nr);
    if (nl == 1) {
      runner.run(ctx.stream, r0, nr, rows_pass, 0);
      continue;
    }
    if (!ctx.lane_ev[0]) {
      for (hipStream_t &ls : ctx.lane_stream) HIP_TRY(hipStreamCreateWithFlags(&ls, hipStreamNonBlocking));
      for (hipEvent_t &e : ctx.lane_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const int64_t nlane = (nr + nl - 1) / nl;  // rows per lane (the last lane: what is left)
    HIP_TRY(hipEventRecord(ctx.lane_ev[0], ctx.stream));  // (the input is on the device, the previous pass has left the scratch)
    try {
      for (int l = 0; l < nl; l++) {
        const int64_t l0 = l * nlane, ln = std::min(nlane, nr - l0);
        if (ln <= 0) break;
        hipStream_t ls = l == 0 ? ctx.stream : ctx.lane_stream[l - 1];
        if (l > 0) HIP_TRY(hipStreamWaitEvent(ls, ctx.lane_ev[0], 0));
        runner.run(ls, r0 + l0, ln, nlane, int64_t(m.scratch_per_row) * nlane * l);
        if (l > 0) {
          HIP_TRY(hipEventRecord(ctx.lane_ev[l], ls));
          HIP_TRY(hipStreamWaitEvent(ctx.stream, ctx.lane_ev[l], 0));
        }
      }
    } catch (...) {
      // a lane that was not joined must not still be writing the scratch / the result when the caller unwinds and the context is reused
      for (hipStream_t ls : ctx.lane_stream)
        if (ls) (void)hipStreamSynchronize(ls);
      throw;
    }
  }
  if (strict) {
    int word = 0;
    HIP_TRY(hipMemcpyAsync(&word, ctx.prep_err, sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    if (word > 0) {
      const Plan::StrictNode &sn = p.prep_strict_nodes[size_t(std::min<int>(word, int(p.prep_strict_nodes.size()))) - 1];
      throw InferaError::onnx(sn.node + sn.message);
    }
  }
}


const DeviceModel &device_model(const LoadedModel &m, int slot) {
  if (m.dev.empty()) throw InferaError::onnx("HIP backend unavailable: " + m.device_error);
  return *m.dev[size_t(slot)];
}


}  // namespace rt
using namespace rt;

void run_device(const LoadedModel &m, int device_ordinal, const float *d_in, float *d_out, int64_t rows) {
  if (m.dev.empty()) throw InferaError::onnx("HIP backend unavailable: " + m.device_error);
  const int slot = slot_of_ordinal(device_ordinal);
  ThreadCtx &ctx = ctx_for_slot(slot);
  exec_plan(m, device_model(m, slot), ctx, d_in, d_out, rows);
}

void sync_device(int device_ordinal) {
  ThreadCtx &ctx = ctx_for_slot(slot_of_ordinal(device_ordinal));
  HIP_TRY(hipStreamSynchronize(ctx.stream));
}

hipStream_t thread_stream(int device_ordinal) { return ctx_for_slot(slot_of_ordinal(device_ordinal)).stream; }

}  // namespace infera_hip
