// recurrent.hpp -- ONNX LSTM / GRU / RNN: load-time validation and the packed tables hip/rnn.hip runs on.
// Semantics: INTEGRATION.md section 2.6; kernel design: the hip/rnn.hip header.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "onnx_model.hpp"

namespace infera_hip {

// caps of the kernel (each rejected at load with its own message): the hidden units of one direction are 16-unit tiles spread over at
// most 8 waves x 4 tiles; x_t and two copies of h live in LDS as [k][16 rows] (64 bytes per k: 128 KB at the caps); T only bounds
// the serial loop
constexpr int64_t kRnnMaxH = 512, kRnnMaxF = 1024, kRnnMaxT = 4096;

enum RnnOp : int { kRnnLstm = 0, kRnnGru = 1, kRnnPlain = 2 };
// what a Recurrent step stores (Step::out_mode): Y [rows, T, D, H], Y_h [rows, D, H], Y_c [rows, D, H]
enum RnnOut : int { kRnnY = 0, kRnnYh = 1, kRnnYc = 2 };

struct RnnError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// an optional input of the node: absent, a constant, or present but computed from the rows (c == nullptr)
struct RnnInput {
  bool present = false;
  const onnx::TensorData *c = nullptr;
};

struct RnnPack {
  int op = kRnnLstm;
  int64_t T = 0, F = 0, H = 0, D = 1, G = 4;
  int64_t Fp = 0, Hp = 0;  // F and H padded to multiples of 16 (zero weights)
  bool reverse = false;    // D == 1: walks t = T-1 .. 0 (D == 2: direction 0 forward, 1 reverse)
  bool lbr = false;        // GRU linear_before_reset
  bool relu = false;       // RNN activation Relu instead of Tanh
  int64_t layout = 0;
  // [D][Hp / 16 tiles][(Fp + Hp) / 16][G][64 lanes][4]: lane l, element j of k-group q holds row g*H + 16*tile + (l & 15), column
  // 16 q + 4 j + (l >> 4) of [W | R] (columns 0..Fp-1: W, Fp..: R): four A fragments of v_mfma_f32_16x16x4_f32 per 16-byte load
  std::vector<float> wr;
  std::vector<float> bias;   // [D][G][Hp]: Wb + Rb summed in f64, rounded once (GRU linear_before_reset = 1, gate h: Wb only)
  std::vector<float> bias2;  // [D][Hp]: Rb of gate h for GRU linear_before_reset = 1, else zeros
  std::vector<float> h0, c0; // [D][Hp]: one row of the initial state (zeros when absent)
};

// Validates node `n` (X [T, F] per row) and packs it.  Throws RnnError with the reason.
RnnPack pack_recurrent(const onnx::NodeDef &n, int64_t T, int64_t F, const RnnInput &W, const RnnInput &R, const RnnInput &B, const RnnInput &seq_lens,
                       const RnnInput &h0, const RnnInput &c0, const RnnInput &P);

}  // namespace infera_hip
