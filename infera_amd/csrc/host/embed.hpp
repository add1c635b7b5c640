// embed.hpp -- embedding lookups as one step kind (INTEGRATION.md 2.6 "Embedding lookups"): what the lowering packs for an
// Embed step and what its kernel (hip/embed.hip) walks.
//   in  [rows, W]     the model input or a buffer a step wrote, row-major: index columns (f32 values, truncated toward zero) and numeric columns
//   out [rows, F]     a sequence of pieces in output order:
//     lookup piece    out[r, o : o + d] = table[i, 0 : d],  i = trunc(in[r, src]) + offset, i in [-V, -1] counts from the end; any other i
//                     (NaN included) raises the call's failure word with the piece's 1-based node id and loads row 0
//     copy piece      out[r, o : o + d] = in[r, src : src + d]
//     gap piece       out[r, o : o + d] = 0: the columns of a Concat input that another step computes; a CopyCols behind this step writes them
//   Every value is a copy of a bit pattern: there is no arithmetic on table or numeric values.
// Caps (refused at load, embed_table_refusal / pack_embed): V <= kEmbedMaxV, d <= kEmbedMaxD, |offset| <= kEmbedMaxV, pieces <= kEmbedMaxPieces,
// F < 2^31 - 4096; the lowering holds the tables of all Embed steps of a model to kEmbedMaxTableElems (each step packs its own copy).
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace infera_hip {

constexpr int64_t kEmbedMaxV = int64_t(1) << 24;  // every index up to here is an exact f32 value
constexpr int64_t kEmbedMaxD = 4096;
constexpr int64_t kEmbedMaxPieces = 1024;
constexpr int64_t kEmbedMaxTableElems = int64_t(1) << 27;  // per model, summed over its Embed steps: 512 MiB on the host and on each device; keeps the kernel's 32-bit table offsets valid
constexpr int kEmbedDescInts = 8;        // per piece on the device: out, len, src, V (0: a copy piece, -1: a gap), offset, table base, node id, 0
constexpr int64_t kEmbedMapMaxF = 8192;  // output rows up to here get a direct column -> piece map (16-bit entries), longer ones a search
constexpr int64_t kEmbedTileBytes = 32768;  // the staged source tile of a work group, at most
constexpr int64_t kEmbedLdsBytes = 65536;
constexpr int64_t kEmbedMaxRowsPerTile = 64;
constexpr int64_t kEmbedTileFloats = 16384;  // output floats a work group aims at

struct EmbedPiece {
  int table = -1;  // index into EmbedPack::tables; -1: a copy piece, -2: a gap
  int64_t src = 0, V = 0, d = 0, offset = 0, out = 0;
  int node = 0;  // lookup pieces: 1-based id in Plan::prep_strict_nodes
};

struct EmbedPack {
  int64_t W = 0, F = 0;
  int64_t win_k = 0, win_d = 0;  // the result is the window [rows, win_k, win_d] (0: a feature row)
  std::vector<EmbedPiece> pieces;
  std::vector<std::shared_ptr<const std::vector<float>>> tables;  // distinct tables (a shared table once); pack_embed copies them into `tab` and lets go of them
  int64_t n_tables = 0;
  std::vector<int64_t> table_base;  // of each table in `tab`, a multiple of 4
  int64_t gathered = 0;  // floats a row takes out of the tables
  // what the kernel reads
  std::vector<int32_t> desc;   // kEmbedDescInts per piece
  std::vector<uint16_t> map;   // piece of every output column, padded to a multiple of 8 entries; empty beyond kEmbedMapMaxF
  std::vector<float> tab;      // the tables one behind the other, each at a multiple of 4 floats
  int R = 1;                   // rows per work-group tile, from the model alone
  bool staged = true;          // the tile's source columns go through LDS (else W is too wide: indices are read where they lie)
  int64_t bytes_per_row() const { return 4 * (W + gathered + F); }
};

// why an f32 table of these dims cannot be looked up ("" = it can)
std::string embed_table_refusal(const std::vector<int64_t> &dims);

// fills the device-side fields from pieces / tables / W; pieces must tile [0, F) in order.  "" or why the step cannot be served
std::string pack_embed(EmbedPack &p);

}  // namespace infera_hip
