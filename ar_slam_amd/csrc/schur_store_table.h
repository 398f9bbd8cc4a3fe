// schur_store_table.h -- the descriptors of k_schur<false>'s output stage.
//
// The stage forms the capture's local reduced system (M = 2 + 6 nblk rows: f,
// six per distinct tag, the rhs row) as 16x16 MFMA tiles (r, cc), cc <= r + 1,
// in that order (kSchurStoreTiles of them), and lane (lk, li) holds the
// elements (16 r + lk + 4 reg, 16 cc + li), reg 0..3, of a tile.  Where an
// element goes in the capture's block-packed slab (schur_block_off), which LDS
// word holds its F'F / F'r / f'F / f'f term and whether it is stored at all
// depend only on nblk, the tile, the lane and the register: one 32-bit entry
// each, built here at compile time from the helpers the gather plan uses, so
// the layout has one source.  The kernel's copy is a constant in its code
// object (13 KB per nblk, shared by every capture); the host's copy is what
// arslam_debug_schur_store_table returns.
#pragma once
#include <cstdint>

#include "lm_problem.h"

namespace arslam {

constexpr int kSchurStoreTiles = 13;
// entry: bits 0..14 the byte offset of the element from the capture's slab
// base, bits 15..29 the byte offset in LDS of the term the product is
// subtracted from, bit 31 "not stored".  The kernel stores through a buffer
// descriptor whose range is the capture's slab, and a "not stored" entry's
// offset field lies past every slab: the range check is the store's predicate.
constexpr int kSchurStoreLdsShift = 15;
constexpr uint32_t kSchurStoreMask = 0x7fffu;
constexpr uint32_t kSchurStoreSkip = 0x80000000u | (kSchurStoreMask & ~7u);
static_assert(schur_slab_size(kSchurMfmaBlocks) * 8 <= (long)(kSchurStoreMask & ~7u), "slab byte offsets fit 15 bits");
static_assert(schur_lds(kSchurMfmaBlocks).ff00 * 8 <= (int)kSchurStoreMask, "LDS byte offsets fit 15 bits");

// e[nblk - 1][tile][lane][reg]: a lane's four registers of a tile are one 16-byte load
struct alignas(16) SchurStoreTable {
  uint32_t e[kSchurMfmaBlocks][kSchurStoreTiles][kWave][4];
};
// the first tile of tile row r in that order (row r has min(r + 2, 4) tiles)
__host__ __device__ constexpr int schur_store_row_tile(int r) { return r == 0 ? 0 : r == 1 ? 2 : r == 2 ? 5 : 9; }

// Element (p, q) of the local system of a capture with nblk tags.
//   stored: the lower block triangle, V <= U (every column of a row's own block)
//   term  : (0, 0) f'f;  (m, q < m) F'r (f'r at q = 0);  a tag row i of block u:
//           (., 0) f'F_u[i], (., q in block u) F_u'F_u packed upper, else none
// An element without a term reads the pad word FF[27] of the first tag block,
// which k_schur zeroes and never adds to: 0.0 - acc either way.  (A "not
// stored" entry reads the LDS word 0, any value.)
constexpr uint32_t schur_store_entry(int nblk, int p, int q) {
  const int m = 1 + 6 * nblk, M = m + 1;
  if (p >= M || q >= M) return kSchurStoreSkip;
  const int U = schur_blk(p, m), V = schur_blk(q, m);
  if (V > U) return kSchurStoreSkip;
  const int sV = schur_blk_size(V, nblk);
  const int i = p - schur_blk_start(U, nblk), j = q - schur_blk_start(V, nblk);
  const long off = schur_block_off(U, V, nblk) + (long)i * sV + j;
  const SchurLds l = schur_lds(nblk);
  int term = l.FF + 27;
  if (p == 0) {
    term = l.ff00;
  } else if (p == m) {
    if (q < m) term = l.Ftr + q;
  } else if (q == 0) {
    term = l.FF + 28 * (U - 1) + 21 + i;
  } else if (V == U) {
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    term = l.FF + 28 * (U - 1) + lo * 6 - lo * (lo - 1) / 2 + (hi - lo);
  }
  return (uint32_t)(8 * off) | ((uint32_t)(8 * term) << kSchurStoreLdsShift);
}

constexpr SchurStoreTable make_schur_store_table() {
  SchurStoreTable t{};
  for (int nblk = 1; nblk <= kSchurMfmaBlocks; ++nblk) {
    int tile = 0;
    for (int r = 0; r < 4; ++r)
      for (int cc = 0; cc < 4 && cc <= r + 1; ++cc, ++tile)
        for (int lane = 0; lane < kWave; ++lane)
          for (int reg = 0; reg < 4; ++reg)
            t.e[nblk - 1][tile][lane][reg] =
                schur_store_entry(nblk, 16 * r + (lane >> 4) + 4 * reg, 16 * cc + (lane & 15));
  }
  return t;
}

}  // namespace arslam
