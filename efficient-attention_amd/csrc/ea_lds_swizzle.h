// ea_lds_swizzle.h -- the 16-byte chunk swizzles of the 128-byte-row LDS tiles, as constexpr functions that compile for the
// host as well as the device: ea_common.h builds its offset functions on them and tools/lds_bank_model.cpp evaluates the LDS
// bank model of MI355X for every access pattern the kernels make to such a tile (tests/test_lds_swizzle_model.py).
//
// A tile row is 64 16-bit channels = eight 16-byte chunks; chunk c of row `row` sits at chunk position c ^ swizzle(row).
// Two rows share one 256-byte span of the 64 banks, so which 16 of the 64 lanes of a ds_read_b128 are served together
// ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...) decides which (row, chunk) pairs must not meet on a bank.
#pragma once

namespace ea {

// Round 3: conflict-free when lane (g, li) reads chunk 2 g + ks of row li (the token passes: a k-step is every other chunk
// pair), for the re-shaped transposed reads and for 16-byte row stores.  With chunk 4 (ks & 1) + g of row li -- a k-step of 32
// contiguous channels, what the register-resident projection kernels read -- every 16-byte slot of a lane group is hit by
// two rows: 8 LDS cycles per ds_read_b128 instead of 4.
constexpr int swz_phi2(int row) { return (((row >> 1) & 3) << 1) | ((row ^ (row >> 3)) & 1); }

// psi: conflict-free for BOTH row-operand mappings (2 g + ks and 4 (ks & 1) + g), the transposed reads and the 16-byte
// stores in slot order; GF(2)-linear in the row bits b1 .. b3:  psi = b1 | (b1 ^ b2) << 1 | (b2 ^ b3) << 2.
constexpr int swz_psi(int row) { return ((row >> 1) ^ (row & ~1)) & 7; }

// byte offset of 16-byte chunk `chunk16` of row `row` in a tile of 128-byte rows
constexpr int swz_off2(int row, int chunk16) { return row * 128 + ((chunk16 ^ swz_phi2(row)) << 4); }
constexpr int swz_off3(int row, int chunk16) { return row * 128 + ((chunk16 ^ swz_psi(row)) << 4); }

}  // namespace ea
