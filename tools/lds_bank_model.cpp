// lds_bank_model.cpp -- host program: LDS-array cycles per wave-instruction, in the bank model of MI355X (lane groups and
// bank widths per instruction as measured by the round-3 probe; DESIGN.md "What round 3 added"), of every access the
// register-resident projection kernels (ea_proj_rs.hip, ea_dgrad_rs.hip) make to a 32-token tile of 128-byte rows, under
// the two chunk swizzles of csrc/ea_lds_swizzle.h.  One line per (pattern, swizzle):
//     <pattern> <swizzle> max=<worst instruction> sum=<all instructions of the pattern> n=<instructions>
// Only lanes of one group can conflict; identical dword addresses broadcast; every further distinct address on a busy bank
// adds one cycle to its group.   c++ -std=c++17 -I efficient-attention_amd/csrc tools/lds_bank_model.cpp
#include <stdio.h>
#include <algorithm>
#include <set>
#include <string>
#include <vector>
#include "ea_lds_swizzle.h"

namespace {

typedef int (*OffFn)(int row, int chunk16);
struct Instr {
  int bytes, banks;                      // per lane; bank of byte address a = (a / 4) mod banks
  std::vector<std::vector<int>> groups;  // lanes served in one LDS cycle when conflict-free
};

std::vector<std::vector<int>> ranges(std::initializer_list<std::initializer_list<int>> gs) {
  std::vector<std::vector<int>> out;     // each group: a list of first, last pairs
  for (auto& g : gs) {
    std::vector<int> lanes, b(g);
    for (size_t i = 0; i + 1 < b.size(); i += 2)
      for (int l = b[i]; l <= b[i + 1]; ++l) lanes.push_back(l);
    out.push_back(lanes);
  }
  return out;
}
std::vector<std::vector<int>> contiguous(int per) {
  std::vector<std::vector<int>> out;
  for (int l = 0; l < 64; l += per) {
    std::vector<int> g;
    for (int i = 0; i < per; ++i) g.push_back(l + i);
    out.push_back(g);
  }
  return out;
}

const Instr READ_B128 = {16, 64, ranges({{0, 3, 12, 15, 20, 27}, {4, 11, 16, 19, 28, 31}, {32, 35, 44, 47, 52, 59}, {36, 43, 48, 51, 60, 63}})};
const Instr READ_B64 = {8, 64, contiguous(32)};       // ds_read_b64 and ds_read_b64_tr_b16
const Instr WRITE_B64 = {8, 32, contiguous(16)};
const Instr WRITE_B128 = {16, 32, contiguous(8)};

int cycles(const Instr& in, const int (&addr)[64]) {
  int total = 0;
  for (const auto& g : in.groups) {
    std::vector<std::set<int>> bank(in.banks);
    for (int lane : g)
      for (int d = 0; d < in.bytes / 4; ++d) bank[(addr[lane] / 4 + d) % in.banks].insert(addr[lane] / 4 + d);
    size_t worst = 1;
    for (const auto& b : bank) worst = std::max(worst, b.size());
    total += (int)worst;
  }
  return total;
}

struct Acc {
  int mx = 0, sum = 0, n = 0;
  void add(int c) { mx = std::max(mx, c); sum += c; ++n; }
  void print(const char* pat, const char* swz) const { printf("%s %s max=%d sum=%d n=%d\n", pat, swz, mx, sum, n); }
};

constexpr int SLAB = 32 * 128;            // one 64-channel slab of a 32-token tile

void model(const char* swz, OffFn off) {
  int a[64];
  // row-operand reads, a k-step = 32 contiguous channels: lane (g, li) reads chunk 4 (ks & 1) + g of row li / 16 + li
  // (proj_rs_kernel, dgrad_rs_kernel, dgrad_fin_kernel: the products)
  Acc r4;
  for (int half = 0; half < 32; half += 16)
    for (int ksp = 0; ksp < 2; ++ksp) {
      for (int l = 0; l < 64; ++l) a[l] = off(half + (l & 15), 4 * ksp + (l >> 4));
      r4.add(cycles(READ_B128, a));
    }
  r4.print("row_read_4ks_g", swz);
  // row-operand reads of the token passes' mapping: chunk 2 g + ks (dgrad_fin_kernel: the q tile of the t correction)
  Acc r2;
  for (int half = 0; half < 32; half += 16)
    for (int ks = 0; ks < 2; ++ks) {
      for (int l = 0; l < 64; ++l) a[l] = off(half + (l & 15), 2 * (l >> 4) + ks);
      r2.add(cycles(READ_B128, a));
    }
  r2.print("row_read_2g_ks", swz);
  // transposed reads: lane (g, li) reads 8 bytes of row 4 g + (li >> 2) (+ 16), channels 16 dt + 4 (li & 3) ..
  // (proj_rs_kernel: pool_x)
  Acc tr;
  for (int half = 0; half < 32; half += 16)
    for (int dt = 0; dt < 4; ++dt) {
      for (int l = 0; l < 64; ++l) {
        const int g = l >> 4, li = l & 15;
        a[l] = off(half + 4 * g + (li >> 2), 2 * dt + ((li & 3) >> 1)) + 8 * (li & 1);
      }
      tr.add(cycles(READ_B64, a));
    }
  tr.print("tr_read", swz);
  // commit, slot order of proj_rs_kernel / dgrad_fin_kernel: thread tid parks chunk tid % 24 of token tid / 24 (16 bytes);
  // the same slots are read back 16 bytes wide for the corrected dq rows
  Acc st, wb;
  for (int wave = 0; wave < 12; ++wave) {
    for (int l = 0; l < 64; ++l) {
      const int tid = 64 * wave + l, tok = tid / 24, c = tid % 24;
      a[l] = (c >> 3) * SLAB + off(tok, c & 7);
    }
    st.add(cycles(WRITE_B128, a));
    wb.add(cycles(READ_B128, a));
  }
  st.print("commit_store_24", swz);
  wb.print("writeback_read_24", swz);
  // commit, slot order of dgrad_rs_kernel: chunk s = tid + 768 i of the tile's 32 x 72 chunks
  Acc st72;
  for (int i = 0; i < 3; ++i)
    for (int wave = 0; wave < 12; ++wave) {
      for (int l = 0; l < 64; ++l) {
        const int s = 64 * wave + l + 768 * i, tok = s / 72, c = s % 72;
        a[l] = (c >> 3) * SLAB + off(tok, c & 7);
      }
      st72.add(cycles(WRITE_B128, a));
    }
  st72.print("commit_store_72", swz);
  // 8-byte read-modify-write of the corrected dq piece: lane (g, li), channels 16 dt + 4 g .. of token 16 fnt + li
  Acc rr, rw;
  for (int fnt = 0; fnt < 2; ++fnt)
    for (int dt = 0; dt < 4; ++dt) {
      for (int l = 0; l < 64; ++l) {
        const int g = l >> 4, li = l & 15;
        a[l] = off(16 * fnt + li, 2 * dt + (g >> 1)) + (g & 1) * 8;
      }
      rr.add(cycles(READ_B64, a));
      rw.add(cycles(WRITE_B64, a));
    }
  rr.print("rmw_read", swz);
  rw.print("rmw_write", swz);
}

// lin_rs192_kernel (ea_linear_rs192.hip): a tile of 32 tokens x 192 channels, three slabs of 32 128-byte rows.
//   reads: wave (pair, half), k-step ks: lane (g, li) reads chunk 4 (ks & 1) + g of row 16 half + li of slab ks >> 1;
//   commit: thread tid parks chunk tid % 24 of token tid / 24.
void model_rs192(const char* swz, OffFn off) {
  int a[64];
  Acc rd, st;
  for (int half = 0; half < 32; half += 16)
    for (int ks = 0; ks < 6; ++ks) {
      for (int l = 0; l < 64; ++l) a[l] = (ks >> 1) * SLAB + off(half + (l & 15), 4 * (ks & 1) + (l >> 4));
      rd.add(cycles(READ_B128, a));
    }
  for (int wave = 0; wave < 12; ++wave) {
    for (int l = 0; l < 64; ++l) {
      const int s = 64 * wave + l, t = s / 24, c = s % 24;
      a[l] = (c >> 3) * SLAB + off(t, c & 7);
    }
    st.add(cycles(WRITE_B128, a));
  }
  rd.print("rs192_row_read", swz);
  st.print("rs192_commit_store", swz);
}

}  // namespace

// no argument: the 32-token tiles of ea_proj_rs.hip / ea_dgrad_rs.hip; "rs192": the tiles of ea_linear_rs192.hip
int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "rs192") {
    model_rs192("phi2", ea::swz_off2);
    model_rs192("psi", ea::swz_off3);
    return 0;
  }
  model("phi2", ea::swz_off2);
  model("psi", ea::swz_off3);
  return 0;
}
