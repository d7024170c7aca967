// ea_linear_rs192.hip -- the 192 -> 192 projection with the WEIGHT RESIDENT IN REGISTERS:
//     Y[t][o] = sum_k A[t][k] W[o][k] (+ bias[o]),   K = NO = 192, A / Y / W 16-bit, t over all B*N tokens
// the output projection of a 192-wide layer (W = W_proj) and its input gradient (W = W_proj^T).  lin_kernel (ea_linear.hip)
// stages the 72 KB weight into the LDS of every workgroup -- 512 workgroups, 37 MB chip-wide through the load pipes for a
// 72 KB weight -- and gives a wave one or two 32-row tiles, too few for a steady state.  Here, in the pattern of
// ea_proj_rs.hip / ea_dgrad_rs.hip, ONE 12-wave workgroup per CU holds the whole weight in its registers: wave w owns the
// 32-column pair w >> 1 (48 VGPRs of MFMA A operands per lane, loaded once, 16 bytes per lane and load, from an image that
// w192_prepare_kernel writes in this order) and the 16-token half w & 1 of every tile.  The activations stream through LDS
// once: a tile of 32 tokens is fetched by all 768 threads (one 16-byte chunk each), double-buffered, one barrier per
// tile, the next tile's loads in flight under the current tile's MFMAs; rows past the end are clamped to the last row
// (loads AND stores, no predicated memory operation in the loop).  The tile has the psi layout (ea_lds_swizzle.h): the reads
// are chunk 4 (ks & 1) + g of row li, as in dgrad_fin_kernel.
//
// Y has the BITS of lin_kernel on the same operands: the same MFMA with the weight as A operand, the weight rows of the
// pair's two tiles interleaved in fours (MFMA row li <-> column 8 (li >> 2) + (li & 3) [+ 4]), k-step ks = channels
// 32 ks .. + 31 with lane group g on 32 ks + 8 g .. + 7, one fp32 chain ks = 0 .. 5, the bias rounded to the element type
// and added in fp32, one rounding at the end; a lane ends up with eight consecutive columns of one token: 16-byte stores.
//
// The image: 16-byte piece ((pair * 2 + j) * 6 + ks) * 64 + lane, lane = 16 g + li, holds
//     W[32 pair + 8 (li >> 2) + (li & 3) + 4 j][32 ks + 8 g .. + 7]            (rs192_row below)
// -- 4608 pieces, a permutation of the 16-byte chunks of the [192, 192] weight (of W_proj for the forward product; for the
// input gradient W = W_proj^T, a piece is eight elements down a column of W_proj).
#include "ea_common.h"
#include "ea_linear.h"

namespace ea {

struct Rs192P {
  const char* a;        // [rows, 192] element type, row stride lda elements
  const char* wimg;     // the weight in register order (above)
  const float* bias;    // [192] fp32 or null
  char* y;              // [rows, 192] element type, row stride ldy elements
  int rows, ntiles;
  long lda, ldy;
};

constexpr int R1_K = 192, R1_WAVES = 12, R1_KT = R1_K / 32, R1_SLABS = R1_K / 64, R1_CPR = R1_K / 8;

// (What the rejected decompositions measured -- 64-token tiles, two workgroups per CU, 16 columns per wave: DESIGN.md 5.)
template <typename E>
__global__ __launch_bounds__(R1_WAVES * 64, 1) void lin_rs192_kernel(const Rs192P p) {
  constexpr int TOK = 32, SLAB = TOK * 128;
  __shared__ __attribute__((aligned(16))) char tile[2][R1_SLABS * SLAB];
  __shared__ __attribute__((aligned(16))) float bias_s[R1_K];          // rounded to the element type
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pair = wave >> 1, half = wave & 1;
  // ---- this thread's staging slot: chunk st_c of token st_tok of the tile (32 tokens x 24 chunks = 768 slots) ----
  const int st_tok = tid / R1_CPR, st_c = tid - st_tok * R1_CPR;
  u32x4 nb;
  auto issue = [&](int t) {
    const int tok = min(t * TOK + st_tok, p.rows - 1);
    nb = ldg16(p.a + (size_t)tok * p.lda * 2 + st_c * 16);
  };
  int t = blockIdx.x;
  issue(t);
  typename E::x8 wr[2][R1_KT];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int ks = 0; ks < R1_KT; ++ks)
      wr[j][ks] = as_x8<E>(ldg16(p.wimg + ((size_t)((pair * 2 + j) * R1_KT + ks) * 64 + lane) * 16));
  for (int i = tid; i < R1_K; i += R1_WAVES * 64) bias_s[i] = p.bias ? E::to_f(E::from_f(p.bias[i])) : 0.f;
  const int st_off = (st_c >> 3) * SLAB + lds_off3<64>(st_tok, st_c & 7);
  const int rd_off = lds_off3<64>(16 * half + li, g);                          // chunk 4 (ks & 1) + g: g ^ psi, then bit 2

  // the weight has to have arrived HERE (an empty asm that reads it): left to the first MFMA that uses a fragment, the waits
  // sit inside the loop and count the previous tile's store on every trip
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int ks = 0; ks < R1_KT; ++ks) asm volatile("" ::"v"(wr[j][ks]));
  int buf = 0;
  for (; t < p.ntiles; t += gridDim.x, buf ^= 1) {
    sts16(tile[buf] + st_off, nb);
    issue(t + gridDim.x);                       // (past the last tile: the clamped last row, in bounds and never committed)
    __syncthreads();
    f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll
    for (int ks = 0; ks < R1_KT; ++ks) {
      const typename E::x8 b = as_x8<E>(lds16(tile[buf] + (ks >> 1) * SLAB + (rd_off ^ ((ks & 1) << 6))));
      acc0 = E::mma(wr[0][ks], b, acc0);
      acc1 = E::mma(wr[1][ks], b, acc1);
    }
    // lane (g, li): columns 32 pair + 8 g .. + 7 of token li of the wave's half
    const int n = 32 * pair + 8 * g;
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bias_s + n), b1 = *reinterpret_cast<const f32x4*>(bias_s + n + 4);
    const int tok = min(t * TOK + 16 * half + li, p.rows - 1);
    const f32x4 v0 = acc0 + b0, v1 = acc1 + b1;
    u32x4 o;
    o[0] = pack2<E>(v0[0], v0[1]); o[1] = pack2<E>(v0[2], v0[3]);
    o[2] = pack2<E>(v1[0], v1[1]); o[3] = pack2<E>(v1[2], v1[3]);
    stg16(p.y + ((size_t)tok * p.ldy + n) * 2, o);
  }
}

// row strides the kernel takes (16-byte rows of at least 192 elements; the token index stays in 32 bits, the offsets in 40)
int linear_rs192_supported(int rows, long lda, long ldy) {
  return rows > 0 && lda >= R1_K && ldy >= R1_K && !(lda & 7) && !(ldy & 7) && (long)rows * (lda > ldy ? lda : ldy) < (1l << 40) &&
         rows <= (1 << 30);
}

int linear_rs192_dispatch(int dtype, const void* a, long lda, const void* wimg, const float* bias, void* y, long ldy, int rows,
                          hipStream_t st) {
  if (rows <= 0) return EA_OK;
  if (!linear_rs192_supported(rows, lda, ldy)) return EA_E_UNSUPPORTED;
  if (dtype != EA_BF16 && dtype != EA_F16) return EA_E_BADARG;
  Rs192P p;
  p.a = (const char*)a; p.wimg = (const char*)wimg; p.bias = bias; p.y = (char*)y;
  p.rows = rows; p.ntiles = (rows + 31) / 32; p.lda = lda; p.ldy = ldy;
  int grid = ea_device_cus();
  if (grid > p.ntiles) grid = p.ntiles;
  const dim3 gr((unsigned)grid), b(R1_WAVES * 64);
  if (dtype == EA_BF16) hipLaunchKernelGGL(lin_rs192_kernel<BF16>, gr, b, 0, st, p);
  else hipLaunchKernelGGL(lin_rs192_kernel<F16>, gr, b, 0, st, p);
  return (int)hipGetLastError();
}

}  // namespace ea
