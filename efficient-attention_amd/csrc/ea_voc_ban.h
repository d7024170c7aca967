// ea_voc_ban.h -- a row's ban list applied to its stored logits and tile candidates (ABI 36): what the constrained beam step's
// row kernel (ea_ceva_decode_vocab.hip) and the adaptive head's constrained selection (ea_adaptive_pick.hip) share.  Included
// inside their anonymous namespace, behind ea_voc_select.h.
//
// lrow [V]: the fp32 logits of one row of one table (a band of the adaptive head: its columns are the tokens base ..
// base + V - 1); tile [ceil(V / 16)]: one candidate per 16-column tile, what voc_select reads.  Every listed token that is a
// column of the table gets -inf stored in its place; behind a barrier every such token's tile candidate is formed again: the
// best of the tile's stored logits under voc_beats, the columns below V alone (a tile of -inf alone: its first column, as the
// table pass writes it).  Several threads may form the same tile's candidate; they store the same value.  A listed token
// outside the table is skipped.  Ordinary vector stores; the workgroup alone reads and writes this row.  Every thread of the
// workgroup calls it; it ends behind a barrier.
EA_DEV void voc_apply_bans(float* lrow, VocPick* tile, int V, const int32_t* ban, int nban, int64_t base) {
  for (int j = threadIdx.x; j < nban; j += blockDim.x) {
    const int64_t c = (int64_t)ban[j] - base;
    if (c >= 0 && c < (int64_t)V) lrow[c] = -INFINITY;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < nban; j += blockDim.x) {
    const int64_t c = (int64_t)ban[j] - base;
    if (c < 0 || c >= (int64_t)V) continue;
    const int c0 = (int)c & ~(VOC_TILE - 1);
    VocPick best = voc_none();
#pragma unroll
    for (int u = 0; u < VOC_TILE; ++u) {
      const int col = min(c0 + u, V - 1);                 // (a column past V: a clamped address, never a candidate)
      const VocPick other = VocPick{lrow[col], col};
      if (c0 + u < V && voc_beats(other, best)) best = other;
    }
    tile[c0 / VOC_TILE] = best;
  }
  __syncthreads();
}
