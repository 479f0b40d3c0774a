// Nearest-atom matching (gfx950): the reduction over column tiles behind the EPI_ROWARGMAX epilogue of the
// grouped GEMM (sae_gemm_kernel.h).
//
// The epilogue leaves, per output row and per 64-column wave tile, the pair (max of alpha * <a_i, b_j> over
// the tile's candidate columns, column of that max) as two fp32 words (the column bit-cast), with
// (-3.0e38, INT_MAX) for a tile that had no candidate.  rowmatch_reduce_kernel folds the T pairs of a row
// into one under the same total order -- larger value first, then the smaller column -- so the lowest
// column wins among equal values whatever the tiling, and the result is the same every run (no atomics).
//   one 16-lane group per row (16 rows per 256-thread block): lane l reads pairs l, l + 16, ... (8-byte
//   loads, a group covers 128 contiguous bytes), then four xor shuffles inside the group.
// Lane 0 of the group writes val[g][row][pass] / idx[g][row][pass]; a row with no winner, or past the
// model's live rows (nact_m), gets (0.0, -1).  With an exclusion list (int32 [G][*][E]) the winner also goes
// into slot e0 + pass (when that slot exists): the next pass of a top-m query excludes it, chained on the
// stream without host work.
#include "common.h"

namespace scamd {

constexpr int RM_NONE = 0x7fffffff;

__global__ __launch_bounds__(256) void rowmatch_reduce_kernel(const float2* __restrict__ part, int T, int Mp, int M,
                                                              float* __restrict__ val, int* __restrict__ idx, long so,
                                                              int ldo, int pass, int* __restrict__ excl, long sexcl,
                                                              int E, int e0, const int* __restrict__ nact_m,
                                                              int row_blocks) {
  const int g = blockIdx.x / row_blocks;
  const int row = (blockIdx.x - g * row_blocks) * 16 + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  if (row >= M) return;  // (a whole 16-lane group leaves together)
  float mx = -3.0e38f;
  int col = RM_NONE;
  if (!nact_m || row < nact_m[g]) {
    const float2* pr = part + ((long)g * Mp + row) * T;
    for (int t = sub; t < T; t += 16) {  // tiles in ascending column order: a strict > keeps the lowest
      const float2 q = pr[t];
      const int oc = __float_as_int(q.y);
      if (oc != RM_NONE && (q.x > mx || col == RM_NONE)) { mx = q.x; col = oc; }
    }
  }
#pragma unroll
  for (int s = 1; s < 16; s <<= 1) {
    const float ov = __shfl_xor(mx, s, 64);
    const int oc = __shfl_xor(col, s, 64);
    if (ov > mx || (ov == mx && oc < col)) { mx = ov; col = oc; }
  }
  if (sub == 0) {
    const bool none = col == RM_NONE;
    const long o = (long)g * so + (long)row * ldo + pass;
    val[o] = none ? 0.f : mx;
    idx[o] = none ? -1 : col;
    if (excl && e0 + pass < E) excl[(long)g * sexcl + (long)row * E + e0 + pass] = none ? -1 : col;
  }
}

}  // namespace scamd

using namespace scamd;

extern "C" {

// part fp32 [G][Mp][T][2] (EPI_ROWARGMAX partials, T = N / 64 wave tiles); val fp32 / idx int32 with group
// stride `so` and row stride `ldo` (elements), written at [g][row][pass] for rows < M; excl (optional)
// int32 with group stride `sexcl` and E slots per row; nact_m (optional) int32 [G] live rows.
int sc_rowmatch_reduce(const void* part, int G, int Mp, int T, int M, float* val, int* idx, long so, int ldo,
                       int pass, int* excl, long sexcl, int E, int e0, const int* nact_m, hipStream_t stream) {
  if (!part || !val || !idx || G < 1 || T < 1 || M < 1 || M > Mp || ldo < 1 || pass < 0 || pass >= ldo || so < 0)
    return 1;
  if (excl && (E < 1 || E > 8 || e0 < 0 || sexcl < (long)M * E)) return 1;
  const int row_blocks = (M + 15) / 16;
  unsigned blocks;
  if (!sc_grid((long)G * row_blocks, 1, blocks)) return 1;
  hipLaunchKernelGGL(rowmatch_reduce_kernel, dim3(blocks), dim3(256), 0, stream,
                     reinterpret_cast<const float2*>(part), T, Mp, M, val, idx, so, ldo, pass, excl, sexcl, E, e0,
                     nact_m, row_blocks);
  return sc_launched();
}

}  // extern "C"
