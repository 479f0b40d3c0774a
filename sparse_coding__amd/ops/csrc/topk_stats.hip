// Per-feature quantities of a top-k ensemble straight from the picks (gfx950): the select's
// (idx, val) [G][B][kmax] pairs are never densified into a [G][B][n] code matrix.
//
// topk_pick_count_kernel: fire counts.  Slot s of row b counts for feature idx[g, b, s] iff
//   s < min(k[g], kmax) and val > 0 (a pick whose score the ReLU clamped to 0 is not a firing; the
//   padded slots (0, 0.0) never count).  Shaped like topk_slot_count_kernel (topk.hip): an LDS
//   histogram per (model, block of rows), then one global 64-bit integer add per non-empty bin, so a
//   feature that every row picks costs one atomic per block.  Integer adds only: exact, and the same
//   bits in any order.  With step_dev and every > 0 the kernel does nothing unless
//   *step_dev % every == 0 (a device predicate: graph-capturable, no host read).
// topk_pick_stats_kernel: the sparse counterpart of col_moments + col_topk (feature_stats.hip).  One
//   wave per (model, feature) walks that feature's slot list (sc_topk_slot_lists over ALL models:
//   slot ids (g B + b) kmax + s in increasing batch row b) and, over the entries with val > 0, adds
//   the count and sum c .. sum c^4 (fp64 products and sums: a bf16-valued code to the 4th power is
//   exact in fp64) to acc [G][5][n], folds the maximum into mx (a column nobody picks has the dense
//   maximum 0.0) and merges the entries into the running top-K lists under col_topk's order (value
//   descending, then row ascending; only strictly positive values; empty slots (0.0, -1); a later
//   equal value never displaces a listed one).  Every feature is owned by one wave, the cross-lane
//   sums are one fixed butterfly and the lists are merged in row order: no floating-point atomics,
//   the same bits every run and under any chunking of the calls.
#include "code_lists.h"

namespace scamd {

__global__ __launch_bounds__(256) void topk_pick_count_kernel(const int* __restrict__ idx, const float* __restrict__ val,
                                                              const int* __restrict__ kv,
                                                              unsigned long long* __restrict__ counts, int B, int n,
                                                              int kmax, int rpb, const int* __restrict__ step_dev,
                                                              int every) {
  extern __shared__ int hist[];
  if (step_dev && every > 0 && (*step_dev % every) != 0) return;  // (uniform: the whole grid leaves)
  const int g = blockIdx.y, b0 = blockIdx.x * rpb, tid = threadIdx.x;
  const int k = min(kv[g], kmax);
  for (int j = tid; j < n; j += 256) hist[j] = 0;
  __syncthreads();
  const int rows = min(rpb, B - b0);
  for (int t = tid; t < rows * k; t += 256) {
    const int r = t / k, sl = t - r * k;
    const long slot = ((long)g * B + b0 + r) * kmax + sl;
    const int j = idx[slot];
    if (val[slot] > 0.f && (unsigned)j < (unsigned)n) atomicAdd(&hist[j], 1);
  }
  __syncthreads();
  for (int j = tid; j < n; j += 256)
    if (hist[j]) atomicAdd(&counts[(long)g * n + j], (unsigned long long)hist[j]);
}

__global__ __launch_bounds__(256) void topk_pick_stats_kernel(const int* __restrict__ perm, const int* __restrict__ offs,
                                                              const float* __restrict__ val, double* __restrict__ acc,
                                                              float* __restrict__ mx, float* __restrict__ top_vals,
                                                              long long* __restrict__ top_rows, int G, int B, int n,
                                                              int kmax, int K, long long row0, long perm_len) {
  ListWalk w;
  if (!list_walk<4>(w, (long)G * n)) return;
  w.split(n);
  const int lane = w.lane, g = w.g, j = w.f;
  const long list = w.id;
  const int beg = offs[list];
  int L = min(max(offs[list + 1] - beg, 0), B);  // (a row picks a feature at most once)
  if (beg < 0 || (long)beg + L > perm_len) L = 0;  // (offsets that are no slot lists: read nothing)
  const long total = (long)G * B * kmax;
  // the running list: entry `lane` of K lives in lane `lane`
  float lv = 0.f;
  long long lr = -1;
  if (K > 0 && lane < K) {
    lv = top_vals[list * K + lane];
    lr = top_rows[list * K + lane];
  }
  double cnt = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
  float vmax = 0.f;
  for (int i0 = 0; i0 < L; i0 += 64) {
    const int i = i0 + lane;
    float v = 0.f;
    long long row = -1;
    if (i < L) {
      const int slot = perm[beg + i];
      if (slot >= 0 && slot < total) {
        v = val[slot];
        row = row0 + (slot / kmax - g * B);
      }
    }
    const bool on = v > 0.f;  // (NaN and the clamped picks stay out)
    if (on) {
      const double c = (double)v, c2 = c * c;
      cnt += 1.0;
      s1 += c;
      s2 += c2;
      s3 += c2 * c;
      s4 += c2 * c2;
      vmax = fmaxf(vmax, v);
    }
    if (K > 0) {
      // candidates above the current K-th value, merged one by one in row order (lane order)
      unsigned long long todo = __ballot(on && v > __shfl(lv, K - 1, 64));
      while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const float cv = __shfl(v, src, 64);
        const long long cr = __shfl(row, src, 64);
        // listed entries come from earlier rows: the equal ones stay ahead of the candidate
        const int p = __popcll(__ballot(lane < K && lv >= cv));
        const float pv = __shfl_up(lv, 1, 64);
        const long long pr = __shfl_up(lr, 1, 64);
        if (p < K) {
          if (lane == p) {
            lv = cv;
            lr = cr;
          } else if (lane > p && lane < K) {
            lv = pv;
            lr = pr;
          }
        }
      }
    }
  }
  cnt = wave_sum_xor<false>(cnt);
  s1 = wave_sum_xor<false>(s1);
  s2 = wave_sum_xor<false>(s2);
  s3 = wave_sum_xor<false>(s3);
  s4 = wave_sum_xor<false>(s4);
  vmax = wave_max(vmax);
  if (lane < 5) {
    const double add = lane == 0 ? cnt : lane == 1 ? s1 : lane == 2 ? s2 : lane == 3 ? s3 : s4;
    double* A = acc + ((long)g * 5 + lane) * n + j;
    *A += add;
  } else if (lane == 5) {
    mx[list] = fmaxf(mx[list], vmax);  // (vmax >= 0: the dense column's maximum over ReLU codes)
  }
  if (K > 0 && lane < K) {
    top_vals[list * K + lane] = lv;
    top_rows[list * K + lane] = lr;
  }
}

}  // namespace scamd

using namespace scamd;

extern "C" {

// counts int64 [G, n] += the batch's fire counts (see topk_pick_count_kernel).  step_dev (device int)
// and every > 0: count only when *step_dev % every == 0; step_dev null or every <= 0: always.
int sc_topk_pick_counts(const int* idx, const float* val, const int* k, long* counts, int G, int B, int n, int kmax,
                        const int* step_dev, int every, hipStream_t stream) {
  if (!idx || !val || !k || !counts || G < 1 || B < 1 || n < 1 || n > 32768 || kmax < 1) return 1;
  const int rpb = 64;
  const dim3 grid((unsigned)((B + rpb - 1) / rpb), (unsigned)G);
  const size_t lds = (size_t)n * sizeof(int);
  hipLaunchKernelGGL(topk_pick_count_kernel, grid, dim3(256), lds, stream, idx, val, k,
                     reinterpret_cast<unsigned long long*>(counts), B, n, kmax, rpb, step_dev, every);
  return sc_launched();
}

// perm / offs: the sorted slot lists of all G models (sc_topk_slot_lists with Gs = G); acc fp64 [G, 5, n],
// mx fp32 [G, n], top_vals fp32 / top_rows int64 [G, n, K] (K = 0: no lists, both may be null); the
// batch's rows are row0 .. row0 + B - 1; perm_len: the entries of perm (B sum_g min(k_g, kmax)).
int sc_topk_pick_stats(const int* perm, const int* offs, const float* val, double* acc, float* mx, float* top_vals,
                       long* top_rows, int G, int B, int n, int kmax, int K, long row0, long perm_len,
                       hipStream_t stream) {
  if (!perm || !offs || !val || !acc || !mx || G < 1 || B < 1 || n < 1 || kmax < 1 || K < 0 || K > 32 || row0 < 0 ||
      perm_len < 1)
    return 1;
  if (K > 0 && (!top_vals || !top_rows)) return 1;
  if ((long)G * B * kmax >= (1l << 31)) return 1;
  unsigned blocks;
  if (!sc_grid((long)G * n, 4, blocks)) return 1;
  hipLaunchKernelGGL(topk_pick_stats_kernel, dim3(blocks), dim3(256), 0, stream, perm, offs, val,
                     acc, mx, top_vals, reinterpret_cast<long long*>(top_rows), G, B, n, kmax, K, (long long)row0, perm_len);
  return sc_launched();
}

}  // extern "C"
