// Per-feature label profiles from sparse codes, and the row gather that puts a pool in label order (gfx950).
//
//   csr_take_rows_kernel   one wave per (model, output row): output row i of the CSR is input row index[i], its
//                          entries copied 64 at a time to out_ptr[g, i] onwards (the host's cumsum of the
//                          gathered lengths).  Every source bound is checked again here: an index outside
//                          [0, N) or a row that fails 0 <= row_ptr[r] <= row_ptr[r + 1] <= cap_in is written as
//                          empty; every store sits behind position < cap_out.
//   label_profile_kernel   one wave per (model, feature) list of the feature-major codes of ops/feature_codes
//                          (col_ptr int64 [G, n + 1], row int32 / val fp32 [G, cap], rows ascending in a list)
//                          over M rows with the labels lab int32 [M], non-decreasing.  Equal labels are then
//                          adjacent in every list; a maximal stretch of entries with one label is a RUN.
//       per run     count int32, max fp32, sum fp64: acc = acc + (double)val from 0.0 over the run's entries
//                   in list order (strictly sequential: not strided over lanes, not a tree)
//       per list    n_entries int64, n_labels int32 (runs), count_sq int64 (sum of count^2), total fp64:
//                   acc = acc + sum_run from 0.0 over the runs in list order
//       top m       the m best runs (1 <= m <= 64, one slot per lane): RANK 0 by the sum (codes are positive: the
//                   fp64 bits order as unsigned integers) descending, RANK 1 by the count descending, then the
//                   label ascending; label / count / sum / max of all m slots are written, empty slots read
//                   (-1, 0, 0.0, 0.0).
//
// A pass takes 64 entries (one per lane) and their labels.  The run heads of the pass come from a ballot of
// "my label differs from that of the valid entry before me" (before lane 0: the run left open by the pass
// before).  The set bits of heads | 1 cut the pass into at most 64 segments; lane k owns the k-th and adds its
// entries one after another out of the other lanes' registers (ds_bpermute with a per-lane index), so every sum
// is sequential while the segments of a pass proceed side by side.  Segment 0 continues the open run unless lane
// 0 is a head; the last segment stays open and is carried, wave-uniform, into the next pass.  Finished runs are
// added to `total` and offered to the sorted winners in list order through a wave-uniform loop over a ballot.
// Loads run two passes ahead (row, code) and one pass ahead (label).
//
// Guards: list bounds are clipped to [0, cap]; an entry whose row lies outside [0, M) is skipped (it is in no
// run and in no count); a `lab` that is not sorted only gives more runs.  No LDS, no floating-point atomics;
// the bits do not depend on the launch geometry.  Every store sits behind its own bound.
//
// Known weak spot: a feature that fires on one label only is one lane adding its entries in sequence, and a
// feature that fires on every row is M sequential adds in one wave.
#include "code_lists.h"

namespace scamd {

constexpr int LP_WAVES = 4;  // waves per block
constexpr int LP_MAX_M = 64;

__global__ __launch_bounds__(64 * LP_WAVES) void csr_take_rows_kernel(
    const long* __restrict__ row_ptr, long ldp, long N, const int* __restrict__ col, const float* __restrict__ val,
    long cap_in, const long* __restrict__ index, long M, const long* __restrict__ out_ptr, int* __restrict__ ocol,
    float* __restrict__ oval, long cap_out, long work, int waves) {
  ListWalk w;  // id: (g, i) flattened
  if (!list_walk(w, work, waves)) return;
  const int lane = w.lane;
  const long g = w.id / M, i = w.id - g * M;
  const long r = index[i];
  if (r < 0 || r >= N) return;
  const long plo = row_ptr[g * ldp + r], phi = row_ptr[g * ldp + r + 1];
  if (plo < 0 || phi < plo || phi > cap_in) return;
  const long dst = out_ptr[g * (M + 1) + i];
  if (dst < 0) return;
  const long len = min(phi - plo, max(out_ptr[g * (M + 1) + i + 1] - dst, 0l));  // (never into the next row)
  col += g * cap_in + plo;
  val += g * cap_in + plo;
  for (long q = lane; q < len; q += 64) {
    const long pos = dst + q;
    if (pos < cap_out) {
      ocol[g * cap_out + pos] = col[q];
      oval[g * cap_out + pos] = val[q];
    }
  }
}

// Position of the k-th (from 0) set bit of `bits`; k < popcount(bits).
__device__ __forceinline__ int lp_select(unsigned long long bits, int k) {
  int pos = 0;
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    const int c = __popcll(bits & (((1ull << w) - 1ull) << pos));
    if (k >= c) {
      k -= c;
      pos += w;
    }
  }
  return pos;
}

struct LpRun {  // a run; as a slot of the sorted winners (one per lane, slots 0 .. m - 1) cnt == 0: empty
  int label;
  int cnt;
  float mx;
  double sum;
};

__device__ __forceinline__ double lp_readlane(double v, int i) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), i),
                          __builtin_amdgcn_readlane(__double2loint(v), i));
}

// Lane i's run in every lane (i wave-uniform).
__device__ __forceinline__ LpRun lp_bcast(const LpRun& r, int i) {
  LpRun x;
  x.label = __builtin_amdgcn_readlane(r.label, i);
  x.cnt = __builtin_amdgcn_readlane(r.cnt, i);
  x.mx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.mx), i));
  x.sum = lp_readlane(r.sum, i);
  return x;
}

// Does run x (cnt >= 1) rank before slot c?
template <int RANK>
__device__ __forceinline__ bool lp_beats(const LpRun& x, const LpRun& c) {
  if (c.cnt == 0) return true;
  if constexpr (RANK == 0) {
    const unsigned long long px = (unsigned long long)__double_as_longlong(x.sum);
    const unsigned long long pc = (unsigned long long)__double_as_longlong(c.sum);
    return px > pc || (px == pc && x.label < c.label);
  } else {
    return x.cnt > c.cnt || (x.cnt == c.cnt && x.label < c.label);
  }
}

// Insert the wave-uniform run x into the K sorted slots; one that does not beat slot K - 1 changes nothing.
template <int RANK>
__device__ __forceinline__ void insert_run(LpRun& cur, const LpRun& x, int K, int lane) {
  const int pos = insert_pos(!lp_beats<RANK>(x, cur), K);  // (the slots that stay ahead: a prefix)
  insert_take(cur.label, x.label, pos, K, lane);  // (field by field: a select between whole structs goes
  insert_take(cur.cnt, x.cnt, pos, K, lane);      // through memory)
  insert_take(cur.mx, x.mx, pos, K, lane);
  insert_take(cur.sum, x.sum, pos, K, lane);
}

// A finished wave-uniform run: into the totals, and into the winners if it beats slot m - 1.
template <int RANK>
__device__ __forceinline__ void lp_finish(const LpRun& x, LpRun& top, double& tot, int& nl, long& csq, int m,
                                          int lane) {
  tot = tot + x.sum;
  nl += 1;
  if (lane == 0) csq += (long)x.cnt * x.cnt;
  if (lp_beats<RANK>(x, lp_bcast(top, m - 1))) insert_run<RANK>(top, x, m, lane);
}

__device__ __forceinline__ int lp_label(const int* __restrict__ lab, int r, int M) {
  return (unsigned)r < (unsigned)M ? lab[r] : 0;
}

template <int RANK>
__global__ __launch_bounds__(64 * LP_WAVES) void label_profile_kernel(
    const long* __restrict__ col_ptr, const int* __restrict__ row, const float* __restrict__ val, long cap, long lists,
    int n, const int* __restrict__ lab, int M, int m, int waves, long* __restrict__ n_entries,
    int* __restrict__ n_labels, long* __restrict__ count_sq, double* __restrict__ total, int* __restrict__ top_label,
    int* __restrict__ top_count, double* __restrict__ top_sum, float* __restrict__ top_max) {
  ListWalk w;
  if (!list_walk(w, lists, waves)) return;
  w.split(n);
  const int lane = w.lane, g = w.g;
  const long id = w.id;
  long lo, hi;
  list_bounds(col_ptr + (long)g * (n + 1), w.f, cap, lo, hi);
  row += (long)g * cap;
  val += (long)g * cap;

  LpRun top;  // the winners, one slot per lane
  top.label = -1;
  top.cnt = 0;
  top.mx = 0.f;
  top.sum = 0.0;
  LpRun open;  // the run the last pass left open (wave-uniform; cnt == 0: none)
  open.label = 0;
  open.cnt = 0;
  open.mx = -INFINITY;
  open.sum = 0.0;
  long ne = 0;        // valid entries (wave-uniform)
  int nl = 0;         // finished runs (wave-uniform)
  long csq = 0;       // count^2 of the runs this lane finished
  double tot = 0.0;   // sum of the finished runs, in list order (wave-uniform)

  int r0, r1, r2, l0, l1;
  float v0, v1, v2;
  list_load(row, val, lo, hi, lane, r0, v0);
  list_load(row, val, lo + 64, hi, lane, r1, v1);
  l0 = lp_label(lab, r0, M);
  for (long b = lo; b < hi; b += 64) {
    l1 = lp_label(lab, r1, M);
    list_load(row, val, b + 128, hi, lane, r2, v2);

    const bool valid = (unsigned)r0 < (unsigned)M;
    const unsigned long long vmask = __ballot(valid);
    if (vmask != 0ull) {
      ne += __popcll(vmask);
      const unsigned long long below = vmask & ((1ull << lane) - 1ull);  // the valid entries before mine
      const int prev = __shfl(l0, below ? 63 - __clzll((long long)below) : 0, 64);
      const bool head = valid && (below ? l0 != prev : (open.cnt == 0 || l0 != open.label));
      const unsigned long long heads = __ballot(head);
      const unsigned long long cuts = heads | 1ull;
      const int ns = __popcll(cuts);               // segments of this pass, 1 .. 64
      const bool cont = (heads & 1ull) == 0ull;    // segment 0 continues the open run
      if (!cont && open.cnt > 0) lp_finish<RANK>(open, top, tot, nl, csq, m, lane);

      const int s = lane < ns ? lp_select(cuts, lane) : 64;  // my segment: entries [s, e) of the pass
      int e = __shfl_down(s, 1, 64);
      if (lane == 63) e = 64;
      LpRun me;
      me.label = __shfl(l0, s & 63, 64);
      me.cnt = 0;
      me.mx = -INFINITY;
      me.sum = 0.0;
      if (cont && lane == 0) me = open;
      for (int t = 0; __ballot(s + t < e) != 0ull; t += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = s + t + u;
          const float x = __shfl(v0, j & 63, 64);
          const bool ok = j < e && ((vmask >> (j & 63)) & 1ull) != 0ull;
          me.sum = ok ? me.sum + (double)x : me.sum;
          me.mx = ok ? fmaxf(me.mx, x) : me.mx;
          me.cnt += ok ? 1 : 0;
        }
      }

      // segments 0 .. ns - 2 are finished runs (an empty one is none), segment ns - 1 stays open
      const bool done = lane < ns - 1 && me.cnt > 0;
      const unsigned long long fin = __ballot(done);
      nl += __popcll(fin);
      if (done) csq += (long)me.cnt * me.cnt;
      for (unsigned long long todo = fin; todo;) {
        const int i = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        todo &= todo - 1ull;
        tot = tot + lp_readlane(me.sum, i);
      }
      // (slot m - 1 only gets harder to beat: a run that does not beat it now never enters)
      for (unsigned long long todo = fin & __ballot(lp_beats<RANK>(me, lp_bcast(top, m - 1))); todo;) {
        const int i = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        todo &= todo - 1ull;
        insert_run<RANK>(top, lp_bcast(me, i), m, lane);
      }
      open = lp_bcast(me, ns - 1);
    }
    r0 = r1;
    v0 = v1;
    l0 = l1;
    r1 = r2;
    v1 = v2;
  }
  if (open.cnt > 0) lp_finish<RANK>(open, top, tot, nl, csq, m, lane);

  csq = wave_sum_xor<true>(csq);  // (integers: any order)
  if (lane == 0) {
    n_entries[id] = ne;
    n_labels[id] = nl;
    count_sq[id] = csq;
    total[id] = tot;
  }
  if (lane < m) {
    const long o = id * m + lane;
    const bool live = top.cnt > 0;
    top_label[o] = live ? top.label : -1;
    top_count[o] = live ? top.cnt : 0;
    top_sum[o] = live ? top.sum : 0.0;
    top_max[o] = live ? top.mx : 0.f;
  }
}

}  // namespace scamd

using namespace scamd;

extern "C" {

// Rows index[0 .. M) (int64, each in [0, N)) of the CSR codes row_ptr int64 [G, ldp] / col int32 / val fp32
// [G, cap_in], copied to ocol / oval [G, cap_out] at out_ptr int64 [G, M + 1] (the cumsum of the gathered row
// lengths).  waves: waves per block, 1 .. 4.
int sc_csr_take_rows(const long* row_ptr, const int* col, const float* val, const long* index, const long* out_ptr,
                     int* ocol, float* oval, int G, long N, long ldp, long cap_in, long M, long cap_out, int waves,
                     hipStream_t stream) {
  if (!row_ptr || !col || !val || !index || !out_ptr || !ocol || !oval) return 1;
  if (G < 1 || N < 1 || ldp < N + 1 || cap_in < 1 || M < 1 || cap_out < 1 || waves < 1 || waves > LP_WAVES) return 1;
  const long work = (long)G * M;
  unsigned blocks;
  if (!sc_grid(work, waves, blocks)) return 1;
  hipLaunchKernelGGL(csr_take_rows_kernel, dim3(blocks), dim3(64 * waves), 0, stream, row_ptr, ldp, N, col,
                     val, cap_in, index, M, out_ptr, ocol, oval, cap_out, work, waves);
  return sc_launched();
}

// The label profile of every (g, f) list of the feature-major codes (col_ptr int64 [G, n + 1], row int32 / val
// fp32 [G, cap]) over M rows labelled lab int32 [M] (non-decreasing): n_entries int64, n_labels int32, count_sq
// int64, total fp64, [G, n] each, and the m best runs top_label int32, top_count int32, top_sum fp64, top_max
// fp32, [G, n, m] each.  rank: 0 by the sum, 1 by the count.  waves: waves per block, 1 .. 4.
int sc_label_profile(const long* col_ptr, const int* row, const float* val, const int* lab, long* n_entries,
                     int* n_labels, long* count_sq, double* total, int* top_label, int* top_count, double* top_sum,
                     float* top_max, int G, int n, long cap, long M, int m, int rank, int waves, hipStream_t stream) {
  if (!col_ptr || !row || !val || !lab || !n_entries || !n_labels || !count_sq || !total || !top_label ||
      !top_count || !top_sum || !top_max)
    return 1;
  if (G < 1 || n < 1 || cap < 0 || cap > 0x7fffffffL || M < 1 || M > 0x7fffffffL || m < 1 || m > LP_MAX_M ||
      rank < 0 || rank > 1 || waves < 1 || waves > LP_WAVES)
    return 1;
  const long lists = (long)G * n;
  unsigned blocks;
  if (!sc_grid(lists, waves, blocks)) return 1;
  const dim3 grid(blocks), block(64 * waves);
  if (rank == 0)
    hipLaunchKernelGGL(label_profile_kernel<0>, grid, block, 0, stream, col_ptr, row, val, cap, lists, n, lab, (int)M,
                       m, waves, n_entries, n_labels, count_sq, total, top_label, top_count, top_sum, top_max);
  else
    hipLaunchKernelGGL(label_profile_kernel<1>, grid, block, 0, stream, col_ptr, row, val, cap, lists, n, lab, (int)M,
                       m, waves, n_entries, n_labels, count_sq, total, top_label, top_count, top_sum, top_max);
  return sc_launched();
}

}  // extern "C"
