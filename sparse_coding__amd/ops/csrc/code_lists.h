// What the kernels that walk sparse codes share: the per-model CSR of ops/sparse_codes (row_ptr int64, col int32,
// val fp32; one wave per row) and the feature-major lists of ops/feature_codes (col_ptr int64, row int32, val
// fp32; one wave per list).  The skip rule of a row, the clipping of list bounds and the insert into sorted
// winners are contracts: the oracles emulate them and the tests compare bits, so each is written here once.
#pragma once
#include "common.h"

namespace scamd {

// ------------------------------------------------------------------ CSR rows
// The columns a model may use: n, or min(n, nactive[g]) when the models carry an active width.
__device__ __forceinline__ int live_limit(const int* __restrict__ nactive, long g, int n) {
  int lim = n;
  if (nactive) lim = min(n, max(0, nactive[g]));
  return lim;
}

// The skip rule (wave-uniform result): row [lo, hi) is used only if its pointers are ordered inside [0, cap],
// it has at most n entries and every column lies in [0, lim).  `col` is the model's column array; all columns
// are checked before any is used as an index.
__device__ __forceinline__ bool csr_row_ok(long lo, long hi, long cap, int n, int lim, const int* __restrict__ col,
                                           int lane) {
  bool ok = lo >= 0 && hi >= lo && hi <= cap && hi - lo <= (long)n;
  if (ok) {
    bool bad = false;
    for (long e = lo + lane; e < hi; e += 64) {
      const int j = col[e];
      bad |= (j < 0) | (j >= lim);
    }
    ok = __ballot(bad) == 0ull;
  }
  return ok;
}

// ------------------------------------------------------------------ feature-major lists
// The stored part [lo, hi) of list f of a model whose pointers are `cp` (0 <= lo <= hi <= cap whatever they hold).
__device__ __forceinline__ void list_bounds(const long* __restrict__ cp, int f, long cap, long& lo, long& hi) {
  lo = min(max(cp[f], 0l), cap);
  hi = min(max(cp[f + 1], lo), cap);
}

// Entry b + lane of a list that ends at hi: (row, code), or (-1, 0) past the end (row -1 is no valid row).
__device__ __forceinline__ void list_load(const int* __restrict__ row, const float* __restrict__ val, long b, long hi,
                                          int lane, int& r, float& v) {
  r = -1;
  v = 0.f;
  if (b + lane < hi) {
    r = row[b + lane];
    v = val[b + lane];
  }
}

// The list of this wave in a launch of one wave per list: `id` counts the lists of the whole launch; split(n)
// gives (g, f) for lists numbered g n + f (a kernel that numbers them otherwise splits `id` itself).
struct ListWalk {
  int lane, wave;
  long id;
  int g, f;
  __device__ __forceinline__ void split(int n) {
    g = (int)(id / n);
    f = (int)(id - (long)g * n);
  }
};

// The preamble of a kernel whose blocks always have WAVES waves: false when this wave's id lies past `lists`.
template <int WAVES>
__device__ __forceinline__ bool list_walk(ListWalk& w, long lists) {
  static_assert(WAVES >= 1 && WAVES <= 16, "waves per block");
  w.lane = threadIdx.x & 63;
  w.wave = threadIdx.x >> 6;
  w.id = (long)blockIdx.x * WAVES + w.wave;
  return w.id < lists;
}

// The preamble of a kernel that takes the waves per block as an argument (its blocks may be launched larger than
// the waves it uses): false for a wave past `waves` or an id past `lists`.  `wave` is provably wave-uniform.
__device__ __forceinline__ bool list_walk(ListWalk& w, long lists, int waves) {
  w.lane = threadIdx.x & 63;
  w.wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w.wave >= waves) return false;
  w.id = (long)blockIdx.x * waves + w.wave;
  return w.id < lists;
}

// ------------------------------------------------------------------ sorted winners, one slot per lane
// K slots (1 <= K <= 64) in lanes 0 .. K - 1, best first.  A wave-uniform candidate goes in at the number of
// slots that stay ahead of it (`ahead`, this lane's verdict on its own slot: a prefix of the slots); a position
// of K means that it does not beat slot K - 1.
__device__ __forceinline__ int insert_pos(bool ahead, int K) {
  const unsigned long long kmask = K >= 64 ? ~0ull : (1ull << K) - 1ull;
  return __popcll(__ballot(ahead) & kmask);
}

// One field of the slots after the insert at `pos`: lane pos takes x, the lanes behind it their neighbour's,
// and pos >= K changes nothing.  Slots of several fields call this once per field (a select between whole
// structs goes through memory).
template <class T>
__device__ __forceinline__ void insert_take(T& cur, T x, int pos, int K, int lane) {
  const T up = __shfl_up(cur, 1, 64);
  if (pos < K) cur = lane == pos ? x : lane > pos ? up : cur;
}

}  // namespace scamd
