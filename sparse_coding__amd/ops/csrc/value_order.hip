// Value-ordered feature lists and the exact AUROC of every (feature, concept) pair from them (gfx950).
//
//   list_sort_kernel    one wave per (model, feature) list of the feature-major codes of ops/feature_codes
//                       (col_ptr int64 [G, n + 1], row int32 / val fp32 [G, cap], rows ascending in a list): the
//                       list ordered by KEY ascending, then row ascending, written to vrow / vval [G, cap_out]
//                       at the list's own positions.  KEY is the order-preserving map of the fp32 bit pattern
//                       (order_key of common.h): a total order on all bit patterns, so -0.0 sorts before
//                       +0.0 and every NaN has its place.  Rows are distinct in a list and the sort is stable on
//                       an input with ascending rows: the output is unique, whatever the launch geometry.
//       L <= 64     a rank sort in registers: every lane counts the entries that go before its own.
//       L > 64      an LSD radix sort with 8-bit digits.  One walk fills the four 256-bin digit histograms of
//                   the list in LDS (4 KiB per wave, integer LDS adds).  A digit whose histogram has one
//                   non-empty bin orders nothing and is skipped: for bf16-valued codes the two low digits are
//                   constant and at most two passes run; for equal codes none does and the list is copied.  A
//                   pass takes 64 entries at a time: a lane's rank among the equal digits of its chunk is the
//                   popcount below its lane of a mask built from eight ballots, the running base of every digit
//                   stays in LDS (its exclusive scan, advanced by the highest lane of every group), so equal
//                   digits keep their order.  The passes alternate between the output and the scratch pairs
//                   (tmp int32 [G, cap, 2]: row, code bits) so that the last lands in the output; the number
//                   of passes is known after the histogram walk.
//   list_auroc_kernel   one wave per value-ordered list and K <= 32 concepts, flags int32 [N]: bit k of
//                       flags[r] says that row r is a positive of concept k.  LANE k KEEPS CONCEPT k: the wave
//                       walks the entries in order (64 loaded at a time, broadcast one by one), a tie run is a
//                       maximal stretch of entries with equal fp32 values, and a finished run with p positives
//                       and q negatives after nb negatives adds p (2 nb + q) to u2.  Integer sums in list
//                       order: the same bits in every run and under every geometry.  pos_in int32 / u2 int64
//                       [G, n, K], every slot written.
//
// Guards: a list is [lo, hi) with lo = clamp(col_ptr[f], 0, lim) and hi = clamp(col_ptr[f + 1], lo, lim), lim
// = min(cap, cap_out) for the sort and cap for the walk: every load and store sits inside the buffers whatever
// the pointers hold, entries at positions >= lim are left out, and positions in no list are not written (the
// tail keeps what the front-end put there).  Lists must not overlap for the sort's result to be defined: the
// front-end passes the running maximum of the clipped pointers.  An entry whose row lies outside [0, N) is in no
// run and in no count of the walk.  The sort's input must not alias its output or the scratch.  No floating-point
// arithmetic at all in the sort, integer sums only in the walk; nothing synchronises.
//
// Known weak spot: one wave per list whatever its length.  A feature that fires on every row is one wave walking
// N entries once per executed pass (at most five times) in the sort and once, entry by entry, in the AUROC walk;
// a block-wide path for long lists is not built.
#include "code_lists.h"

namespace scamd {

constexpr int VO_WAVES = 4;   // waves per block
constexpr int VO_MAX_K = 32;  // concepts per flag word

// list_bounds with provably wave-uniform results.
__device__ __forceinline__ void vo_bounds(const long* __restrict__ cp, int f, long lim, long& lo, long& hi) {
  list_bounds(cp, f, lim, lo, hi);
  lo = __builtin_amdgcn_readfirstlane((int)lo);  // (lim < 2^31; wave-uniform: the loops below branch in scalars)
  hi = __builtin_amdgcn_readfirstlane((int)hi);
}

// Where a pass reads from or writes to: separate row / code-bit arrays, or (row, code bits) pairs.
struct VoBuf {
  int* row;
  uint32_t* bits;
  int2* pair;  // non-null: the pairs are used
};

__device__ __forceinline__ void vo_read(const VoBuf& s, long e, int& r, uint32_t& b) {
  if (s.pair) {
    const int2 p = s.pair[e];
    r = p.x;
    b = (uint32_t)p.y;
  } else {
    r = s.row[e];
    b = s.bits[e];
  }
}

__device__ __forceinline__ void vo_write(const VoBuf& d, long e, int r, uint32_t b) {
  if (d.pair) {
    d.pair[e] = make_int2(r, (int)b);
  } else {
    d.row[e] = r;
    d.bits[e] = b;
  }
}

__global__ __launch_bounds__(64 * VO_WAVES) void list_sort_kernel(
    const long* __restrict__ col_ptr, const int* row, const uint32_t* val, long cap, long lim, long lists, int n,
    int waves, int* vrow, uint32_t* vval, long cap_out, int2* tmp) {
  __shared__ uint32_t hist_all[VO_WAVES][4][256];
  ListWalk w;
  if (!list_walk(w, lists, waves)) return;
  w.split(n);
  const int lane = w.lane, wave = w.wave, g = w.g;
  long lo, hi;
  vo_bounds(col_ptr + (long)g * (n + 1), w.f, lim, lo, hi);
  const long L = hi - lo;
  if (L <= 0) return;
  const VoBuf in = {const_cast<int*>(row) + (long)g * cap, const_cast<uint32_t*>(val) + (long)g * cap, nullptr};
  const VoBuf out = {vrow + (long)g * cap_out, vval + (long)g * cap_out, nullptr};
  const VoBuf scr = {nullptr, nullptr, tmp + (long)g * cap};

  if (L <= 64) {  // rank sort in registers
    int r = 0;
    uint32_t b = 0, key = 0;
    if (lane < L) {
      vo_read(in, lo + lane, r, b);
      key = order_key(b);
    }
    int rank = 0;
    for (int j = 0; j < (int)L; ++j) {
      const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)key, j);
      rank += (kj < key || (kj == key && j < lane)) ? 1 : 0;
    }
    if (lane < L && rank < L) vo_write(out, lo + rank, r, b);
    return;
  }

  uint32_t(*hist)[256] = hist_all[wave];
  for (int i = lane; i < 4 * 256; i += 64) (&hist[0][0])[i] = 0u;
  for (long e = lo + lane; e < hi; e += 64) {
    const uint32_t key = order_key(in.bits[e]);
    atomicAdd(&hist[0][key & 255u], 1u);
    atomicAdd(&hist[1][(key >> 8) & 255u], 1u);
    atomicAdd(&hist[2][(key >> 16) & 255u], 1u);
    atomicAdd(&hist[3][key >> 24], 1u);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  int act = 0;  // digits that order something
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    bool full = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) full |= hist[d][lane * 4 + q] == (uint32_t)L;
    if (__ballot(full) == 0ull) act |= 1 << d;
  }
  const int npass = __popc(act);
  if (npass == 0) {  // equal keys: the input's order is the answer
    for (long e = lo + lane; e < hi; e += 64) vo_write(out, e, in.row[e], in.bits[e]);
    return;
  }

  VoBuf src = in;
  int k = 0;
  for (int d = 0; d < 4; ++d) {
    if (!((act >> d) & 1)) continue;
    {  // exclusive scan of the digit's histogram, in place: lane i owns bins 4 i .. 4 i + 3
      uint32_t c[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) c[q] = hist[d][lane * 4 + q];
      const uint32_t own = c[0] + c[1] + c[2] + c[3];
      uint32_t incl = own;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      uint32_t run = incl - own;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        hist[d][lane * 4 + q] = run;
        run += c[q];
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    const VoBuf dst = ((npass - 1 - k) & 1) ? scr : out;  // (the last pass lands in the output)
    const int shift = 8 * d;
    int r1 = 0;
    uint32_t b1 = 0;
    if (lo + lane < hi) vo_read(src, lo + lane, r1, b1);
    for (long b = lo; b < hi; b += 64) {
      const int r0 = r1;
      const uint32_t b0 = b1;
      const bool valid = b + lane < hi;
      if (b + 64 + lane < hi) vo_read(src, b + 64 + lane, r1, b1);  // (the next chunk, while this one is ranked)
      const uint32_t dg = (order_key(b0) >> shift) & 255u;
      unsigned long long peers = __ballot(valid);
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const bool mine = (dg >> bit) & 1u;
        const unsigned long long m = __ballot(mine);
        peers &= mine ? m : ~m;
      }
      const int rank = __popcll(peers & ((1ull << lane) - 1ull));
      uint32_t base = 0;
      if (valid) base = hist[d][dg];
      __builtin_amdgcn_wave_barrier();
      if (valid && (peers >> lane) == 1ull) hist[d][dg] = base + (uint32_t)__popcll(peers);  // (the group's last lane)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      const long pos = lo + (long)base + rank;
      if (valid && pos < hi) vo_write(dst, pos, r0, b0);
    }
    __threadfence_block();  // (the next pass reads what other lanes of this wave wrote)
    src = dst;
    ++k;
  }
}

__device__ __forceinline__ uint32_t vo_flags(const int* __restrict__ flags, int r, int N) {
  return (unsigned)r < (unsigned)N ? (uint32_t)flags[r] : 0u;
}

__global__ __launch_bounds__(64 * VO_WAVES) void list_auroc_kernel(
    const long* __restrict__ col_ptr, const int* __restrict__ row, const float* __restrict__ val, long cap, long lists,
    int n, const int* __restrict__ flags, int N, int K, int waves, int* __restrict__ pos_in, long* __restrict__ u2) {
  ListWalk w;
  if (!list_walk(w, lists, waves)) return;
  w.split(n);
  const int lane = w.lane, g = w.g;
  const long id = w.id;
  long lo, hi;
  vo_bounds(col_ptr + (long)g * (n + 1), w.f, cap, lo, hi);
  row += (long)g * cap;
  val += (long)g * cap;

  // concept `lane`: positives so far, negatives before the open run, the open run's positives and negatives
  int pos = 0, nb = 0, rp = 0, rn = 0;
  long acc = 0;
  bool have = false;  // (wave-uniform) a valid entry was seen: `last` is its value
  float last = 0.f;

  int r0, r1, r2;
  float v0, v1, v2;
  uint32_t w0, w1;
  list_load(row, val, lo, hi, lane, r0, v0);
  list_load(row, val, lo + 64, hi, lane, r1, v1);
  w0 = vo_flags(flags, r0, N);
  for (long b = lo; b < hi; b += 64) {
    w1 = vo_flags(flags, r1, N);
    list_load(row, val, b + 128, hi, lane, r2, v2);
    unsigned long long todo = __ballot((unsigned)r0 < (unsigned)N);
    while (todo) {
      const int j = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
      todo &= todo - 1ull;
      const float vj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v0), j));
      const uint32_t wj = (uint32_t)__builtin_amdgcn_readlane((int)w0, j);
      if (!have || !(vj == last)) {  // a new run: the open one is finished
        acc += (long)rp * (2l * nb + rn);
        nb += rn;
        rp = 0;
        rn = 0;
      }
      have = true;
      last = vj;
      const int bit = (int)((wj >> (lane & 31)) & 1u);
      rp += bit;
      rn += 1 - bit;
      pos += bit;
    }
    r0 = r1;
    v0 = v1;
    w0 = w1;
    r1 = r2;
    v1 = v2;
  }
  acc += (long)rp * (2l * nb + rn);
  if (lane < K) {
    pos_in[id * K + lane] = pos;
    u2[id * K + lane] = acc;
  }
}

}  // namespace scamd

using namespace scamd;

extern "C" {

// Every (g, f) list of the feature-major codes (col_ptr int64 [G, n + 1], row int32 / val fp32 [G, cap]) ordered
// by the key of its codes, then by row, into vrow / vval [G, cap_out] at the same positions; positions >=
// min(cap, cap_out) are left out and positions in no list are not written.  tmp: int32 [G, cap, 2] scratch.
// waves: waves per block, 1 .. 4.
int sc_list_sort_by_value(const long* col_ptr, const int* row, const float* val, int* vrow, float* vval, int* tmp,
                          int G, int n, long cap, long cap_out, int waves, hipStream_t stream) {
  if (!col_ptr || !row || !val || !vrow || !vval || !tmp) return 1;
  if (G < 1 || n < 1 || cap < 1 || cap > 0x7fffffffL || cap_out < 1 || cap_out > 0x7fffffffL || waves < 1 ||
      waves > VO_WAVES)
    return 1;
  if ((const void*)row == (const void*)vrow || (const void*)val == (const void*)vval) return 1;
  const long lists = (long)G * n;
  unsigned blocks;
  if (!sc_grid(lists, waves, blocks)) return 1;
  hipLaunchKernelGGL(list_sort_kernel, dim3(blocks), dim3(64 * waves), 0, stream, col_ptr, row,
                     (const uint32_t*)val, cap, min(cap, cap_out), lists, n, waves, vrow, (uint32_t*)vval, cap_out,
                     (int2*)tmp);
  return sc_launched();
}

// One walk per value-ordered list (col_ptr int64 [G, n + 1], vrow int32 / vval fp32 [G, cap]) against flags int32
// [N] holding K <= 32 concepts: pos_in int32 and u2 int64, [G, n, K] each.  waves: waves per block, 1 .. 4.
int sc_list_auroc(const long* col_ptr, const int* vrow, const float* vval, const int* flags, int* pos_in, long* u2,
                  int G, int n, long cap, long N, int K, int waves, hipStream_t stream) {
  if (!col_ptr || !vrow || !vval || !flags || !pos_in || !u2) return 1;
  if (G < 1 || n < 1 || cap < 0 || cap > 0x7fffffffL || N < 1 || N > 0x7fffffffL || K < 1 || K > VO_MAX_K ||
      waves < 1 || waves > VO_WAVES)
    return 1;
  const long lists = (long)G * n;
  unsigned blocks;
  if (!sc_grid(lists, waves, blocks)) return 1;
  hipLaunchKernelGGL(list_auroc_kernel, dim3(blocks), dim3(64 * waves), 0, stream, col_ptr, vrow, vval, cap,
                     lists, n, flags, (int)N, K, waves, pos_in, u2);
  return sc_launched();
}

}  // extern "C"
