// Feature-major sparse codes and per-feature example fragments (gfx950).
//
// Input is the per-model CSR of ops/sparse_codes: row_ptr int64 [G, ldp], col int32 [G, cap], val fp32 [G, cap].
// The transposition writes col_ptr-ordered lists (row int32 [G, ocap], val fp32 [G, ocap]): the list of feature
// f of model g holds the rows on which f fires, ROWS ASCENDING, with their codes.  Three launches, none of which
// waits for another block:
//
//   fc_count_kernel    cnt[g, s, f] += entries of feature f in the rows of segment s (segments of 2^seg_shift
//                      rows; a block takes `rpb` rows of one segment, one wave per row).  With LDSH the block
//                      counts into an LDS histogram of n bins and adds every non-empty bin once; without it
//                      (n above the width limit) every entry is one global integer add.  Integer adds commute:
//                      the counts are exact whatever the order.
//   (host, torch)      col_ptr = cumsum of the per-feature totals; base[g, s, f] = col_ptr[g, f] + the entries
//                      of f in the segments before s: where sub-list (g, f, s) starts.  Device-side cumsums.
//   fc_scatter_kernel  the same walk; a block reserves its range of every sub-list it adds to with one integer
//                      add on cur[g, s, f] per non-empty bin (LDSH) or per entry, and stores (row, val) as ONE
//                      8-byte element at base + reserved position in a temporary buffer.  Order INSIDE a
//                      sub-list is arbitrary.
//   fc_order_kernel    one wave per sub-list: a row occurs at most once in a list and lies in the segment's
//                      window, so a presence bitmap of 2^seg_shift bits in LDS, the prefix sum of its word
//                      popcounts and rank = bits below my row give every entry its final position.  The output
//                      depends only on the SET of entries of the sub-list: the same bits every run and for any
//                      segment size, rows per block or histogram path.
//
// Skip rule (that of sc_active_capacity / sc_recon_*): a row is left out whole -- and counted in skipped[g] by
// the count kernel -- unless 0 <= row_ptr[r] <= row_ptr[r + 1] <= cap, L <= n and every column is in [0, lim),
// lim = n or min(n, nactive[g]).  All columns of a row are checked before any is used as an index, in both
// walks.  Every store sits behind its own bound (bin < n, position < tcap / ocap): with undersized buffers
// entries are dropped, nothing is written outside.  Only integer atomics.
//
//   fragment_examples_kernel   one wave per (model, feature) list, walked once in row order, 64 entries per load.
//                      Fragment of a row = row / L.  A fragment's entries are contiguous; the open run (fragment,
//                      running maximum) is carried across loads.  Every closed run is a candidate for two sorted
//                      lists kept one slot per lane: the Kt largest keys (float bits of the maximum << 32 |
//                      0xFFFFFFFF - fragment: maximum descending, then fragment ascending -- positive floats order
//                      as unsigned integers) and the Kr smallest keys mix32(h0 ^ fragment) << 32 | fragment,
//                      h0 = mix32(seed + 0x9E3779B9 (g n + f + 1)).  A candidate that beats the K-th slot is
//                      inserted with one ballot and one shuffle.  Empty slots read (-1, 0.0) / -1.
//   fragment_acts_kernel       one wave per (model, feature, slot): the L codes of the feature on the rows of
//                      fragment frags[g, f, k], 0 where it does not fire, all zeros for a slot outside
//                      [0, n_frags).  A wave-uniform binary search finds the fragment's first entry, a per-lane
//                      search over the next <= L entries the row of each output.  Every element is written.
#include "code_lists.h"

namespace scamd {

constexpr int FC_WAVES = 4;            // waves per block, all kernels
constexpr int FC_MAX_LDS_BINS = 16384;  // 64 KiB of int32 bins: the largest LDS histogram a launch may ask for
constexpr int FC_MAX_SEG_SHIFT = 13;    // segments of at most 8192 rows (2 KiB of bitmap and prefix per wave)

struct FcWalk {  // what a block of the two row walks works on
  int g, s;
  long r0, r1;
  int lim;
};

__device__ __forceinline__ FcWalk fc_walk(long N, int n, int seg_shift, int rpb, int bps,
                                          const int* __restrict__ nactive) {
  FcWalk w;
  w.g = blockIdx.y;
  w.s = blockIdx.x / bps;
  w.r0 = ((long)w.s << seg_shift) + (long)(blockIdx.x % bps) * rpb;
  w.r1 = min(w.r0 + rpb, N);
  w.lim = live_limit(nactive, w.g, n);
  return w;
}

template <bool LDSH>
__global__ __launch_bounds__(64 * FC_WAVES) void fc_count_kernel(
    const long* __restrict__ row_ptr, long ldp, long N, const int* __restrict__ col, long cap,
    const int* __restrict__ nactive, int n, int seg_shift, int S, int rpb, int bps, int* __restrict__ cnt,
    unsigned long long* __restrict__ skipped) {
  extern __shared__ int fc_hist[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const FcWalk w = fc_walk(N, n, seg_shift, rpb, bps, nactive);
  if constexpr (LDSH) {
    for (int i = threadIdx.x; i < n; i += 64 * FC_WAVES) fc_hist[i] = 0;
    __syncthreads();
  }
  row_ptr += (long)w.g * ldp;
  col += (long)w.g * cap;
  int* gc = cnt + ((long)w.g * S + w.s) * n;
  for (long r = w.r0 + wave; r < w.r1; r += FC_WAVES) {
    const long lo = row_ptr[r], hi = row_ptr[r + 1];
    if (!csr_row_ok(lo, hi, cap, n, w.lim, col, lane)) {
      if (lane == 0) atomicAdd(skipped + w.g, 1ull);
      continue;
    }
    for (long e = lo + lane; e < hi; e += 64) {
      const int j = col[e];
      if ((unsigned)j < (unsigned)n) {
        if constexpr (LDSH) atomicAdd(&fc_hist[j], 1);
        else atomicAdd(&gc[j], 1);
      }
    }
  }
  if constexpr (LDSH) {
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 64 * FC_WAVES) {
      const int h = fc_hist[i];
      if (h) atomicAdd(&gc[i], h);
    }
  }
}

template <bool LDSH>
__global__ __launch_bounds__(64 * FC_WAVES) void fc_scatter_kernel(
    const long* __restrict__ row_ptr, long ldp, long N, const int* __restrict__ col, const float* __restrict__ val,
    long cap, const int* __restrict__ nactive, int n, int seg_shift, int S, int rpb, int bps,
    const long* __restrict__ base, int* __restrict__ cur, u32x2_t* __restrict__ tmp, long tcap) {
  extern __shared__ int fc_hist[];
  __shared__ unsigned char okf[256];  // (rpb <= 256) the skip rule's verdict on the block's rows
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const FcWalk w = fc_walk(N, n, seg_shift, rpb, bps, nactive);
  row_ptr += (long)w.g * ldp;
  col += (long)w.g * cap;
  val += (long)w.g * cap;
  tmp += (long)w.g * tcap;
  const long sub = ((long)w.g * S + w.s) * n;
  base += sub;
  cur += sub;
  if constexpr (LDSH) {
    for (int i = threadIdx.x; i < n; i += 64 * FC_WAVES) fc_hist[i] = 0;
    __syncthreads();
    for (long r = w.r0 + wave; r < w.r1; r += FC_WAVES) {
      const long lo = row_ptr[r], hi = row_ptr[r + 1];
      const bool ok = csr_row_ok(lo, hi, cap, n, w.lim, col, lane);
      if (lane == 0) okf[r - w.r0] = ok;
      if (!ok) continue;
      for (long e = lo + lane; e < hi; e += 64) {
        const int j = col[e];
        if ((unsigned)j < (unsigned)n) atomicAdd(&fc_hist[j], 1);
      }
    }
    __syncthreads();
    // reserve this block's range of every sub-list it adds to; the bin now holds the next free position
    for (int i = threadIdx.x; i < n; i += 64 * FC_WAVES) {
      const int h = fc_hist[i];
      fc_hist[i] = h ? atomicAdd(&cur[i], h) : 0;
    }
    __syncthreads();
  }
  for (long r = w.r0 + wave; r < w.r1; r += FC_WAVES) {
    const long lo = row_ptr[r], hi = row_ptr[r + 1];
    if constexpr (LDSH) {
      if (!okf[r - w.r0]) continue;
      if (!(lo >= 0 && hi >= lo && hi <= cap)) continue;  // (the verdict covered these pointers)
    } else {
      if (!csr_row_ok(lo, hi, cap, n, w.lim, col, lane)) continue;
    }
    for (long e = lo + lane; e < hi; e += 64) {
      const int j = col[e];
      if ((unsigned)j >= (unsigned)n) continue;
      int p;
      if constexpr (LDSH) p = atomicAdd(&fc_hist[j], 1);
      else p = atomicAdd(&cur[j], 1);
      const long pos = base[j] + p;
      if (p >= 0 && pos >= 0 && pos < tcap) {
        u32x2_t rv;
        rv[0] = (uint32_t)r;
        rv[1] = __float_as_uint(val[e]);
        tmp[pos] = rv;
      }
    }
  }
}

__global__ __launch_bounds__(64 * FC_WAVES) void fc_order_kernel(
    const int* __restrict__ cnt, const long* __restrict__ base, const u32x2_t* __restrict__ tmp, long tcap,
    int* __restrict__ orow, float* __restrict__ oval, long ocap,
    long lists, int n, int S, int seg_shift) {
  extern __shared__ uint32_t fc_bits[];  // per wave: W words of bitmap, W words of exclusive prefix
  ListWalk w;  // id: (g, s, f) flattened, as cnt and base
  if (!list_walk<FC_WAVES>(w, lists)) return;
  const int lane = w.lane, wave = w.wave;
  const long id = w.id;
  long len = cnt[id];
  const long start = base[id];
  if (len <= 0 || start < 0 || start >= tcap) return;
  len = min(len, tcap - start);  // (what the scatter could store)
  const int g = (int)(id / ((long)S * n)), s = (int)((id / n) % S);
  const int seg = 1 << seg_shift, W = seg >> 5;
  const long seg0 = (long)s << seg_shift;
  uint32_t* bm = fc_bits + wave * 2 * W;
  uint32_t* pre = bm + W;
  tmp += (long)g * tcap + start;
  orow += (long)g * ocap;
  oval += (long)g * ocap;
  for (int q = lane; q < W; q += 64) bm[q] = 0u;
  wave_sync();
  for (long i = lane; i < len; i += 64) {
    const long o = (long)(int)tmp[i][0] - seg0;
    if (o >= 0 && o < seg) atomicOr(&bm[o >> 5], 1u << (o & 31));
  }
  wave_sync();
  int carry = 0;
  for (int q0 = 0; q0 < W; q0 += 64) {
    const int q = q0 + lane;
    const int c = q < W ? __popc(bm[q]) : 0;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (q < W) pre[q] = (uint32_t)(carry + incl - c);
    carry += __shfl(incl, 63, 64);
  }
  wave_sync();
  for (long i = lane; i < len; i += 64) {
    const u32x2_t rv = tmp[i];
    const int r = (int)rv[0];
    const long o = (long)r - seg0;
    if (o < 0 || o >= seg) continue;
    const int rank = (int)pre[o >> 5] + __popc(bm[o >> 5] & ((1u << (o & 31)) - 1u));
    const long pos = start + rank;
    if (pos < ocap) {
      orow[pos] = r;
      oval[pos] = __uint_as_float(rv[1]);
    }
  }
}

// ------------------------------------------------------------------ example fragments
__device__ __forceinline__ uint32_t fc_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// Insert the wave-uniform key x into the sorted list held one slot per lane (slots 0 .. K-1; DESC: largest
// first).  Keys are distinct.  A key that does not beat slot K-1 changes nothing.
template <bool DESC>
__device__ __forceinline__ void insert_key(unsigned long long& cur, unsigned long long x, int K, int lane) {
  insert_take(cur, x, insert_pos(DESC ? cur > x : cur < x, K), K, lane);
}

__device__ __forceinline__ unsigned long long fc_top_key(float v, uint32_t frag) {
  return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xFFFFFFFFu - frag);
}

__device__ __forceinline__ unsigned long long fc_rnd_key(uint32_t h0, uint32_t frag) {
  return ((unsigned long long)fc_mix32(h0 ^ frag) << 32) | (unsigned long long)frag;
}

__global__ __launch_bounds__(64 * FC_WAVES) void fragment_examples_kernel(
    const long* __restrict__ col_ptr, const int* __restrict__ row, const float* __restrict__ val, long cap, int G,
    int n, uint32_t L, int Kt, int Kr, uint32_t seed, long* __restrict__ n_frags, int* __restrict__ top_frag,
    float* __restrict__ top_max, int* __restrict__ rand_frag) {
  ListWalk w;
  if (!list_walk<FC_WAVES>(w, (long)G * n)) return;
  w.split(n);
  const int lane = w.lane, g = w.g;
  const long id = w.id;
  long lo, hi;
  list_bounds(col_ptr + (long)g * (n + 1), w.f, cap, lo, hi);
  row += (long)g * cap;
  val += (long)g * cap;
  const uint32_t h0 = fc_mix32(seed + 0x9E3779B9u * (uint32_t)(id + 1));
  unsigned long long top = 0ull, rnd = ~0ull;
  long nfr = 0;
  bool open = false;
  uint32_t ofrag = 0;
  float omax = 0.f;
  auto single = [&](uint32_t fr, float v) {  // one closed run, wave-uniform
    ++nfr;
    if (Kt) insert_key<true>(top, fc_top_key(v, fr), Kt, lane);
    if (Kr) insert_key<false>(rnd, fc_rnd_key(h0, fr), Kr, lane);
  };
  for (long b = lo; b < hi; b += 64) {
    const int cnt = (int)min(64l, hi - b);
    const bool valid = lane < cnt;
    const uint32_t fr = valid ? (uint32_t)row[b + lane] / L : 0xFFFFFFFFu;
    float v = valid ? val[b + lane] : 0.f;
    // running maximum inside each run of equal fragments
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float u = __shfl_up(v, o, 64);
      const uint32_t fu = __shfl_up(fr, o, 64);
      if (lane >= o && fu == fr) v = fmaxf(v, u);
    }
    const uint32_t first = __shfl(fr, 0, 64);
    if (open) {
      if (ofrag == first) {
        if (fr == ofrag) v = fmaxf(v, omax);  // (the open run goes on)
      } else {
        single(ofrag, omax);
      }
    }
    const uint32_t nxt = __shfl_down(fr, 1, 64);
    const bool is_end = valid && lane < cnt - 1 && nxt != fr;
    nfr += __popcll(__ballot(is_end));
    if (Kt) {
      const unsigned long long k = fc_top_key(v, fr);
      const unsigned long long kth = __shfl(top, Kt - 1, 64);  // (read by all lanes, outside the && below)
      unsigned long long m = __ballot(is_end && k > kth);
      while (m) {
        const int i = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        insert_key<true>(top, __shfl(k, i, 64), Kt, lane);
      }
    }
    if (Kr) {
      const unsigned long long k = fc_rnd_key(h0, fr);
      const unsigned long long kth = __shfl(rnd, Kr - 1, 64);
      unsigned long long m = __ballot(is_end && k < kth);
      while (m) {
        const int i = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        insert_key<false>(rnd, __shfl(k, i, 64), Kr, lane);
      }
    }
    open = true;
    ofrag = __shfl(fr, cnt - 1, 64);
    omax = __shfl(v, cnt - 1, 64);
  }
  if (open) single(ofrag, omax);
  if (lane == 0) n_frags[id] = nfr;
  if (lane < Kt) {
    top_frag[id * Kt + lane] = (int)(0xFFFFFFFFu - (uint32_t)top);
    top_max[id * Kt + lane] = __uint_as_float((uint32_t)(top >> 32));
  }
  if (lane < Kr) rand_frag[id * Kr + lane] = (int)(uint32_t)rnd;
}

__global__ __launch_bounds__(64 * FC_WAVES) void fragment_acts_kernel(
    const long* __restrict__ col_ptr, const int* __restrict__ row, const float* __restrict__ val, long cap, int n,
    int f0, int nf, int K, int L, long nfrag, long slots, const int* __restrict__ frags, float* __restrict__ out) {
  ListWalk w;  // id: (g, f - f0, k) flattened
  if (!list_walk<FC_WAVES>(w, slots)) return;
  const int lane = w.lane;
  const long id = w.id;
  const int g = (int)(id / ((long)nf * K)), f = f0 + (int)((id / K) % nf);
  float* o = out + id * L;
  const long fr = frags[id];
  if (fr < 0 || fr >= nfrag) {
    for (int t = lane; t < L; t += 64) o[t] = 0.f;
    return;
  }
  long lo, hi;
  list_bounds(col_ptr + (long)g * (n + 1), f, cap, lo, hi);
  row += (long)g * cap;
  val += (long)g * cap;
  const long r0 = fr * L;
  long a = lo, b = hi;  // first entry with row >= r0 (the same search in every lane)
  while (a < b) {
    const long m = (a + b) >> 1;
    if ((long)row[m] < r0) a = m + 1;
    else b = m;
  }
  const long p0 = a, p1 = min(hi, p0 + L);
  for (int t = lane; t < L; t += 64) {
    const long want = r0 + t;
    long x = p0, y = p1;
    while (x < y) {
      const long m = (x + y) >> 1;
      if ((long)row[m] < want) x = m + 1;
      else y = m;
    }
    o[t] = (x < p1 && (long)row[x] == want) ? val[x] : 0.f;
  }
}

}  // namespace scamd

using namespace scamd;

static bool fc_bad_walk(const void* row_ptr, const void* col, int G, long N, int n, long ldp, long cap, int seg_shift,
                        int S, int rpb, int use_lds) {
  if (!row_ptr || !col || G < 1 || G > 65535 || n < 1 || N < 1 || N > 0x7fffffffL || ldp < N + 1 || cap < 0 ||
      cap > 0x7fffffffL)
    return true;
  if (seg_shift < 6 || seg_shift > FC_MAX_SEG_SHIFT || rpb < 1 || rpb > 256 || (rpb & (rpb - 1)) ||
      rpb > (1 << seg_shift))
    return true;
  if ((long)S != (N + (1l << seg_shift) - 1) >> seg_shift) return true;
  if (use_lds && n > FC_MAX_LDS_BINS) return true;
  return (long)S * ((1 << seg_shift) / rpb) > 0x7fffffffL;
}

extern "C" {

// cnt int32 [G, S, n] (zeroed by the caller) += the per-segment entry counts of every feature over the valid rows
// of the CSR (row_ptr int64 [G, ldp], col int32 [G, cap]); skipped int64 [G] += the rows the skip rule leaves out.
// Segments of 2^seg_shift rows, S of them; a block takes rpb rows (a power of two <= 256 and <= the segment).
int sc_feature_count(const long* row_ptr, const int* col, const int* nactive, int* cnt, void* skipped, int G, long N,
                     int n, long ldp, long cap, int seg_shift, int S, int rpb, int use_lds, hipStream_t stream) {
  if (fc_bad_walk(row_ptr, col, G, N, n, ldp, cap, seg_shift, S, rpb, use_lds) || !cnt || !skipped) return 1;
  const int bps = (1 << seg_shift) / rpb;
  const dim3 grid((unsigned)((long)S * bps), (unsigned)G);
  if (use_lds)
    hipLaunchKernelGGL(fc_count_kernel<true>, grid, dim3(64 * FC_WAVES), (size_t)n * sizeof(int), stream, row_ptr, ldp,
                       N, col, cap, nactive, n, seg_shift, S, rpb, bps, cnt,
                       reinterpret_cast<unsigned long long*>(skipped));
  else
    hipLaunchKernelGGL(fc_count_kernel<false>, grid, dim3(64 * FC_WAVES), 0, stream, row_ptr, ldp, N, col, cap, nactive,
                       n, seg_shift, S, rpb, bps, cnt, reinterpret_cast<unsigned long long*>(skipped));
  return sc_launched();
}

// The same walk: every entry of a valid row goes to tmp[g, base[g, s, f] + its reserved position], behind
// position < tcap.  base int64 [G, S, n]; cur int32 [G, S, n] zeroed by the caller; tmp [G, tcap] pairs of 32-bit
// words (row, float bits of val), 8-byte aligned.
int sc_feature_scatter(const long* row_ptr, const int* col, const float* val, const int* nactive, const long* base,
                       int* cur, void* tmp, int G, long N, int n, long ldp, long cap, long tcap,
                       int seg_shift, int S, int rpb, int use_lds, hipStream_t stream) {
  if (fc_bad_walk(row_ptr, col, G, N, n, ldp, cap, seg_shift, S, rpb, use_lds) || !val || !base || !cur || !tmp ||
      tcap < 0 || (reinterpret_cast<uintptr_t>(tmp) & 7))
    return 1;
  const int bps = (1 << seg_shift) / rpb;
  const dim3 grid((unsigned)((long)S * bps), (unsigned)G);
  if (use_lds)
    hipLaunchKernelGGL(fc_scatter_kernel<true>, grid, dim3(64 * FC_WAVES), (size_t)n * sizeof(int), stream, row_ptr,
                       ldp, N, col, val, cap, nactive, n, seg_shift, S, rpb, bps, base, cur,
                       reinterpret_cast<u32x2_t*>(tmp), tcap);
  else
    hipLaunchKernelGGL(fc_scatter_kernel<false>, grid, dim3(64 * FC_WAVES), 0, stream, row_ptr, ldp, N, col, val, cap,
                       nactive, n, seg_shift, S, rpb, bps, base, cur, reinterpret_cast<u32x2_t*>(tmp), tcap);
  return sc_launched();
}

// Every sub-list (g, s, f) of the temporary buffer, rows ascending, into (orow, oval) [G, ocap] behind position < ocap.
int sc_feature_order(const int* cnt, const long* base, const void* tmp, int* orow, float* oval,
                     int G, int n, int S, int seg_shift, long tcap, long ocap, hipStream_t stream) {
  if (!cnt || !base || !tmp || (reinterpret_cast<uintptr_t>(tmp) & 7) || !orow || !oval || G < 1 || n < 1 || S < 1 || seg_shift < 6 ||
      seg_shift > FC_MAX_SEG_SHIFT || tcap < 0 || ocap < 0)
    return 1;
  const long lists = (long)G * S * n;
  unsigned blocks;
  if (!sc_grid(lists, FC_WAVES, blocks)) return 1;
  const size_t lds = (size_t)FC_WAVES * 2 * ((1 << seg_shift) >> 5) * sizeof(uint32_t);
  hipLaunchKernelGGL(fc_order_kernel, dim3(blocks), dim3(64 * FC_WAVES), lds, stream, cnt, base,
                     reinterpret_cast<const u32x2_t*>(tmp), tcap, orow, oval, ocap, lists, n, S, seg_shift);
  return sc_launched();
}

// Per (g, f) list of the feature-major codes (col_ptr int64 [G, n + 1], row int32 / val fp32 [G, cap]): n_frags
// int64 [G, n], top_frag int32 / top_max fp32 [G, n, Kt], rand_frag int32 [G, n, Kr]; fragment = row / L.
int sc_fragment_examples(const long* col_ptr, const int* row, const float* val, long* n_frags, int* top_frag,
                         float* top_max, int* rand_frag, int G, int n, long cap, long L, int Kt, int Kr,
                         unsigned seed, hipStream_t stream) {
  if (!col_ptr || !row || !val || !n_frags || G < 1 || n < 1 || cap < 0 || L < 1 || L > 0x7fffffffL) return 1;
  if (Kt < 0 || Kt > 32 || Kr < 0 || Kr > 32 || (Kt && (!top_frag || !top_max)) || (Kr && !rand_frag)) return 1;
  unsigned blocks;
  if (!sc_grid((long)G * n, FC_WAVES, blocks)) return 1;
  hipLaunchKernelGGL(fragment_examples_kernel, dim3(blocks), dim3(64 * FC_WAVES), 0, stream, col_ptr, row,
                     val, cap, G, n, (uint32_t)L, Kt, Kr, (uint32_t)seed, n_frags, top_frag, top_max, rand_frag);
  return sc_launched();
}

// out fp32 [G, nf, K, L]: the codes of features f0 .. f0 + nf - 1 on the rows of the fragments frags int32 [G, nf, K]
// (n_frag fragments of L rows exist).
int sc_fragment_acts(const long* col_ptr, const int* row, const float* val, const int* frags, float* out, int G, int n,
                     long cap, int f0, int nf, int K, int L, long n_frag, hipStream_t stream) {
  if (!col_ptr || !row || !val || !frags || !out || G < 1 || n < 1 || cap < 0 || L < 1 || K < 1 || nf < 1 || f0 < 0 ||
      (long)f0 + nf > n || n_frag < 0 || n_frag > 0x7fffffffL / L)
    return 1;
  const long slots = (long)G * nf * K;
  unsigned blocks;
  if (!sc_grid(slots, FC_WAVES, blocks)) return 1;
  hipLaunchKernelGGL(fragment_acts_kernel, dim3(blocks), dim3(64 * FC_WAVES), 0, stream, col_ptr, row, val,
                     cap, n, f0, nf, K, L, n_frag, slots, frags, out);
  return sc_launched();
}

}  // extern "C"
