// Co-activation partners per feature from sparse codes, across models (gfx950).
//
// Source: the feature-major lists of ops/feature_codes (col_ptr int64 [Ga, n_a + 1], row int32 / val fp32
// [Ga, capa], rows ascending in a list).  Target: the per-model CSR of ops/sparse_codes (row_ptr int64
// [Gb, ldp], col int32 / val fp32 [Gb, capb]).  For source model g, feature f, target model h, column j:
//
//   both[j] = rows on which f and j both fire                      (int32)
//   dot[j]  = sum over those rows, ascending, of a_r * b_r         (fp32: acc = fmaf(a_r, b_r, acc) from 0)
//
//   list_moments_kernel   one wave per (model, feature) list: cnt int32, s1 = sum c, s2 = sum c^2 in fp64.  The
//                         order is fixed: per lane the entries lane, lane + 64, ... ascending, then the xor
//                         butterfly 1, 2, 4, 8, 16, 32 (a + b commutes, every lane ends with the same bits).
//   coact_topm_kernel     one wave per (g, f, h) with private LDS accumulators over a window of W target
//                         columns (the host picks W and the waves per block so a block stays within 64 KiB).
//                         The wave walks the source list 64 entries per load (one (row, code) per lane), loads
//                         their 64 target row-pointer pairs, and visits the rows in ascending order with
//                         wave-uniform reads of those registers.  ONE TARGET ROW PER LDS UPDATE INSTRUCTION:
//                         lanes take the row's entries 64 at a time and the columns of a row are distinct, so
//                         an address has at most one contributor per instruction and program order between rows
//                         fixes the fp32 order.  The first 64 columns / codes of the next CO_PREFETCH rows are
//                         loaded before the first of them is added (list entry -> row pointer -> entries is
//                         otherwise three dependent memory latencies per row).
//       DOT = true   (pearson / cosine) two accumulators, dot fp32 and both int32: 8 bytes per column; a model
//                    wider than W is walked once per window of columns, the winners carried across windows.
//       DOT = false  (jaccard) one accumulator, both int32: 4 bytes per column; the dot of the winners comes
//                    from a second walk into the same words once the winners are chosen.
//                         After a walk each lane scores its columns lane, lane + 64, ... in fp32 with unfused
//                         operations; a candidate (both >= min_both, not the excluded own column) that beats
//                         the m-th slot is inserted into the sorted list held one slot per lane, on the key
//                         (order-preserving map of the score's bits) << 32 | (0xFFFFFFFF - column): score
//                         descending, then column ascending.  All four outputs are written for all m slots;
//                         empty slots read (-1, 0.0, 0, 0.0).
//
// Skip rule of the target (that of fc_count_kernel): a row is left out whole unless 0 <= row_ptr[r] <=
// row_ptr[r + 1] <= capb, L <= n_b and every column lies in [0, lim), lim = n_b or min(n_b, nactive[h]).  All
// columns of a row are checked before any is used as an LDS index, and an index is used only inside the window.
// Source lists are guarded too: 0 <= col_ptr[f] <= col_ptr[f + 1] <= capa (clipped), 0 <= row < N per entry.
// Rows with a repeated column are outside the contract (one contributor wins); nothing is written outside.
// No floating-point atomics; every store sits behind its own bound.
//
// Known weak spot: a feature that fires on every row is one wave walking N rows in sequence.
#include "code_lists.h"

namespace scamd {

constexpr int CO_WAVES = 4;            // waves per block where LDS allows
constexpr int CO_MAX_LDS = 65536;      // bytes of accumulators a block may ask for
constexpr int CO_MAX_COLS = 16384;     // widest target model
constexpr int CO_PREFETCH = 8;         // target rows whose first 64 entries are in flight together
constexpr int CO_MAX_M = 32;

__global__ __launch_bounds__(64 * CO_WAVES) void list_moments_kernel(
    const long* __restrict__ col_ptr, const float* __restrict__ val, long cap, long lists, int n,
    int* __restrict__ cnt, double* __restrict__ s1, double* __restrict__ s2) {
  ListWalk w;
  if (!list_walk(w, lists, CO_WAVES)) return;  // (every block has CO_WAVES waves; the wave index stays scalar)
  w.split(n);
  const int lane = w.lane, g = w.g;
  const long id = w.id;
  long lo, hi;
  list_bounds(col_ptr + (long)g * (n + 1), w.f, cap, lo, hi);
  val += (long)g * cap;
  double a = 0.0, b = 0.0;
  for (long e = lo + lane; e < hi; e += 64) {
    const double c = (double)val[e];
    a = a + c;
    b = b + c * c;  // (c * c is exact in fp64: fused or not, the same bits)
  }
  a = wave_sum_xor<true>(a);
  b = wave_sum_xor<true>(b);
  if (lane == 0) {
    cnt[id] = (int)(hi - lo);
    s1[id] = a;
    s2[id] = b;
  }
}

// a - b c with the product rounded on its own.  HIP's __fmul_rn / __fsub_rn lower to plain operators, which the
// compiler contracts into one fma (measured: a contract(off) pragma did not stop it); the empty asm makes the
// rounded product a value of its own.
__device__ __forceinline__ float co_sub_mul(float a, float b, float c) {
  float p = __fmul_rn(b, c);
  asm volatile("" : "+v"(p));
  return __fsub_rn(a, p);
}

struct CoSlot {  // one slot of the sorted winners, one per lane (slots 0 .. m - 1); key 0: empty
  unsigned long long key;
  int both;
  float dot;
};

// Insert the wave-uniform candidate x (keys are distinct); one that does not beat slot K - 1 changes nothing.
__device__ __forceinline__ void insert_slot(CoSlot& cur, const CoSlot& x, int K, int lane) {
  const int pos = insert_pos(cur.key > x.key, K);
  insert_take(cur.key, x.key, pos, K, lane);
  insert_take(cur.both, x.both, pos, K, lane);
  insert_take(cur.dot, x.dot, pos, K, lane);
}

struct CoTarget {  // the CSR of target model h
  const long* __restrict__ row_ptr;
  const int* __restrict__ col;
  const float* __restrict__ val;
  long N, cap;
  int n, lim;
};

// MODE 0: both[o] += 1 (ib).  MODE 1: dot[o] = fmaf(a, v, dot[o]) and both[o] += 1.  MODE 2: dot only (fd).
template <int MODE>
__device__ __forceinline__ void co_update(float* fd, int* ib, int j, float v, float a, int c0, int W) {
  const unsigned o = (unsigned)(j - c0);
  if (o < (unsigned)W) {
    if constexpr (MODE != 0) fd[o] = __fmaf_rn(a, v, fd[o]);
    if constexpr (MODE != 2) ib[o] += 1;
  }
}

// One walk over the source list [lo, hi) (rows `arow`, codes `aval`): every valid target row adds its entries
// with a column in [c0, c0 + W) to the accumulators.
template <int MODE>
__device__ __forceinline__ void co_walk(long lo, long hi, const int* __restrict__ arow,
                                        const float* __restrict__ aval, const CoTarget& t, float* fd, int* ib,
                                        int c0, int W, int lane) {
  for (long b = lo; b < hi; b += 64) {
    const int cnt = (int)min(64l, hi - b);
    int elo = 0, elen = 0;
    float a = 0.f;
    if (lane < cnt) {
      const long r = arow[b + lane];
      a = aval[b + lane];
      if (r >= 0 && r < t.N) {
        const long plo = t.row_ptr[r], phi = t.row_ptr[r + 1];
        if (plo >= 0 && phi >= plo && phi <= t.cap && phi - plo <= (long)t.n) {
          elo = (int)plo;  // (cap < 2^31)
          elen = (int)(phi - plo);
        }
      }
    }
    for (int i0 = 0; i0 < cnt; i0 += CO_PREFETCH) {
      int e0[CO_PREFETCH], len[CO_PREFETCH], cj[CO_PREFETCH];
      float av[CO_PREFETCH], cv[CO_PREFETCH];
#pragma unroll
      for (int k = 0; k < CO_PREFETCH; ++k) {
        const int i = min(i0 + k, 63);
        e0[k] = __builtin_amdgcn_readlane(elo, i);
        len[k] = i0 + k < cnt ? __builtin_amdgcn_readlane(elen, i) : 0;
        av[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), i));
        cj[k] = 0;
        cv[k] = 0.f;
        if (lane < len[k]) {  // (the first 64 entries; e0 + lane < e0 + len <= cap)
          cj[k] = t.col[(long)e0[k] + lane];
          cv[k] = t.val[(long)e0[k] + lane];
        }
      }
#pragma unroll
      for (int k = 0; k < CO_PREFETCH; ++k) {
        const int L = len[k];
        if (L == 0) continue;
        if (L <= 64) {
          const bool bad = lane < L && (unsigned)cj[k] >= (unsigned)t.lim;
          if (__ballot(bad) != 0ull) continue;
          if (lane < L) co_update<MODE>(fd, ib, cj[k], cv[k], av[k], c0, W);
        } else {
          bool bad = false;
          for (int q = lane; q < L; q += 64) bad |= (unsigned)t.col[(long)e0[k] + q] >= (unsigned)t.lim;
          if (__ballot(bad) != 0ull) continue;
          for (int q0 = 0; q0 < L; q0 += 64) {  // 64 distinct columns per update instruction
            const int q = q0 + lane;
            if (q < L) co_update<MODE>(fd, ib, t.col[(long)e0[k] + q], t.val[(long)e0[k] + q], av[k], c0, W);
            __builtin_amdgcn_wave_barrier();
          }
        }
        __builtin_amdgcn_wave_barrier();  // (rows stay in program order)
      }
    }
  }
}

template <bool DOT>
__global__ __launch_bounds__(64 * CO_WAVES) void coact_topm_kernel(
    const long* __restrict__ a_col_ptr, const int* __restrict__ a_row, const float* __restrict__ a_val, long capa,
    int Ga, int n_a, const long* __restrict__ b_row_ptr, long ldp, long N, const int* __restrict__ b_col,
    const float* __restrict__ b_val, long capb, int Gb, int n_b, const int* __restrict__ nactive_b,
    const float* __restrict__ shift_a, const float* __restrict__ scale_a, const int* __restrict__ cnt_a,
    const float* __restrict__ shift_b, const float* __restrict__ scale_b, const int* __restrict__ cnt_b, int m,
    int min_both, int exclude_self, int W, int waves, int* __restrict__ partner, float* __restrict__ score,
    int* __restrict__ both, float* __restrict__ dot) {
  extern __shared__ int co_lds[];
  ListWalk lw;  // id: (g, f, h) flattened
  if (!list_walk(lw, (long)Ga * n_a * Gb, waves)) return;
  const int lane = lw.lane, wave = lw.wave;
  const long id = lw.id;
  const int h = (int)(id % Gb), f = (int)((id / Gb) % n_a), g = (int)(id / ((long)Gb * n_a));
  int* ib = co_lds + (long)wave * (DOT ? 2 : 1) * W;  // both
  float* fd = reinterpret_cast<float*>(DOT ? ib + W : ib);  // dot (DOT: its own words; else the second walk's)

  long lo, hi;
  list_bounds(a_col_ptr + (long)g * (n_a + 1), f, capa, lo, hi);
  const int* arow = a_row + (long)g * capa;
  const float* aval = a_val + (long)g * capa;
  CoTarget t;
  t.row_ptr = b_row_ptr + (long)h * ldp;
  t.col = b_col + (long)h * capb;
  t.val = b_val + (long)h * capb;
  t.N = N;
  t.cap = capb;
  t.n = n_b;
  t.lim = live_limit(nactive_b, h, n_b);

  const long af = (long)g * n_a + f;
  const float sha = shift_a[af], sca = scale_a[af];
  const int cna = cnt_a[af];
  const int own = (exclude_self && g == h) ? f : -1;
  shift_b += (long)h * n_b;
  scale_b += (long)h * n_b;
  cnt_b += (long)h * n_b;

  CoSlot top;
  top.key = 0ull;
  top.both = 0;
  top.dot = 0.f;
  if (hi > lo) {
    for (int c0 = 0; c0 < n_b; c0 += W) {
      const int w = min(W, n_b - c0);
      for (int o = lane; o < w; o += 64) {
        ib[o] = 0;
        if constexpr (DOT) fd[o] = 0.f;
      }
      wave_sync();
      co_walk<DOT ? 1 : 0>(lo, hi, arow, aval, t, fd, ib, c0, w, lane);
      wave_sync();
      for (int o0 = 0; o0 < w; o0 += 64) {
        const int o = o0 + lane, j = c0 + o;
        CoSlot x;
        x.key = 0ull;
        x.both = 0;
        x.dot = 0.f;
        if (o < w) {
          x.both = ib[o];
          if (x.both >= min_both && j != own) {
            float s;
            if constexpr (DOT) {
              x.dot = fd[o];
              s = co_sub_mul(x.dot, sha, shift_b[j]);
              s = __fmul_rn(__fmul_rn(s, sca), scale_b[j]);
            } else {
              s = __fdiv_rn((float)x.both, (float)(cna + cnt_b[j] - x.both));
            }
            s = __fadd_rn(s, 0.f);  // (-0.0 reads +0.0)
            x.key = ((unsigned long long)order_key(s) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)j);
          }
        }
        const unsigned long long kth = __shfl(top.key, m - 1, 64);
        unsigned long long todo = __ballot(x.key > kth);
        while (todo) {
          const int i = __ffsll((long long)todo) - 1;
          todo &= todo - 1ull;
          CoSlot y;
          y.key = __shfl(x.key, i, 64);
          y.both = __shfl(x.both, i, 64);
          y.dot = __shfl(x.dot, i, 64);
          insert_slot(top, y, m, lane);
        }
      }
      wave_sync();  // (the next window clears the words just read)
    }
    if constexpr (!DOT) {  // the dot of the winners: a second walk into the same words, window by window
      if (__ballot(lane < m && top.key != 0ull) != 0ull) {
        const int j = (int)(0xFFFFFFFFu - (uint32_t)top.key);
        for (int c0 = 0; c0 < n_b; c0 += W) {
          const int w = min(W, n_b - c0);
          for (int o = lane; o < w; o += 64) fd[o] = 0.f;
          wave_sync();
          co_walk<2>(lo, hi, arow, aval, t, fd, ib, c0, w, lane);
          wave_sync();
          if (lane < m && top.key != 0ull && j >= c0 && j < c0 + w) top.dot = fd[j - c0];
          wave_sync();
        }
      }
    }
  }
  if (lane < m) {
    const long o = (((long)g * Gb + h) * n_a + f) * m + lane;
    const bool live = top.key != 0ull;
    float s = 0.f;
    if (live) {
      const uint32_t u = (uint32_t)(top.key >> 32);
      s = __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
    }
    partner[o] = live ? (int)(0xFFFFFFFFu - (uint32_t)top.key) : -1;
    score[o] = s;
    both[o] = live ? top.both : 0;
    dot[o] = live ? top.dot : 0.f;
  }
}

}  // namespace scamd

using namespace scamd;

extern "C" {

// Per (g, f) list of the feature-major codes (col_ptr int64 [G, n + 1], val fp32 [G, cap]): cnt int32 [G, n] its
// stored entries, s1 / s2 fp64 [G, n] the sums of its codes and of their squares in the kernel's fixed order.
int sc_list_moments(const long* col_ptr, const float* val, int* cnt, double* s1, double* s2, int G, int n, long cap,
                    hipStream_t stream) {
  if (!col_ptr || !val || !cnt || !s1 || !s2 || G < 1 || n < 1 || cap < 0) return 1;
  const long lists = (long)G * n;
  unsigned blocks;
  if (!sc_grid(lists, CO_WAVES, blocks)) return 1;
  hipLaunchKernelGGL(list_moments_kernel, dim3(blocks), dim3(64 * CO_WAVES), 0, stream, col_ptr, val, cap,
                     lists, n, cnt, s1, s2);
  return sc_launched();
}

// The m best co-activation partners of every source list among the columns of every target model: partner int32,
// score fp32, both int32, dot fp32, [Ga, Gb, n_a, m] each.  use_dot: 1 the dot instantiation (score = ((dot -
// shift_a shift_b) scale_a) scale_b, 8 bytes of LDS per window column), 0 the count instantiation (score = both /
// (cnt_a + cnt_b - both), 4 bytes).  window: target columns per walk; waves: waves per block;
// waves * window * bytes <= 64 KiB.
int sc_coactivation_topm(const long* a_col_ptr, const int* a_row, const float* a_val, const long* b_row_ptr,
                         const int* b_col, const float* b_val, const int* nactive_b, const float* shift_a,
                         const float* scale_a, const int* cnt_a, const float* shift_b, const float* scale_b,
                         const int* cnt_b, int* partner, float* score, int* both, float* dot, int Ga, int n_a,
                         long capa, int Gb, int n_b, long N, long ldp, long capb, int m, int use_dot, int min_both,
                         int exclude_self, int window, int waves, hipStream_t stream) {
  if (!a_col_ptr || !a_row || !a_val || !b_row_ptr || !b_col || !b_val || !shift_a || !scale_a || !cnt_a ||
      !shift_b || !scale_b || !cnt_b)
    return 1;
  if (Ga < 1 || Gb < 1 || n_a < 1 || n_b < 1 || n_b > CO_MAX_COLS || N < 1 || N > 0x7fffffffL || ldp < N + 1 ||
      capa < 0 || capa > 0x7fffffffL || capb < 0 || capb > 0x7fffffffL || m < 0 || m > CO_MAX_M || min_both < 1)
    return 1;
  if (m == 0) return 0;
  if (!partner || !score || !both || !dot) return 1;
  const long bytes = (long)(use_dot ? 8 : 4) * window;
  if (window < 1 || waves < 1 || waves > CO_WAVES || bytes * waves > CO_MAX_LDS) return 1;
  const long work = (long)Ga * n_a * Gb;
  unsigned blocks;
  if (!sc_grid(work, waves, blocks)) return 1;
  const dim3 grid(blocks), block(64 * waves);
  const size_t lds = (size_t)(bytes * waves);
  if (use_dot)
    hipLaunchKernelGGL(coact_topm_kernel<true>, grid, block, lds, stream, a_col_ptr, a_row, a_val, capa, Ga, n_a,
                       b_row_ptr, ldp, N, b_col, b_val, capb, Gb, n_b, nactive_b, shift_a, scale_a, cnt_a, shift_b,
                       scale_b, cnt_b, m, min_both, exclude_self, window, waves, partner, score, both, dot);
  else
    hipLaunchKernelGGL(coact_topm_kernel<false>, grid, block, lds, stream, a_col_ptr, a_row, a_val, capa, Ga, n_a,
                       b_row_ptr, ldp, N, b_col, b_val, capb, Gb, n_b, nactive_b, shift_a, scale_a, cnt_a, shift_b,
                       scale_b, cnt_b, m, min_both, exclude_self, window, waves, partner, score, both, dot);
  return sc_launched();
}

}  // extern "C"
