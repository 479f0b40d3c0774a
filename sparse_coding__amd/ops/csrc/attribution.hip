// Per-feature ablation effect and shrinkage from sparse codes (gfx950).
//
// Inputs as sparse_recon.hip: a CSR (row_ptr int64 [G, ldp], col int32 [G, cap], val fp32 [G, cap]: row r of
// model g holds the entries e with columns col_e ascending and codes c_e > 0), the unit-norm bf16 dictionary
// D [G, n, d] (d % 64 == 0, 64 <= d <= 1024, 16-byte aligned) and the bf16 rows x the decoder sees ([n_rows, d]
// shared, stride 0, or [G, n_rows, d]; row r of x belongs to CSR row row0 + r).  With the row's final residual
// r = x - sum_e c_e D[g, col_e], everything a feature does for the reconstruction follows from one number per
// entry, the projection p_e = <r, D[g, col_e]>: removing entry e alone changes the row's squared error by
// 2 c_e p_e + c_e^2 |D[g, col_e]|^2.
//
//   residual_proj_kernel    one wave per (model, row), four waves per block, no LDS; lane / element layout,
//                           loads, axpy and norm are those of sparse_recon.hip (sr_rows.h).
//       pass 1   the full residual exactly as recon_split_kernel forms it: r starts at x, every entry is
//                subtracted in CSR order with one fma per element, 64 entries per load, atoms gathered SR_AHEAD
//                ahead of their subtraction.  sse_row[g, r] = |r|^2 in sr_norm2's order: the bits of column 0
//                of sc_recon_split on the same inputs.
//       pass 2   the same entries again, their atoms gathered again (they were read a moment ago), and per
//                entry p_e: per lane s <- fma(r_i, a_i, s) over the lane's elements i ascending from s = 0,
//                then the xor butterfly 1, 2, 4, 8, 16, 32.  Lane e % 64 keeps p_e, and one coalesced store per
//                64 entries writes proj[g, position of e], aligned with col / val.
//   attr_list_sums_kernel   one wave per (model, feature) list of the feature-major codes of ops/feature_codes
//                           built from the SAME CSR (col_ptr int64 [G, n + 1], row int32 / val fp32 [G, fcap],
//                           rows ascending in a list).  Per pass of 64 entries lane l takes entry l: its
//                           (row, c), the entry's CSR position by a binary search for column f in the row's
//                           columns, proj there, and with q_f = norm2[g, f] and delta = 2 p + c q_f in fp64
//                           (the product is exact, the sum rounded once):
//       cnt int64, A = sum c p, P1 = sum p, C2 = sum c^2 in fp64 (the products are exact), n_harm int64 =
//       entries with delta < 0, min_delta / max_delta fp32 = delta rounded to fp32 (0.0 for an empty list).
//                           The order is list_moments_kernel's: entry i of the list goes to lane i % 64, a
//                           lane adds its entries ascending from 0.0, then the xor butterfly.  Loads of
//                           (row, c) run one pass ahead.
//
// Safety.  residual_proj_kernel applies sparse_recon.hip's skip rule: a row with bad pointers, more than n
// entries or a column outside [0, lim) writes sse_row 0, stores nothing into proj and adds 1 to skipped[g]; all
// columns are checked before the first gather, and every store sits behind the row's id < G n_rows test and
// position < cap.  attr_list_sums_kernel clips its list bounds to [0, fcap]; an entry whose row lies outside
// [0, N), whose row pointers fail 0 <= lo <= hi <= cap, or whose column f is not found by the search (the found
// column must equal f) is left out of every sum and counted in missing[g]; the search only reads col inside
// [lo, hi).  No LDS, no floating-point atomics; the only atomics are 64-bit integer adds on skipped / missing.
// The bits of the list sums do not depend on the waves per block.
#include "sr_rows.h"

namespace scamd {

constexpr int AT_WAVES = 4;  // most waves per block of the list walk

template <int P>
__global__ __launch_bounds__(64 * SR_ROWS) void residual_proj_kernel(
    const long* __restrict__ row_ptr, long ldp, long row0, long n_rows, const int* __restrict__ col,
    const float* __restrict__ val, long cap, const uint16_t* __restrict__ D, const uint16_t* __restrict__ x,
    long x_stride, const int* __restrict__ nactive, int G, int n, float* __restrict__ proj,
    float* __restrict__ sse_row, unsigned long long* __restrict__ skipped) {
  constexpr int d = 64 * P;
  const int lane = threadIdx.x & 63;
  const long id = (long)blockIdx.x * SR_ROWS + (threadIdx.x >> 6);  // (g, row) flattened
  if (id >= (long)G * n_rows) return;                                // (the whole wave)
  const int g = (int)(id / n_rows);
  const long r = id - (long)g * n_rows;
  const long lo = row_ptr[(long)g * ldp + row0 + r], hi = row_ptr[(long)g * ldp + row0 + r + 1];
  const int lim = live_limit(nactive, g, n);
  col += (long)g * cap;
  val += (long)g * cap;
  proj += (long)g * cap;
  if (!csr_row_ok(lo, hi, cap, n, lim, col, lane)) {
    if (lane == 0) {
      sse_row[id] = 0.f;
      atomicAdd(skipped + g, 1ull);
    }
    return;
  }
  const int L = (int)(hi - lo);
  col += lo;
  val += lo;
  D += (long)g * n * d;
  float res[P];
  {
    uint32_t w[SrLay<P>::W];
    sr_load<P>(x + (long)g * x_stride + r * d, lane, w);
#pragma unroll
    for (int i = 0; i < P; ++i) res[i] = sr_elem<P>(w, i);
  }
  // pass 1: the full residual, in recon_split_kernel's order
  for (int base = 0; base < L; base += 64) {
    const int cnt = min(64, L - base);
    int mycol = 0;
    float myval = 0.f;
    if (lane < cnt) {
      mycol = col[base + lane];  // (checked above: 0 <= mycol < lim <= n)
      myval = val[base + lane];
    }
    for (int i0 = 0; i0 < cnt; i0 += SR_AHEAD) {
      uint32_t a[SR_AHEAD][SrLay<P>::W];
#pragma unroll
      for (int u = 0; u < SR_AHEAD; ++u)
        if (i0 + u < cnt) sr_load<P>(D + (long)__shfl(mycol, i0 + u, 64) * d, lane, a[u]);
#pragma unroll
      for (int u = 0; u < SR_AHEAD; ++u)
        if (i0 + u < cnt) sr_axpy<P>(res, __shfl(myval, i0 + u, 64), a[u]);
    }
  }
  const float sse = sr_norm2<P>(res);
  if (lane == 0) sse_row[id] = sse;
  // pass 2: the projection of the residual on every entry's atom
  for (int base = 0; base < L; base += 64) {
    const int cnt = min(64, L - base);
    int mycol = 0;
    if (lane < cnt) mycol = col[base + lane];
    float myp = 0.f;
    for (int i0 = 0; i0 < cnt; i0 += SR_AHEAD) {
      uint32_t a[SR_AHEAD][SrLay<P>::W];
#pragma unroll
      for (int u = 0; u < SR_AHEAD; ++u)
        if (i0 + u < cnt) sr_load<P>(D + (long)__shfl(mycol, i0 + u, 64) * d, lane, a[u]);
#pragma unroll
      for (int u = 0; u < SR_AHEAD; ++u)
        if (i0 + u < cnt) {
          float s = 0.f;
#pragma unroll
          for (int i = 0; i < P; ++i) s = fmaf(res[i], sr_elem<P>(a[u], i), s);
          s = wave_sum_xor<true>(s);
          if (lane == i0 + u) myp = s;
        }
    }
    const long pos = lo + base + lane;
    if (lane < cnt && pos < cap) proj[pos] = myp;
  }
}

__global__ __launch_bounds__(64 * AT_WAVES) void attr_list_sums_kernel(
    const long* __restrict__ col_ptr, const int* __restrict__ frow, const float* __restrict__ fval, long fcap,
    long lists, int n, const long* __restrict__ row_ptr, long ldp, long N, const int* __restrict__ col,
    const float* __restrict__ proj, long cap, const float* __restrict__ norm2, int waves, long* __restrict__ cnt,
    double* __restrict__ A, double* __restrict__ P1, double* __restrict__ C2, long* __restrict__ n_harm,
    float* __restrict__ min_delta, float* __restrict__ max_delta, unsigned long long* __restrict__ missing) {
  ListWalk w;
  if (!list_walk(w, lists, waves)) return;
  w.split(n);
  const int lane = w.lane, g = w.g, f = w.f;
  const long id = w.id;
  long lo, hi;
  list_bounds(col_ptr + (long)g * (n + 1), f, fcap, lo, hi);
  frow += (long)g * fcap;
  fval += (long)g * fcap;
  row_ptr += (long)g * ldp;
  col += (long)g * cap;
  proj += (long)g * cap;
  const double qf = (double)norm2[id];

  double a = 0.0, p1 = 0.0, c2 = 0.0;
  long k = 0, harm = 0, miss = 0;
  float mn = INFINITY, mx = -INFINITY;
  int r0, r1;
  float c0, c1;
  list_load(frow, fval, lo, hi, lane, r0, c0);
  for (long b = lo; b < hi; b += 64) {
    list_load(frow, fval, b + 64, hi, lane, r1, c1);
    if (b + lane < hi) {
      bool found = false;
      float p = 0.f;
      if (r0 >= 0 && (long)r0 < N) {
        const long s = row_ptr[r0], e = row_ptr[r0 + 1];
        if (s >= 0 && e >= s && e <= cap) {
          long lb = s, ub = e;  // the first position in [s, e) whose column is >= f
          while (lb < ub) {
            const long m = (lb + ub) >> 1;
            if (col[m] < f) lb = m + 1;
            else ub = m;
          }
          if (lb < e && col[lb] == f) {
            found = true;
            p = proj[lb];
          }
        }
      }
      if (found) {
        const double c = (double)c0, pd = (double)p;
        a = a + c * pd;    // (c * pd, c * c and c * qf are exact in fp64: fused or not, the same bits)
        p1 = p1 + pd;
        c2 = c2 + c * c;
        const double dl = 2.0 * pd + c * qf;
        harm += dl < 0.0 ? 1 : 0;
        const float df = (float)dl;
        mn = fminf(mn, df);
        mx = fmaxf(mx, df);
        k += 1;
      } else {
        miss += 1;
      }
    }
    r0 = r1;
    c0 = c1;
  }
  a = wave_sum_xor<true>(a);
  p1 = wave_sum_xor<true>(p1);
  c2 = wave_sum_xor<true>(c2);
  k = wave_sum_xor<true>(k);
  harm = wave_sum_xor<true>(harm);
  miss = wave_sum_xor<true>(miss);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) {
    cnt[id] = k;
    A[id] = a;
    P1[id] = p1;
    C2[id] = c2;
    n_harm[id] = harm;
    min_delta[id] = k > 0 ? mn : 0.f;
    max_delta[id] = k > 0 ? mx : 0.f;
    if (miss > 0) atomicAdd(missing + g, (unsigned long long)miss);
  }
}

}  // namespace scamd

using namespace scamd;

extern "C" {

// Rows row0 .. row0 + n_rows - 1 of the CSR against D bf16 [G, n, d] and the rows x bf16, arguments as
// sc_recon_split; proj fp32 [G, cap] receives p_e at the position of every entry of the rows that pass the skip
// rule (other positions are left as they are), sse_row fp32 [G, n_rows] is written, skipped int64 [G] is added to.
int sc_residual_proj(const long* row_ptr, const int* col, const float* val, const void* D, const void* x,
                     const int* nactive, float* proj, float* sse_row, void* skipped, int G, long n_rows, int n, int d,
                     long ldp, long row0, long cap, long x_stride, hipStream_t stream) {
  if (!proj || sr_bad_rows(row_ptr, col, val, D, x, sse_row, skipped, G, n_rows, n, d, ldp, row0, cap, x_stride))
    return 1;
  if (n_rows == 0) return 0;
  const unsigned blocks = (unsigned)(((long)G * n_rows + SR_ROWS - 1) / SR_ROWS);
  SR_DISPATCH(d / 64, hipLaunchKernelGGL(residual_proj_kernel<P>, dim3(blocks), dim3(64 * SR_ROWS), 0, stream,
                                         row_ptr, ldp, row0, n_rows, col, val, cap,
                                         reinterpret_cast<const uint16_t*>(D), reinterpret_cast<const uint16_t*>(x),
                                         x_stride, nactive, G, n, proj, sse_row,
                                         reinterpret_cast<unsigned long long*>(skipped)))
  return sc_launched();
}

// The raw attribution sums of every (g, f) list of the feature-major codes (col_ptr int64 [G, n + 1], frow int32 /
// fval fp32 [G, fcap]) of the CSR row_ptr int64 [G, ldp] (N rows) / col int32 [G, cap] with proj fp32 [G, cap]
// and norm2 fp32 [G, n]: cnt int64, A, P1, C2 fp64, n_harm int64, min_delta, max_delta fp32, [G, n] each, are
// written; missing int64 [G] is added to.  waves: waves per block, 1 .. 4.
int sc_attr_list_sums(const long* col_ptr, const int* frow, const float* fval, const long* row_ptr, const int* col,
                      const float* proj, const float* norm2, long* cnt, double* A, double* P1, double* C2,
                      long* n_harm, float* min_delta, float* max_delta, void* missing, int G, int n, long fcap,
                      long N, long ldp, long cap, int waves, hipStream_t stream) {
  if (!col_ptr || !frow || !fval || !row_ptr || !col || !proj || !norm2 || !cnt || !A || !P1 || !C2 || !n_harm ||
      !min_delta || !max_delta || !missing)
    return 1;
  if (G < 1 || n < 1 || fcap < 0 || fcap > 0x7fffffffL || N < 0 || N > 0x7fffffffL || ldp < N + 1 || cap < 0 ||
      waves < 1 || waves > AT_WAVES)
    return 1;
  const long lists = (long)G * n;
  unsigned blocks;
  if (!sc_grid(lists, waves, blocks)) return 1;
  hipLaunchKernelGGL(attr_list_sums_kernel, dim3(blocks), dim3(64 * waves), 0, stream, col_ptr, frow, fval,
                     fcap, lists, n, row_ptr, ldp, N, col, proj, cap, norm2, waves, cnt, A, P1, C2, n_harm, min_delta,
                     max_delta, reinterpret_cast<unsigned long long*>(missing));
  return sc_launched();
}

}  // extern "C"
