// Reconstruction error of sparse codes under truncation and under a feature split (gfx950).
//
// Two kernels over a CSR (row_ptr int64 [G, ldp], col int32 [G, cap], val fp32 [G, cap]: row r of model g
// holds the entries e = 0 .. L-1 with columns col_e and codes c_e > 0), a unit-norm bf16 dictionary
// D [G, n, d] (d % 64 == 0, 64 <= d <= 1024, 16-byte aligned) and the bf16 rows x the decoder sees
// ([n_rows, d] shared by the models, stride 0, or [G, n_rows, d]; row r of x belongs to CSR row row0 + r).
// The reconstruction from an entry set S is x^_S = sum_{e in S} c_e D[g, col_e], and its residual is
// accumulated in fp32 as r_k <- fma(-c_e, D[g, col_e, k], r_k) starting from r = x:
//
//   recon_curve_kernel   out[g, r, j] = |x - x^_{prefix_j}|^2 for j = 0 .. J (J <= 64), prefix_j the first
//                        min(j, L) entries in RANK ORDER: code descending, then column ascending.  The atoms
//                        are subtracted in rank order; j = 0 is |x|^2; a row with L <= j repeats its last value.
//   recon_split_kernel   out[g, r, 0..2] = |x - x^_S|^2 for S = all entries, the entries with
//                        keep[g, col_e] (packed words uint32 [G, ceil(n / 32)], bit col & 31 of word
//                        col >> 5) and the others; each residual subtracts its atoms in the order the CSR
//                        stores them (ascending column).  Without a mask columns 1 and 2 are written 0.
//
// One wave per (model, row), four waves per block, no LDS.  Lane l keeps d / 64 = P residual elements in
// registers, cut into pieces of V = 8, 4, 2 or 1 elements (the largest that divides P): element i = p V + j
// of the lane is k = 64 V p + V l + j, so one piece is one 16-, 8-, 4- or 2-byte load per lane and a wave
// reads 64 V contiguous elements (P = 8, 12, 16 at d = 512, 768, 1024: 16, 8 and 16 bytes per lane).
//
// Rank order needs no "taken" set: it is a strict total order on the 64-bit key
// (float bits of c) << 32 | (0xFFFFFFFF - col) -- positive floats order as unsigned integers -- so round t
// takes the wave-wide maximum over the entries whose key is below the key of round t - 1.  Lane l keeps
// the key of entry l in a register; entries from 64 on are re-read each round (they are L2 resident).
// The key of round t + 1 is chosen and its atom's load issued before the atom of round t is subtracted.
// The split kernel loads 64 entries at a time (one per lane, with its keep bit) and gathers four atoms
// ahead of their subtraction.
//
// fp32 order, fixed by the code: an atom is subtracted element by element with one fma each; a squared
// norm is, per lane, s <- fma(r_i, r_i, s) over i ascending from s = 0, then the butterfly
// s += shfl_xor(s, 1), 2, 4, 8, 16, 32 joins the lanes (every lane ends with the same bits).  The same
// inputs give the same bits every run and under any split of the rows.
//
// Safety (the kernels gather by indices they read): a row is skipped -- zeros are written to its outputs
// and 1 is added to skipped[g] -- unless 0 <= row_ptr[g, r] <= row_ptr[g, r + 1] <= cap, L <= n, and every
// column is in [0, lim), lim = n or min(n, nactive[g]).  All columns are checked before the first gather;
// a gathered column is one of the checked ones.  Every store is behind the row's id < G n_rows test and
// its own j <= J / j < 3 bound.  The only atomic is the 64-bit integer add on skipped.
#include "sr_rows.h"  // the layout, load / axpy / norm helpers (shared with attribution.hip); brings code_lists.h

namespace scamd {

__device__ __forceinline__ unsigned long long sr_max64(unsigned long long v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return uniform_u64(v);  // (every lane holds the maximum)
}

__device__ __forceinline__ unsigned long long sr_key(float c, int col) {
  return ((unsigned long long)__float_as_uint(c) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)col);
}

template <int P>
__global__ __launch_bounds__(64 * SR_ROWS) void recon_curve_kernel(
    const long* __restrict__ row_ptr, long ldp, long row0, long n_rows, const int* __restrict__ col,
    const float* __restrict__ val, long cap, const uint16_t* __restrict__ D, const uint16_t* __restrict__ x,
    long x_stride, const int* __restrict__ nactive, int G, int n, int J, float* __restrict__ out,
    unsigned long long* __restrict__ skipped) {
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
  float* o = out + id * (long)(J + 1);
  if (!csr_row_ok(lo, hi, cap, n, lim, col, lane)) {
    for (int j = lane; j <= J; j += 64) o[j] = 0.f;
    if (lane == 0) atomicAdd(skipped + g, 1ull);
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
  const float s0 = sr_norm2<P>(res);
  float mine = s0;  // point lane + 1 of the curve
  const int T = min(J, L);
  const unsigned long long k0 = lane < L ? sr_key(val[lane], col[lane]) : 0ull;
  // the largest key below `prev` (0: there is none)
  auto select = [&](unsigned long long prev) {
    unsigned long long best = k0 < prev ? k0 : 0ull;
    for (int e = 64 + lane; e < L; e += 64) {
      const unsigned long long k = sr_key(val[e], col[e]);
      if (k < prev && k > best) best = k;
    }
    return sr_max64(best);
  };
  // a chosen key's column is one of the row's checked columns
  auto atom = [&](unsigned long long key) { return D + (long)(0xFFFFFFFFu - (uint32_t)key) * d; };
  unsigned long long cur = T > 0 ? select(~0ull) : 0ull;
  uint32_t a[SrLay<P>::W] = {}, b[SrLay<P>::W] = {};
  if (cur) sr_load<P>(atom(cur), lane, a);
  for (int t = 0; t < T && cur; ++t) {
    const unsigned long long nxt = t + 1 < T ? select(cur) : 0ull;
    if (nxt) sr_load<P>(atom(nxt), lane, b);
    sr_axpy<P>(res, __uint_as_float((uint32_t)(cur >> 32)), a);
    const float s = sr_norm2<P>(res);
    if (lane >= t) mine = s;  // (later points repeat it until their own round)
    cur = nxt;
#pragma unroll
    for (int i = 0; i < SrLay<P>::W; ++i) a[i] = b[i];
  }
  if (lane == 0) o[0] = s0;
  if (lane < J) o[1 + lane] = mine;
}

template <int P, bool KEEP>
__global__ __launch_bounds__(64 * SR_ROWS) void recon_split_kernel(
    const long* __restrict__ row_ptr, long ldp, long row0, long n_rows, const int* __restrict__ col,
    const float* __restrict__ val, long cap, const uint16_t* __restrict__ D, const uint16_t* __restrict__ x,
    long x_stride, const int* __restrict__ nactive, const uint32_t* __restrict__ keep, int G, int n,
    float* __restrict__ out, unsigned long long* __restrict__ skipped) {
  constexpr int d = 64 * P;
  constexpr int Q = KEEP ? P : 1;
  const int lane = threadIdx.x & 63;
  const long id = (long)blockIdx.x * SR_ROWS + (threadIdx.x >> 6);
  if (id >= (long)G * n_rows) return;
  const int g = (int)(id / n_rows);
  const long r = id - (long)g * n_rows;
  const long lo = row_ptr[(long)g * ldp + row0 + r], hi = row_ptr[(long)g * ldp + row0 + r + 1];
  const int lim = live_limit(nactive, g, n);
  col += (long)g * cap;
  val += (long)g * cap;
  float* o = out + id * 3;
  if (!csr_row_ok(lo, hi, cap, n, lim, col, lane)) {
    if (lane < 3) o[lane] = 0.f;
    if (lane == 0) atomicAdd(skipped + g, 1ull);
    return;
  }
  const int L = (int)(hi - lo);
  col += lo;
  val += lo;
  D += (long)g * n * d;
  if constexpr (KEEP) keep += (long)g * ((n + 31) >> 5);
  float full[P], kept[Q], rest[Q];
  {
    uint32_t w[SrLay<P>::W];
    sr_load<P>(x + (long)g * x_stride + r * d, lane, w);
#pragma unroll
    for (int i = 0; i < P; ++i) {
      full[i] = sr_elem<P>(w, i);
      if constexpr (KEEP) kept[i] = rest[i] = full[i];
    }
  }
  for (int base = 0; base < L; base += 64) {
    const int cnt = min(64, L - base);
    int mycol = 0;
    float myval = 0.f;
    bool mykeep = false;
    if (lane < cnt) {
      mycol = col[base + lane];  // (checked above: 0 <= mycol < lim <= n)
      myval = val[base + lane];
      if constexpr (KEEP) mykeep = (keep[mycol >> 5] >> (mycol & 31)) & 1u;
    }
    const unsigned long long kbits = __ballot(mykeep);
    for (int i0 = 0; i0 < cnt; i0 += SR_AHEAD) {
      uint32_t a[SR_AHEAD][SrLay<P>::W];
#pragma unroll
      for (int u = 0; u < SR_AHEAD; ++u)
        if (i0 + u < cnt) sr_load<P>(D + (long)__shfl(mycol, i0 + u, 64) * d, lane, a[u]);
#pragma unroll
      for (int u = 0; u < SR_AHEAD; ++u)
        if (i0 + u < cnt) {
          const float c = __shfl(myval, i0 + u, 64);
          sr_axpy<P>(full, c, a[u]);
          if constexpr (KEEP) {
            if ((kbits >> (i0 + u)) & 1ull) sr_axpy<P>(kept, c, a[u]);
            else sr_axpy<P>(rest, c, a[u]);
          }
        }
    }
  }
  const float sf = sr_norm2<P>(full);
  float sk = 0.f, sr = 0.f;
  if constexpr (KEEP) {
    sk = sr_norm2<P>(kept);
    sr = sr_norm2<P>(rest);
  }
  if (lane < 3) o[lane] = lane == 0 ? sf : lane == 1 ? sk : sr;
}

}  // namespace scamd

using namespace scamd;

extern "C" {

// Rows row0 .. row0 + n_rows - 1 of the CSR (row_ptr int64 [G, ldp], col int32 [G, cap], val fp32 [G, cap])
// against D bf16 [G, n, d] and the rows x bf16 (model g's row r at x + g x_stride + r d; x_stride 0: shared);
// nactive int32 [G] or null; out fp32 [G, n_rows, J + 1] is written, skipped int64 [G] is added to.  cap may be 0
// (col and val are then never read: only rows with row_ptr 0 .. 0 pass the skip rule).
int sc_recon_curve(const long* row_ptr, const int* col, const float* val, const void* D, const void* x,
                   const int* nactive, float* out, void* skipped, int G, long n_rows, int n, int d, int J, long ldp,
                   long row0, long cap, long x_stride, hipStream_t stream) {
  if (sr_bad_rows(row_ptr, col, val, D, x, out, skipped, G, n_rows, n, d, ldp, row0, cap, x_stride)) return 1;
  if (J < 0 || J > 64) return 1;
  if (n_rows == 0) return 0;
  const unsigned blocks = (unsigned)(((long)G * n_rows + SR_ROWS - 1) / SR_ROWS);
  SR_DISPATCH(d / 64, hipLaunchKernelGGL(recon_curve_kernel<P>, dim3(blocks), dim3(64 * SR_ROWS), 0, stream, row_ptr,
                                         ldp, row0, n_rows, col, val, cap, reinterpret_cast<const uint16_t*>(D),
                                         reinterpret_cast<const uint16_t*>(x), x_stride, nactive, G, n, J, out,
                                         reinterpret_cast<unsigned long long*>(skipped)))
  return sc_launched();
}

// As sc_recon_curve; keep uint32 [G, ceil(n / 32)] or null; out fp32 [G, n_rows, 3] is written.
int sc_recon_split(const long* row_ptr, const int* col, const float* val, const void* D, const void* x,
                   const int* nactive, const void* keep, float* out, void* skipped, int G, long n_rows, int n, int d,
                   long ldp, long row0, long cap, long x_stride, hipStream_t stream) {
  if (sr_bad_rows(row_ptr, col, val, D, x, out, skipped, G, n_rows, n, d, ldp, row0, cap, x_stride)) return 1;
  if (n_rows == 0) return 0;
  const unsigned blocks = (unsigned)(((long)G * n_rows + SR_ROWS - 1) / SR_ROWS);
#define SR_SPLIT(K)                                                                                              \
  hipLaunchKernelGGL((recon_split_kernel<P, K>), dim3(blocks), dim3(64 * SR_ROWS), 0, stream, row_ptr, ldp, row0, \
                     n_rows, col, val, cap, reinterpret_cast<const uint16_t*>(D),                                \
                     reinterpret_cast<const uint16_t*>(x), x_stride, nactive,                                    \
                     reinterpret_cast<const uint32_t*>(keep), G, n, out,                                         \
                     reinterpret_cast<unsigned long long*>(skipped))
  if (keep) {
    SR_DISPATCH(d / 64, SR_SPLIT(true))
  } else {
    SR_DISPATCH(d / 64, SR_SPLIT(false))
  }
#undef SR_SPLIT
  return sc_launched();
}

}  // extern "C"
