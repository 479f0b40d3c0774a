// Sparse-times-dense products of the sparse codes with 32 right-hand sides, for whole-dictionary linear probes
// (gfx950): the two products of a least-squares iteration on the codes C [N, n] of every model, and the
// reductions and vector updates between them.
//
// Dense operands always have 32 columns, [G, M, 32] fp32 (unused concepts are zero columns): one row of an
// operand is one 128-byte line, and a wave reads two of them per step -- LANE l SERVES CONCEPT l & 31 OF ENTRY
// 2 i + (l >> 5) of the row or list it walks.  Entries are loaded 64 at a time, one per lane, and handed to the
// two halves by a lane shuffle; the gathers of a chunk are independent of each other.
//
//   probe_rows_kernel    Q = C P - 1 (x) c, masked.  One wave per (model, row) of the CSR of ops/sparse_codes
//                        (row_ptr int64 [G, N + 1], col int32 / val fp32 [G, cap]); P [G, n, 32]; c fp64 [G, 32]
//                        or null; w uint8 [N] or null (a row with w[r] == 0 writes zeros); Q [G, N, 32].
//   probe_lists_kernel   S = C^T R over the feature-major lists of ops/feature_codes (col_ptr int64 [G, n + 1],
//                        row int32 / val fp32 [G, cap]); R [G, N, 32]; S [G, n, 32].  A list is cut into segments
//                        of `seg` entries (ops/probe.py: PROBE_SEG) and one wave takes one segment, so the longest
//                        list does not set the time: segment j of list f covers its entries [j seg, (j + 1) seg).
//                        The front-end's segment table (seg_ptr int64 [G, n + 1]: the first segment of every
//                        list, every list has at least one; seg_feat int32 [G, maxseg]: the list of every
//                        segment, -1 past the last) is device arithmetic on col_ptr; the grid is G maxseg waves.
//                        Every wave writes its fp64 partial [G, maxseg, 32]; probe_lists_fold_kernel adds the
//                        partials of a list in segment order and rounds once.
//   probe_dots_kernel    out[g, k] = sum_m A[g, m, k] B[g, m, k] (B null: the column sums of A), fp64 [G, 32].  One
//                        wave per slab of PROBE_SLAB rows; probe_dots_fold_kernel adds the slabs in order.
//   probe_axpby_kernel   y[g, m, k] <- a[g, k] x[g, m, k] + b[g, k] y[g, m, k] with fp64 coefficients [G, 32]: the
//                        vector updates of the iteration, computed in fp64 and rounded once.
//
// For logistic probes (the Newton loop of engine/probe.py), on margins Z [G, N, 32] with the targets t = bit k of
// the flag words int32 [N] and the fit mask w uint8 [N]:
//   probe_rows_scaled_kernel  Q = D o (C P - 1 (x) c), masked: the body of probe_rows_kernel with one more fp64
//                        multiply before the rounding (D fp32 [G, N, 32]), so a Hessian product needs no pass of its
//                        own over [G, N, 32].
//   probe_logit_kernel   R = sigma(Z) - t, D = sigma(Z) (1 - sigma(Z)) (zeros off the fit rows) and the loss sums
//                        sum_fit softplus(z) - t z, fp64 [G, 32]: sigma and the loss in fp64 from the fp32 margin,
//                        rounded once; slabs and fold as probe_dots_kernel.
//   probe_line_kernel    the loss sums at z + 2^-j u, j = 0 .. 7, fp64 [G, 8, 32]: one read of Z and U.
//
// fp64 order, fixed by the code: every lane starts from +0.0 and takes its entries in order with one
// fma((double)code, (double)operand, acc) each -- even entries (of the row, of the segment, of the slab) in half 0,
// odd ones in half 1 -- and the result is half 0 + half 1; a fold adds partials in ascending order starting from
// the first.  The order does not depend on the waves per block or on anything else of the launch: the same inputs
// give the same bits every run.  No floating-point atomics, no LDS, nothing synchronises.
//
// Safety (the kernels gather by indices they read): a CSR row is used only if it passes csr_row_ok (code_lists.h;
// otherwise zeros are written and 1 is added to skipped[g], the contract of sparse_recon.hip); list bounds go
// through list_bounds; a list entry whose row lies outside [0, N) is skipped; a segment whose list or number is
// not one the pointers describe writes a zero partial, and the fold clips its range to the partials that exist.
// Every store is behind its wave's id test.  The only atomic is the 64-bit integer add on skipped.
#include "code_lists.h"

namespace scamd {

constexpr int PROBE_WAVES = 4;     // waves per block, at most
constexpr int PROBE_SLAB = 1024;   // rows per slab of the dot products (a contract: it fixes the fp64 order)
constexpr int PROBE_STEPS = 8;     // line-search candidates 2^-j, j = 0 .. 7

// This lane's half of sum_e val[e] T[idx[e], lane & 31] over the entries [lo, hi) (wave-uniform bounds), T [M, 32]
// with M >= 1: entry lo + 2 i + (lane >> 5) at step i, in order; an entry whose index lies outside [0, M) is left
// out.
__device__ __forceinline__ double probe_walk(const int* __restrict__ idx, const float* __restrict__ val, long lo,
                                             long hi, const float* __restrict__ T, int M, int lane) {
  const int k = lane & 31, half = lane >> 5;
  double acc = 0.0;
  for (long b = lo; b < hi; b += 64) {
    int j;
    float v;
    list_load(idx, val, b, hi, lane, j, v);  // (-1, 0) past the end: in no sum
    const int steps = ((int)min(64l, hi - b) + 1) >> 1;
#pragma unroll 4
    for (int i = 0; i < steps; ++i) {
      const int src = 2 * i + half;
      const int je = __shfl(j, src, 64);
      const float ve = __shfl(v, src, 64);
      const bool ok = (unsigned)je < (unsigned)M;
      const float t = T[(long)(ok ? je : 0) * 32 + k];  // (an unconditional load of a valid line)
      acc = ok ? fma((double)ve, (double)t, acc) : acc;
    }
  }
  return acc;
}

// half 0 + half 1 in every lane (the addition commutes: both halves hold the same bits).
__device__ __forceinline__ double probe_join(double acc) { return acc + __shfl_xor(acc, 32, 64); }

__device__ __forceinline__ long probe_uniform(long v) { return (long)__builtin_amdgcn_readfirstlane((int)v); }

// The body of the two row kernels.  SCALED: the row of Q is multiplied by the row of D [G, N, 32] in fp64 before
// the one rounding; otherwise D is not read.
template <bool SCALED>
__device__ __forceinline__ void probe_rows_body(
    const long* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ val, long cap,
    const int* __restrict__ nactive, const float* __restrict__ P, const double* __restrict__ c,
    const uint8_t* __restrict__ w, const float* __restrict__ D, int G, int N, int n, int waves,
    float* __restrict__ Q, unsigned long long* __restrict__ skipped) {
  ListWalk lw;
  if (!list_walk(lw, (long)G * N, waves)) return;
  lw.split(N);
  const int lane = lw.lane, g = lw.g, r = lw.f;
  long lo = row_ptr[(long)g * (N + 1) + r], hi = row_ptr[(long)g * (N + 1) + r + 1];
  col += (long)g * cap;
  val += (long)g * cap;
  float* q = Q + lw.id * 32;
  float scale = 1.f;  // (SCALED: loaded before the walk, whose gathers hide its latency; every (g, r) has a row of D)
  if constexpr (SCALED) scale = D[lw.id * 32 + (lane & 31)];
  if (!csr_row_ok(lo, hi, cap, n, live_limit(nactive, g, n), col, lane)) {
    if (lane < 32) q[lane] = 0.f;
    if (lane == 0) atomicAdd(skipped + g, 1ull);
    return;
  }
  if (w && !w[r]) {
    if (lane < 32) q[lane] = 0.f;
    return;
  }
  lo = probe_uniform(lo);  // (0 <= lo <= hi <= cap < 2^31)
  hi = probe_uniform(hi);
  double acc = probe_join(probe_walk(col, val, lo, hi, P + (long)g * n * 32, n, lane));
  if (c) acc -= c[g * 32 + (lane & 31)];
  if constexpr (SCALED) acc *= (double)scale;
  if (lane < 32) q[lane] = (float)acc;
}

__global__ __launch_bounds__(64 * PROBE_WAVES) void probe_rows_kernel(
    const long* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ val, long cap,
    const int* __restrict__ nactive, const float* __restrict__ P, const double* __restrict__ c,
    const uint8_t* __restrict__ w, int G, int N, int n, int waves, float* __restrict__ Q,
    unsigned long long* __restrict__ skipped) {
  probe_rows_body<false>(row_ptr, col, val, cap, nactive, P, c, w, nullptr, G, N, n, waves, Q, skipped);
}

__global__ __launch_bounds__(64 * PROBE_WAVES) void probe_rows_scaled_kernel(
    const long* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ val, long cap,
    const int* __restrict__ nactive, const float* __restrict__ P, const double* __restrict__ c,
    const uint8_t* __restrict__ w, const float* __restrict__ D, int G, int N, int n, int waves,
    float* __restrict__ Q, unsigned long long* __restrict__ skipped) {
  probe_rows_body<true>(row_ptr, col, val, cap, nactive, P, c, w, D, G, N, n, waves, Q, skipped);
}

__global__ __launch_bounds__(64 * PROBE_WAVES) void probe_lists_kernel(
    const long* __restrict__ col_ptr, const int* __restrict__ row, const float* __restrict__ val, long cap,
    const long* __restrict__ seg_ptr, const int* __restrict__ seg_feat, long maxseg, long seg,
    const float* __restrict__ R, int G, int N, int n, int waves, double* __restrict__ part) {
  ListWalk lw;
  if (!list_walk(lw, (long)G * maxseg, waves)) return;
  const int lane = lw.lane;
  const int g = (int)(lw.id / maxseg);
  const long s = lw.id - (long)g * maxseg;
  const int f = __builtin_amdgcn_readfirstlane(seg_feat[lw.id]);
  double acc = 0.0;
  if ((unsigned)f < (unsigned)n) {
    const long j = s - seg_ptr[(long)g * (n + 1) + f];
    long lo, hi;
    list_bounds(col_ptr + (long)g * (n + 1), f, cap, lo, hi);
    if (j >= 0 && j <= (hi - lo) / seg) {
      const long a = probe_uniform(lo + j * seg);  // (<= hi <= cap < 2^31)
      const long e = probe_uniform(min(hi, a + seg));
      acc = probe_walk(row + (long)g * cap, val + (long)g * cap, a, e, R + (long)g * N * 32, N, lane);
    }
  }
  acc = probe_join(acc);
  if (lane < 32) part[lw.id * 32 + lane] = acc;
}

// One thread per (model, list, concept): the list's partials in segment order.
__global__ __launch_bounds__(256) void probe_lists_fold_kernel(const long* __restrict__ seg_ptr,
                                                               const double* __restrict__ part, long maxseg, int G,
                                                               int n, float* __restrict__ S) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)G * n * 32) return;
  const int k = (int)(t & 31);
  const long gf = t >> 5;
  const int g = (int)(gf / n), f = (int)(gf - (long)g * n);
  const long s0 = min(max(seg_ptr[(long)g * (n + 1) + f], 0l), maxseg);
  const long s1 = min(max(seg_ptr[(long)g * (n + 1) + f + 1], s0), maxseg);
  const double* p = part + ((long)g * maxseg) * 32 + k;
  double acc = 0.0;
  if (s0 < s1) {
    acc = p[s0 * 32];
    for (long s = s0 + 1; s < s1; ++s) acc += p[s * 32];
  }
  S[t] = (float)acc;
}

__global__ __launch_bounds__(64 * PROBE_WAVES) void probe_dots_kernel(const float* __restrict__ A,
                                                                      const float* __restrict__ B, int G, long M,
                                                                      long slabs, int waves,
                                                                      double* __restrict__ part) {
  ListWalk lw;
  if (!list_walk(lw, (long)G * slabs, waves)) return;
  const int lane = lw.lane, k = lane & 31, half = lane >> 5;
  const int g = (int)(lw.id / slabs);
  const long sl = lw.id - (long)g * slabs;
  const long r0 = sl * PROBE_SLAB, r1 = min(M, r0 + PROBE_SLAB);
  const long base = (long)g * M * 32 + k;
  double acc = 0.0;
  if (B) {
#pragma unroll 8
    for (long r = r0 + half; r < r1; r += 2) acc = fma((double)A[base + r * 32], (double)B[base + r * 32], acc);
  } else {
#pragma unroll 8
    for (long r = r0 + half; r < r1; r += 2) acc += (double)A[base + r * 32];
  }
  acc = probe_join(acc);
  if (lane < 32) part[lw.id * 32 + lane] = acc;
}

// One thread per (model, concept): the slabs in order.
__global__ __launch_bounds__(64) void probe_dots_fold_kernel(const double* __restrict__ part, long slabs, int G,
                                                             double* __restrict__ out) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= G * 32) return;
  const double* p = part + (long)(t >> 5) * slabs * 32 + (t & 31);
  double acc = p[0];
#pragma unroll 8
  for (long s = 1; s < slabs; ++s) acc += p[s * 32];
  out[t] = acc;
}

// The logistic terms of one margin in fp64, from e = exp(-|z|) alone: sigma(|z|) = 1 / (1 + e) and sigma(-|z|) =
// e / (1 + e), so neither sigma nor 1 - sigma is a difference of nearly equal numbers, and the loss is the stable
// softplus max(z, 0) + log1p(e) minus t z.  r = sigma(z) - t, D = sigma(z) (1 - sigma(z)).
__device__ __forceinline__ double probe_softplus_loss(double z, bool t) {
  return fmax(z, 0.0) + log1p(exp(-fabs(z))) - (t ? z : 0.0);
}

__device__ __forceinline__ void probe_logit_terms(double z, bool t, double& r, double& D, double& loss) {
  const double e = exp(-fabs(z));
  const double big = 1.0 / (1.0 + e), small = e * big;
  const bool up = z >= 0.0;
  r = t ? -(up ? small : big) : (up ? big : small);
  D = big * small;
  loss = fmax(z, 0.0) + log1p(e) - (t ? z : 0.0);
}

// One wave per slab of PROBE_SLAB rows, as probe_dots_kernel: R = sigma(Z) - t and D = sigma (1 - sigma) on the
// rows with w != 0 (t: bit k of flags[r]), zeros on the others, and the slab's fp64 loss partial.
__global__ __launch_bounds__(64 * PROBE_WAVES) void probe_logit_kernel(
    const float* __restrict__ Z, const int* __restrict__ flags, const uint8_t* __restrict__ w, int G, long N,
    long slabs, int waves, float* __restrict__ R, float* __restrict__ D, double* __restrict__ part) {
  ListWalk lw;
  if (!list_walk(lw, (long)G * slabs, waves)) return;
  const int lane = lw.lane, k = lane & 31, half = lane >> 5;
  const int g = (int)(lw.id / slabs);
  const long sl = lw.id - (long)g * slabs;
  const long r0 = sl * PROBE_SLAB, r1 = min(N, r0 + PROBE_SLAB);
  const long base = (long)g * N * 32 + k;
  double acc = 0.0;
  for (long r = r0 + half; r < r1; r += 2) {
    float ro = 0.f, dv = 0.f;
    if (w[r]) {
      double rr, dd, ll;
      probe_logit_terms((double)Z[base + r * 32], (flags[r] >> k) & 1, rr, dd, ll);
      ro = (float)rr;
      dv = (float)dd;
      acc += ll;
    }
    R[base + r * 32] = ro;
    D[base + r * 32] = dv;
  }
  acc = probe_join(acc);
  if (lane < 32) part[lw.id * 32 + lane] = acc;
}

// The same walk for the eight line-search candidates: part [G, 8, slabs, 32] holds the slab's partial of
// sum loss(z + 2^-j u, t) (the product 2^-j u is exact in fp64, the sum is rounded once).
__global__ __launch_bounds__(64 * PROBE_WAVES) void probe_line_kernel(
    const float* __restrict__ Z, const float* __restrict__ U, const int* __restrict__ flags,
    const uint8_t* __restrict__ w, int G, long N, long slabs, int waves, double* __restrict__ part) {
  ListWalk lw;
  if (!list_walk(lw, (long)G * slabs, waves)) return;
  const int lane = lw.lane, k = lane & 31, half = lane >> 5;
  const int g = (int)(lw.id / slabs);
  const long sl = lw.id - (long)g * slabs;
  const long r0 = sl * PROBE_SLAB, r1 = min(N, r0 + PROBE_SLAB);
  const long base = (long)g * N * 32 + k;
  double acc[PROBE_STEPS];
#pragma unroll
  for (int j = 0; j < PROBE_STEPS; ++j) acc[j] = 0.0;
  for (long r = r0 + half; r < r1; r += 2) {
    if (!w[r]) continue;
    const double z = (double)Z[base + r * 32], u = (double)U[base + r * 32];
    const bool t = (flags[r] >> k) & 1;
    double s = 1.0;
#pragma unroll
    for (int j = 0; j < PROBE_STEPS; ++j) {
      acc[j] += probe_softplus_loss(z + s * u, t);
      s *= 0.5;
    }
  }
#pragma unroll
  for (int j = 0; j < PROBE_STEPS; ++j) {
    const double a = probe_join(acc[j]);
    if (lane < 32) part[(((long)g * PROBE_STEPS + j) * slabs + sl) * 32 + lane] = a;
  }
}

// Four concepts per thread: y <- a x + b y in fp64, one rounding.
__global__ __launch_bounds__(256) void probe_axpby_kernel(const float* __restrict__ x, const double* __restrict__ a,
                                                          const double* __restrict__ b, int G, long M,
                                                          float* __restrict__ y) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)G * M * 8) return;
  const int g = (int)(t / (M * 8)), k = (int)(t & 7) * 4;
  const f32x4_t xv = reinterpret_cast<const f32x4_t*>(x)[t];
  f32x4_t yv = reinterpret_cast<const f32x4_t*>(y)[t];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    yv[i] = (float)fma(a[g * 32 + k + i], (double)xv[i], b[g * 32 + k + i] * (double)yv[i]);
  reinterpret_cast<f32x4_t*>(y)[t] = yv;
}

}  // namespace scamd

using namespace scamd;

static inline bool probe_waves_ok(int waves) { return waves == 1 || waves == 2 || waves == 4; }

extern "C" {

// Q [G, N, 32] = C P - 1 (x) c on the rows with w != 0, zeros elsewhere: the CSR (row_ptr int64 [G, N + 1], col
// int32 / val fp32 [G, cap]) of G models with n features, P fp32 [G, n, 32], c fp64 [G, 32] or null, w uint8 [N] or
// null, nactive int32 [G] or null.  skipped int64 [G]: += the rows of each model that fail the skip rule.
int sc_probe_rows(const long* row_ptr, const int* col, const float* val, const int* nactive, const float* P,
                  const double* c, const unsigned char* w, float* Q, long* skipped, int G, long N, int n, long cap,
                  int waves, hipStream_t stream) {
  if (!row_ptr || !col || !val || !P || !Q || !skipped) return 1;
  if (G < 1 || N < 1 || N >= 0x7fffffffL || n < 1 || cap < 0 || cap > 0x7fffffffL || !probe_waves_ok(waves)) return 1;
  unsigned blocks;
  if (!sc_grid((long)G * N, waves, blocks)) return 1;
  hipLaunchKernelGGL(probe_rows_kernel, dim3(blocks), dim3(64 * waves), 0, stream, row_ptr, col, val, cap, nactive,
                     P, c, w, G, (int)N, n, waves, Q, (unsigned long long*)skipped);
  return sc_launched();
}

// sc_probe_rows with every row of Q multiplied by the row of D fp32 [G, N, 32] before the rounding.
int sc_probe_rows_scaled(const long* row_ptr, const int* col, const float* val, const int* nactive, const float* P,
                         const double* c, const unsigned char* w, const float* D, float* Q, long* skipped, int G,
                         long N, int n, long cap, int waves, hipStream_t stream) {
  if (!row_ptr || !col || !val || !P || !D || !Q || !skipped) return 1;
  if (G < 1 || N < 1 || N >= 0x7fffffffL || n < 1 || cap < 0 || cap > 0x7fffffffL || !probe_waves_ok(waves)) return 1;
  unsigned blocks;
  if (!sc_grid((long)G * N, waves, blocks)) return 1;
  hipLaunchKernelGGL(probe_rows_scaled_kernel, dim3(blocks), dim3(64 * waves), 0, stream, row_ptr, col, val, cap,
                     nactive, P, c, w, D, G, (int)N, n, waves, Q, (unsigned long long*)skipped);
  return sc_launched();
}

// R, D fp32 [G, N, 32] and loss fp64 [G, 32] from the margins Z fp32 [G, N, 32], the flag words int32 [N] and the
// fit mask w uint8 [N] (R, D: not Z).  part: fp64 [G, ceil(N / 1024), 32] scratch.
int sc_probe_logit(const float* Z, const int* flags, const unsigned char* w, float* R, float* D, double* part,
                   double* loss, int G, long N, int waves, hipStream_t stream) {
  if (!Z || !flags || !w || !R || !D || !part || !loss) return 1;
  if (G < 1 || G > 0x3ffffff || N < 1 || N > 0x7fffffffL || !probe_waves_ok(waves)) return 1;
  const long slabs = (N + PROBE_SLAB - 1) / PROBE_SLAB;
  unsigned blocks, fold;
  if (!sc_grid((long)G * slabs, waves, blocks) || !sc_grid((long)G * 32, 64, fold)) return 1;
  hipLaunchKernelGGL(probe_logit_kernel, dim3(blocks), dim3(64 * waves), 0, stream, Z, flags, w, G, N, slabs, waves,
                     R, D, part);
  hipLaunchKernelGGL(probe_dots_fold_kernel, dim3(fold), dim3(64), 0, stream, part, slabs, G, loss);
  return sc_launched();
}

// out fp64 [G, 8, 32]: sum over the rows with w != 0 of the loss at Z + 2^-j U, j = 0 .. 7.  part: fp64
// [G, 8, ceil(N / 1024), 32] scratch.
int sc_probe_line(const float* Z, const float* U, const int* flags, const unsigned char* w, double* part,
                  double* out, int G, long N, int waves, hipStream_t stream) {
  if (!Z || !U || !flags || !w || !part || !out) return 1;
  if (G < 1 || G > 0x3fffff || N < 1 || N > 0x7fffffffL || !probe_waves_ok(waves)) return 1;
  const long slabs = (N + PROBE_SLAB - 1) / PROBE_SLAB;
  unsigned blocks, fold;
  if (!sc_grid((long)G * slabs, waves, blocks) || !sc_grid((long)G * PROBE_STEPS * 32, 64, fold)) return 1;
  hipLaunchKernelGGL(probe_line_kernel, dim3(blocks), dim3(64 * waves), 0, stream, Z, U, flags, w, G, N, slabs, waves,
                     part);
  hipLaunchKernelGGL(probe_dots_fold_kernel, dim3(fold), dim3(64), 0, stream, part, slabs, G * PROBE_STEPS, out);
  return sc_launched();
}

// S [G, n, 32] = C^T R: the lists (col_ptr int64 [G, n + 1] with 0 <= col_ptr <= cap, row int32 / val fp32
// [G, cap]), R fp32 [G, N, 32], the segment table (seg_ptr int64 [G, n + 1], seg_feat int32 [G, maxseg]) for
// segments of `seg` entries (even, >= 64) and the partials' scratch part fp64 [G, maxseg, 32].
int sc_probe_lists(const long* col_ptr, const int* row, const float* val, const long* seg_ptr, const int* seg_feat,
                   const float* R, double* part, float* S, int G, int n, long cap, long N, long maxseg, long seg,
                   int waves, hipStream_t stream) {
  if (!col_ptr || !row || !val || !seg_ptr || !seg_feat || !R || !part || !S) return 1;
  if (G < 1 || n < 1 || cap < 0 || cap > 0x7fffffffL || N < 1 || N > 0x7fffffffL || maxseg < 1 ||
      maxseg > 0x7fffffffL || seg < 64 || (seg & 1) || seg > 0x40000000L || !probe_waves_ok(waves))
    return 1;
  unsigned blocks, fold;
  if (!sc_grid((long)G * maxseg, waves, blocks) || !sc_grid((long)G * n * 32, 256, fold)) return 1;
  hipLaunchKernelGGL(probe_lists_kernel, dim3(blocks), dim3(64 * waves), 0, stream, col_ptr, row, val, cap, seg_ptr,
                     seg_feat, maxseg, seg, R, G, (int)N, n, waves, part);
  hipLaunchKernelGGL(probe_lists_fold_kernel, dim3(fold), dim3(256), 0, stream, seg_ptr, part, maxseg, G, n, S);
  return sc_launched();
}

// out fp64 [G, 32]: sum_m A[g, m, k] B[g, m, k] over A, B fp32 [G, M, 32]; B null: the column sums of A.  part: fp64
// [G, ceil(M / 1024), 32] scratch.
int sc_probe_dots(const float* A, const float* B, double* part, double* out, int G, long M, int waves,
                  hipStream_t stream) {
  if (!A || !part || !out) return 1;
  if (G < 1 || G > 0x3ffffff || M < 1 || M > 0x7fffffffL || !probe_waves_ok(waves)) return 1;
  const long slabs = (M + PROBE_SLAB - 1) / PROBE_SLAB;
  unsigned blocks, fold;
  if (!sc_grid((long)G * slabs, waves, blocks) || !sc_grid((long)G * 32, 64, fold)) return 1;
  hipLaunchKernelGGL(probe_dots_kernel, dim3(blocks), dim3(64 * waves), 0, stream, A, B, G, M, slabs, waves, part);
  hipLaunchKernelGGL(probe_dots_fold_kernel, dim3(fold), dim3(64), 0, stream, part, slabs, G, out);
  return sc_launched();
}

// y <- a x + b y in place over x, y fp32 [G, M, 32] (16-byte aligned, y not x) with a, b fp64 [G, 32].
int sc_probe_axpby(const float* x, const double* a, const double* b, float* y, int G, long M, hipStream_t stream) {
  if (!x || !a || !b || !y || (const void*)x == (const void*)y) return 1;
  if (G < 1 || G > 0x3ffffff || M < 1 || M > 0x7fffffffL || ((uintptr_t)x | (uintptr_t)y) % 16) return 1;
  unsigned blocks;
  if (!sc_grid((long)G * M * 8, 256, blocks)) return 1;
  hipLaunchKernelGGL(probe_axpby_kernel, dim3(blocks), dim3(256), 0, stream, x, a, b, G, M, y);
  return sc_launched();
}

}  // extern "C"
