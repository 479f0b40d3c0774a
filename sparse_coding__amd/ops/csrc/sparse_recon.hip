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
#include "common.h"

namespace scamd {

constexpr int SR_ROWS = 4;   // rows (waves) per block
constexpr int SR_AHEAD = 4;  // atoms the split kernel gathers ahead of their subtraction

template <int P>
struct SrLay {
  static constexpr int V = P % 8 == 0 ? 8 : P % 4 == 0 ? 4 : P % 2 == 0 ? 2 : 1;  // elements per piece
  static constexpr int NP = P / V;                                                // pieces per lane
  static constexpr int W = V == 1 ? P : P / 2;                                    // 32-bit words of a packed row
};

// This lane's P elements of the bf16 row at `p`, packed as they lie in memory.
template <int P>
__device__ __forceinline__ void sr_load(const uint16_t* __restrict__ p, int lane, uint32_t (&w)[SrLay<P>::W]) {
  constexpr int V = SrLay<P>::V;
#pragma unroll
  for (int pc = 0; pc < SrLay<P>::NP; ++pc) {
    const uint16_t* q = p + pc * 64 * V + V * lane;
    if constexpr (V == 8) {
      const u32x4_t t = *reinterpret_cast<const u32x4_t*>(q);
      w[4 * pc] = t[0], w[4 * pc + 1] = t[1], w[4 * pc + 2] = t[2], w[4 * pc + 3] = t[3];
    } else if constexpr (V == 4) {
      const u32x2_t t = *reinterpret_cast<const u32x2_t*>(q);
      w[2 * pc] = t[0], w[2 * pc + 1] = t[1];
    } else if constexpr (V == 2) {
      w[pc] = *reinterpret_cast<const uint32_t*>(q);
    } else {
      w[pc] = *q;
    }
  }
}

// Element i (0 .. P-1) of a packed row as fp32.
template <int P>
__device__ __forceinline__ float sr_elem(const uint32_t (&w)[SrLay<P>::W], int i) {
  if constexpr (SrLay<P>::V == 1) return __uint_as_float(w[i] << 16);
  else return __uint_as_float((i & 1) ? (w[i >> 1] & 0xffff0000u) : (w[i >> 1] << 16));
}

// r <- r - c a, one fma per element.
template <int P>
__device__ __forceinline__ void sr_axpy(float (&r)[P], float c, const uint32_t (&a)[SrLay<P>::W]) {
#pragma unroll
  for (int i = 0; i < P; ++i) r[i] = fmaf(-c, sr_elem<P>(a, i), r[i]);
}

// |r|^2 over the wave: per lane ascending, then the xor butterfly 1, 2, 4, 8, 16, 32.
template <int P>
__device__ __forceinline__ float sr_norm2(const float (&r)[P]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < P; ++i) s = fmaf(r[i], r[i], s);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
  return s;
}

__device__ __forceinline__ unsigned long long sr_max64(unsigned long long v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  // every lane holds the maximum: hand it on as a wave-uniform value
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long sr_key(float c, int col) {
  return ((unsigned long long)__float_as_uint(c) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)col);
}

// The skip rule (wave-uniform result).  `col` is the model's column array.
__device__ __forceinline__ bool sr_row_ok(long lo, long hi, long cap, int n, int lim, const int* __restrict__ col,
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
  int lim = n;
  if (nactive) lim = min(n, max(0, nactive[g]));
  col += (long)g * cap;
  val += (long)g * cap;
  float* o = out + id * (long)(J + 1);
  if (!sr_row_ok(lo, hi, cap, n, lim, col, lane)) {
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
  int lim = n;
  if (nactive) lim = min(n, max(0, nactive[g]));
  col += (long)g * cap;
  val += (long)g * cap;
  float* o = out + id * 3;
  if (!sr_row_ok(lo, hi, cap, n, lim, col, lane)) {
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

static int launched() { return hipGetLastError() == hipSuccess ? 0 : 3; }

static bool bad_rows(const void* row_ptr, const void* col, const void* val, const void* D, const void* x,
                     const void* out, const void* skipped, int G, long n_rows, int n, int d, long ldp, long row0,
                     long cap, long x_stride) {
  if (!row_ptr || !col || !val || !D || !x || !out || !skipped) return true;
  if (G < 1 || n < 1 || d < 64 || d > 1024 || d % 64) return true;
  if (n_rows < 0 || row0 < 0 || ldp < row0 + n_rows + 1 || cap < 0) return true;
  if (x_stride != 0 && x_stride < n_rows * (long)d) return true;
  return ((long)G * n_rows + SR_ROWS - 1) / SR_ROWS > 0x7fffffffL;
}

#define SR_DISPATCH(P_, CALL) \
  switch (P_) {               \
    case 1: { constexpr int P = 1; CALL; } break;   \
    case 2: { constexpr int P = 2; CALL; } break;   \
    case 3: { constexpr int P = 3; CALL; } break;   \
    case 4: { constexpr int P = 4; CALL; } break;   \
    case 5: { constexpr int P = 5; CALL; } break;   \
    case 6: { constexpr int P = 6; CALL; } break;   \
    case 7: { constexpr int P = 7; CALL; } break;   \
    case 8: { constexpr int P = 8; CALL; } break;   \
    case 9: { constexpr int P = 9; CALL; } break;   \
    case 10: { constexpr int P = 10; CALL; } break; \
    case 11: { constexpr int P = 11; CALL; } break; \
    case 12: { constexpr int P = 12; CALL; } break; \
    case 13: { constexpr int P = 13; CALL; } break; \
    case 14: { constexpr int P = 14; CALL; } break; \
    case 15: { constexpr int P = 15; CALL; } break; \
    case 16: { constexpr int P = 16; CALL; } break; \
    default: return 1;                              \
  }

extern "C" {

// Rows row0 .. row0 + n_rows - 1 of the CSR (row_ptr int64 [G, ldp], col int32 [G, cap], val fp32 [G, cap])
// against D bf16 [G, n, d] and the rows x bf16 (model g's row r at x + g x_stride + r d; x_stride 0: shared);
// nactive int32 [G] or null; out fp32 [G, n_rows, J + 1] is written, skipped int64 [G] is added to.  cap may be 0
// (col and val are then never read: only rows with row_ptr 0 .. 0 pass the skip rule).
int sc_recon_curve(const long* row_ptr, const int* col, const float* val, const void* D, const void* x,
                   const int* nactive, float* out, void* skipped, int G, long n_rows, int n, int d, int J, long ldp,
                   long row0, long cap, long x_stride, hipStream_t stream) {
  if (bad_rows(row_ptr, col, val, D, x, out, skipped, G, n_rows, n, d, ldp, row0, cap, x_stride)) return 1;
  if (J < 0 || J > 64) return 1;
  if (n_rows == 0) return 0;
  const unsigned blocks = (unsigned)(((long)G * n_rows + SR_ROWS - 1) / SR_ROWS);
  SR_DISPATCH(d / 64, hipLaunchKernelGGL(recon_curve_kernel<P>, dim3(blocks), dim3(64 * SR_ROWS), 0, stream, row_ptr,
                                         ldp, row0, n_rows, col, val, cap, reinterpret_cast<const uint16_t*>(D),
                                         reinterpret_cast<const uint16_t*>(x), x_stride, nactive, G, n, J, out,
                                         reinterpret_cast<unsigned long long*>(skipped)))
  return launched();
}

// As sc_recon_curve; keep uint32 [G, ceil(n / 32)] or null; out fp32 [G, n_rows, 3] is written.
int sc_recon_split(const long* row_ptr, const int* col, const float* val, const void* D, const void* x,
                   const int* nactive, const void* keep, float* out, void* skipped, int G, long n_rows, int n, int d,
                   long ldp, long row0, long cap, long x_stride, hipStream_t stream) {
  if (bad_rows(row_ptr, col, val, D, x, out, skipped, G, n_rows, n, d, ldp, row0, cap, x_stride)) return 1;
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
  return launched();
}

}  // extern "C"
