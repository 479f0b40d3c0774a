// Sparse export of stacked SAE codes (gfx950): the strictly positive entries of the bf16 code matrix
// c [G, B, n] the grouped encoder launch writes (B % 128 == 0, n % 128 == 0), per model in CSR order.
//
// Two launches of one streaming body (code_rows_kernel<FILL>), one wave per (model, row), four rows per
// 256-thread block:
//   count: nnz[g, r] = #(c[g, r, :] > 0)  (-0.0, +0.0, negatives and NaN do not count).
//   fill:  the row's positives go to col[g, p ..] / val[g, p ..], p = row_ptr[g, row0 + r], in ascending
//          column order; val is the bf16 code widened to fp32 (exact).
// The host turns the counts into row pointers between the two (a cumsum, ops/sparse_codes.py).
//
// A wave pass covers 512 columns: lane l loads the 16 bytes of columns 512 pass + 8 l .. + 7 (a lane past n
// loads nothing and holds zeros, so n = 128 leaves 48 lanes idle and n = 640 ends in a 16-lane pass); four
// passes are in flight.  Sub-position k of every lane gives one 64-bit ballot of (code > 0).  The row count
// is the sum of the ballots' popcounts on the scalar unit.  A lane's write offset is the number of positives
// in lower lanes -- the eight ballots masked to the lanes below, chained through v_mbcnt -- plus its own
// lower sub-positions: order (pass, lane, sub-position) is ascending column order.  No atomics, no
// data-dependent write order: the same bits every run.
//
// Overflow: an entry whose position is not in [0, cap) is dropped -- every store is behind that test, so
// nothing is written outside col[g, 0 .. cap) / val[g, 0 .. cap) whatever row_ptr holds -- and a row that
// starts at or past cap is not read at all.
#include "common.h"

namespace scamd {

constexpr int SC_ROWS = 4;      // rows (waves) per block
constexpr int SC_PASS = 512;    // columns per wave pass
constexpr int SC_AHEAD = 4;     // passes in flight

template <bool FILL>
__global__ __launch_bounds__(64 * SC_ROWS) void code_rows_kernel(const uint16_t* __restrict__ c, int B, int n,
                                                                 int* __restrict__ nnz,
                                                                 const long* __restrict__ row_ptr, long ldp,
                                                                 long row0, int* __restrict__ col,
                                                                 float* __restrict__ val, long cap) {
  const int lane = threadIdx.x & 63;
  const long id = (long)blockIdx.x * SC_ROWS + (threadIdx.x >> 6);  // (g, row) flattened; B % SC_ROWS == 0
  const int g = (int)(id / B), r = (int)(id - (long)g * B);
  const uint16_t* p = c + id * n + lane * 8;
  long pos = 0;   // wave-uniform: where the next positive of this row goes
  if constexpr (FILL) {
    pos = row_ptr[(long)g * ldp + row0 + r];
    if (pos < 0 || pos >= cap) return;  // (the whole wave: nothing of this row fits)
    col += (long)g * cap;
    val += (long)g * cap;
  }
  int total = 0;
  for (int c0 = 0; c0 < n; c0 += SC_PASS * SC_AHEAD) {
    u32x4_t q[SC_AHEAD];
#pragma unroll
    for (int u = 0; u < SC_AHEAD; ++u) {
      const int cc = c0 + u * SC_PASS + lane * 8;
      q[u] = u32x4_t{0u, 0u, 0u, 0u};
      if (cc < n) q[u] = *reinterpret_cast<const u32x4_t*>(p + c0 + u * SC_PASS);
    }
#pragma unroll
    for (int u = 0; u < SC_AHEAD; ++u) {
      float v[8];
      unsigned below = 0;  // positives of this pass in lower lanes
      int pass_total = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t w = q[u][k >> 1];
        v[k] = __uint_as_float((k & 1) ? (w & 0xffff0000u) : (w << 16));
        const unsigned long long m = __ballot(v[k] > 0.f);
        pass_total += __popcll(m);
        if constexpr (FILL)
          below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, below));
      }
      if constexpr (FILL) {
        if (pass_total) {  // (wave-uniform)
          long at = pos + below;
          const int cc = c0 + u * SC_PASS + lane * 8;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            if (v[k] > 0.f) {
              if (at < cap) {
                col[at] = cc + k;
                val[at] = v[k];
              }
              ++at;
            }
          }
          pos += pass_total;
        }
      } else {
        total += pass_total;
      }
    }
    if constexpr (FILL) {
      if (pos >= cap) return;  // (wave-uniform: the rest of the row is dropped)
    }
  }
  if constexpr (!FILL) {
    if (lane == 0) nnz[id] = total;
  }
}

}  // namespace scamd

using namespace scamd;

static bool codes_ok(const void* c, int G, int B, int n) {
  return c && G >= 1 && B >= 128 && B % 128 == 0 && n >= 128 && n % 128 == 0 &&
         (long)G * B / SC_ROWS <= 0x7fffffffL;
}

extern "C" {

// c bf16 [G, B, n]; nnz int32 [G, B].
int sc_code_row_counts(const void* c, int* nnz, int G, int B, int n, hipStream_t stream) {
  if (!codes_ok(c, G, B, n) || !nnz) return 1;
  hipLaunchKernelGGL(code_rows_kernel<false>, dim3((unsigned)((long)G * B / SC_ROWS)), dim3(64 * SC_ROWS), 0,
                     stream, reinterpret_cast<const uint16_t*>(c), B, n, nnz, nullptr, 0L, 0L, nullptr, nullptr,
                     0L);
  return sc_launched();
}

// row_ptr int64 [G, ldp]: row r of model g starts at row_ptr[g, row0 + r]; col int32 [G, cap], val fp32 [G, cap].
int sc_code_compact(const void* c, const long* row_ptr, int* col, float* val, int G, int B, int n, long ldp,
                    long row0, long cap, hipStream_t stream) {
  if (!codes_ok(c, G, B, n) || !row_ptr || !col || !val || cap < 1 || row0 < 0 || ldp < row0 + B + 1) return 1;
  hipLaunchKernelGGL(code_rows_kernel<true>, dim3((unsigned)((long)G * B / SC_ROWS)), dim3(64 * SC_ROWS), 0,
                     stream, reinterpret_cast<const uint16_t*>(c), B, n, nullptr, row_ptr, ldp, row0, col, val,
                     cap);
  return sc_launched();
}

}  // extern "C"
