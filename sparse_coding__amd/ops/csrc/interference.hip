// Activity-weighted capacity ("expected interference", Scherlis et al. 2022) of sparse codes (gfx950).
//
// Two kernels over a bf16 dictionary D [G, n, d] (d % 32 == 0, 16-byte aligned):
//
//   row_norm2_kernel      norm2[g, f] = sum_k D[g, f, k]^2 in fp32.
//   active_capacity_kernel  for row r of model g of a CSR (row_ptr int64 [G, ldp], col int32 [G, cap],
//                         val fp32 [G, cap]) with entries e = 0 .. L-1, columns j_e and codes c_e:
//       G_ab    = <D[j_a], D[j_b]>                               (v_mfma_f32_16x16x32_bf16, fp32)
//       cos2_ab = (G_ab * G_ab) / (max(norm2[j_a], 1e-16) * max(norm2[j_b], 1e-16))   for a != b
//       total_a = c_a + sum_{b != a} cos2_ab * c_b               (the diagonal is exactly c_a)
//       cap_a   = c_a / max(total_a, 1e-8)
//     and per entry: qsum[g, j_a] += llrint(cap_a * 2^32), count[g, j_a] += 1 (64-bit integer atomics:
//     integer adds commute, so the sums are the same bits every run and under any split of the rows),
//     entry_cap[g, pos_a] = cap_a when that buffer is given.  No floating-point atomic anywhere.
//
// One wave per (model, row), four waves per block, no LDS.  The row's entries are cut into tiles of 16.
// For the Gram tile (i-tile, j-tile) lane l holds, per k-step ks, the 16 bytes
// D[g, j_{16 it + (l & 15)}, 32 ks + 8 (l >> 4) ..] as the A fragment and the same bytes of the j-tile's
// atom as the B fragment: a gathered row feeds the matrix unit as it lies in memory.  Entries past L
// are zero fragments.  The i-tile's d / 32 fragments stay in registers while d <= 512 (CACHED); for a
// larger d both operands are loaded per k-step.  A diagonal tile uses the i-tile's registers twice, and
// a row of 17 .. 32 entries (two tiles, the common case at an L0 of 20 - 30) takes eight k-steps of both
// tiles at a time into four accumulators, so every atom is loaded once; a longer row loads the j-tile of
// an off-diagonal pair in two halves.  The paths differ in what they load, not in any sum's order.  The
// register budget (three waves per SIMD, the launch attribute below) is what the kernel's time follows.
// Accumulator: column b = lane & 15, row a = 4 (lane >> 4) + reg.
//
// fp32 order, fixed by the code: G_ab sums its k-steps ascending (inside a step the matrix unit's own
// order); within a j-tile the 16 terms cos2_ab * c_b of a row are summed over the lanes' low four bits by
// the butterfly (x + x^1) + ..., then ^2, ^4, ^8 (every lane of the 16 ends with the same bits); the
// j-tiles' sums are added to total_a in ascending tile order.  norm2: lane q of the 16 that share a
// row adds the squares of elements 8 q .. 8 q + 7, then 8 (q + 16) .., ascending, into one fp32, and the
// same butterfly joins the 16 lanes.
//
// Safety (the kernel gathers by indices it reads): a row is skipped -- it contributes nothing and adds 1
// to skipped[g] -- unless 0 <= row_ptr[g, r] <= row_ptr[g, r + 1] <= cap, L <= n, and every column is in
// [0, lim), lim = n or min(n, nactive[g]).  All columns are checked before the first gather, and every
// entry_cap store is behind pos < cap.
#include "code_lists.h"

namespace scamd {

constexpr int IC_ROWS = 4;       // rows (waves) per block
constexpr int IC_KS_REG = 16;    // k-steps of the i-tile kept in registers (d <= 512)

// Sum over the 16 lanes that share lane >> 4; every one of them gets the same bits.
__device__ __forceinline__ float sum16(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}

__global__ __launch_bounds__(256) void row_norm2_kernel(const uint16_t* __restrict__ D, float* __restrict__ norm2,
                                                        long rows, int d) {
  const int lane = threadIdx.x & 63, q = lane & 15;
  const long row = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
  float s = 0.f;
  if (row < rows) {
    const uint16_t* p = D + row * d;
    for (int k = 8 * q; k < d; k += 128) {
      const u32x4_t w = *reinterpret_cast<const u32x4_t*>(p + k);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t u = w[j >> 1];
        const float x = __uint_as_float((j & 1) ? (u & 0xffff0000u) : (u << 16));
        s = fmaf(x, x, s);
      }
    }
  }
  s = sum16(s);
  if (row < rows && q == 0) norm2[row] = s;
}

template <bool CACHED>
__global__ __launch_bounds__(64 * IC_ROWS) __attribute__((amdgpu_waves_per_eu(3))) void active_capacity_kernel(
    const long* __restrict__ row_ptr, long ldp, long row0, long n_rows, const int* __restrict__ col,
    const float* __restrict__ val, long cap, const uint16_t* __restrict__ D, const float* __restrict__ norm2,
    const int* __restrict__ nactive, int G, int n, int d, unsigned long long* __restrict__ qsum,
    unsigned long long* __restrict__ count, unsigned long long* __restrict__ skipped,
    float* __restrict__ entry_cap) {
  const int lane = threadIdx.x & 63, lc = lane & 15, lq = lane >> 4;
  const long id = (long)blockIdx.x * IC_ROWS + (threadIdx.x >> 6);  // (g, row) flattened
  if (id >= (long)G * n_rows) return;                                // (the whole wave)
  const int g = (int)(id / n_rows);
  const long r = id - (long)g * n_rows;
  const long lo = row_ptr[(long)g * ldp + row0 + r], hi = row_ptr[(long)g * ldp + row0 + r + 1];
  const int lim = live_limit(nactive, g, n);
  col += (long)g * cap;
  val += (long)g * cap;
  // ---- validate before anything is gathered (all tests wave-uniform)
  if (!csr_row_ok(lo, hi, cap, n, lim, col, lane)) {
    if (lane == 0) atomicAdd(skipped + g, 1ull);
    return;
  }
  const int L = (int)(hi - lo);
  if (L == 0) return;
  col += lo;
  val += lo;
  D += (long)g * n * d;
  norm2 += (long)g * n;
  const int nks = d >> 5, T = (L + 15) >> 4;
  const bf16x8_t zero = __builtin_bit_cast(bf16x8_t, u32x4_t{0u, 0u, 0u, 0u});

  // this lane's 16 bytes of k-step 0 of the atom of entry e (null past L: a zero fragment)
  auto frag_ptr = [&](int e) -> const uint16_t* { return e < L ? D + (long)col[e] * d + 8 * lq : nullptr; };
  auto load_tile = [&](bf16x8_t(&f)[IC_KS_REG], const uint16_t* p) {
#pragma unroll
    for (int ks = 0; ks < IC_KS_REG; ++ks) {
      f[ks] = zero;
      if (ks < nks && p) f[ks] = *reinterpret_cast<const bf16x8_t*>(p + 32 * ks);
    }
  };
  auto gram = [&](const bf16x8_t(&fa)[IC_KS_REG], const bf16x8_t(&fb)[IC_KS_REG]) {
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < IC_KS_REG; ++ks)
      if (ks < nks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[ks], fb[ks], acc, 0, 0, 0);
    return acc;
  };
  // clamped squared norms of the four entries a = 16 it + 4 lq + t whose totals this lane accumulates
  auto row_norms = [&](int it, float(&na)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int a = it * 16 + 4 * lq + t;
      na[t] = (a < L) ? fmaxf(norm2[col[a]], 1e-16f) : 1.f;
    }
  };
  // code and clamped squared norm of this lane's column b = 16 jt + lc of a j-tile (0 / 1 past L)
  auto col_terms = [&](int jt, float& cb, float& nb) {
    const int ej = jt * 16 + lc;
    cb = ej < L ? val[ej] : 0.f;
    nb = ej < L ? fmaxf(norm2[col[ej]], 1e-16f) : 1.f;
  };
  // the j-tile's sixteen terms cos2(a, b) c_b of each of the four rows, summed and added to the totals
  auto add_tile = [&](const f32x4_t& acc, const float(&na)[4], int it, int jt, float cb, float nb,
                      float(&total)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float term = (acc[t] * acc[t]) / (na[t] * nb) * cb;
      if (it * 16 + 4 * lq + t == jt * 16 + lc) term = cb;  // cos2(a, a) := 1: the diagonal adds exactly c_a
      total[t] += sum16(term);
    }
  };
  // lanes lc = 0 .. 3 of each 16 finish entry a = 16 it + 4 lq + lc
  auto finish = [&](int it, const float(&total)[4]) {
    const float tot = lc == 0 ? total[0] : lc == 1 ? total[1] : lc == 2 ? total[2] : total[3];
    const int a = it * 16 + 4 * lq + lc;
    if (lc < 4 && a < L) {
      const float cp = val[a] / fmaxf(tot, 1e-8f);
      const long long q = llrintf(cp * 4294967296.f);
      const long f = (long)g * n + col[a];
      atomicAdd(qsum + f, (unsigned long long)q);
      atomicAdd(count + f, 1ull);
      if (entry_cap && lo + a < cap) entry_cap[(long)g * cap + lo + a] = cp;
    }
  };

  if constexpr (CACHED) {
    if (T == 2) {  // (wave-uniform) 17 .. 32 entries: all four tile pairs at once, every atom loaded once
      const uint16_t* p[2] = {frag_ptr(lc), frag_ptr(16 + lc)};
      float cb[2], nb[2];
      col_terms(0, cb[0], nb[0]);
      col_terms(1, cb[1], nb[1]);
      f32x4_t acc[2][2] = {};
#pragma unroll
      for (int k0 = 0; k0 < IC_KS_REG; k0 += 8) {  // eight k-steps of both tiles at a time: 64 VGPRs
        if (k0 < nks) {
          bf16x8_t f[2][8];
#pragma unroll
          for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              f[s][u] = zero;
              if (k0 + u < nks && p[s]) f[s][u] = *reinterpret_cast<const bf16x8_t*>(p[s] + 32 * (k0 + u));
            }
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (k0 + u < nks) {
#pragma unroll
              for (int it = 0; it < 2; ++it)
#pragma unroll
                for (int jt = 0; jt < 2; ++jt)
                  acc[it][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[it][u], f[jt][u], acc[it][jt], 0, 0, 0);
            }
        }
      }
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        float na[4], total[4] = {0.f, 0.f, 0.f, 0.f};
        row_norms(it, na);
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) add_tile(acc[it][jt], na, it, jt, cb[jt], nb[jt], total);
        finish(it, total);
      }
      return;
    }
  }
  for (int it = 0; it < T; ++it) {
    const uint16_t* pa = frag_ptr(it * 16 + lc);
    float na[4], total[4] = {0.f, 0.f, 0.f, 0.f};
    row_norms(it, na);
    bf16x8_t fa[CACHED ? IC_KS_REG : 1];
    if constexpr (CACHED) load_tile(fa, pa);
    for (int jt = 0; jt < T; ++jt) {
      const uint16_t* pb = frag_ptr(jt * 16 + lc);
      float cb, nb;
      col_terms(jt, cb, nb);
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
      if constexpr (CACHED) {
        if (jt == it) {
          acc = gram(fa, fa);
        } else {  // the j-tile in two halves of eight k-steps: the register budget is the two-tile path's
#pragma unroll
          for (int k0 = 0; k0 < IC_KS_REG; k0 += 8) {
            bf16x8_t fb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              fb[u] = zero;
              if (k0 + u < nks && pb) fb[u] = *reinterpret_cast<const bf16x8_t*>(pb + 32 * (k0 + u));
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
              if (k0 + u < nks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[k0 + u], fb[u], acc, 0, 0, 0);
          }
        }
      } else {
        for (int ks = 0; ks < nks; ++ks) {
          const bf16x8_t a = pa ? *reinterpret_cast<const bf16x8_t*>(pa + 32 * ks) : zero;
          const bf16x8_t b = pb ? *reinterpret_cast<const bf16x8_t*>(pb + 32 * ks) : zero;
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
        }
      }
      add_tile(acc, na, it, jt, cb, nb, total);
    }
    finish(it, total);
  }
}

}  // namespace scamd

using namespace scamd;

extern "C" {

// D bf16 [G, n, d] -> norm2 fp32 [G, n].
int sc_row_norm2(const void* D, float* norm2, int G, int n, int d, hipStream_t stream) {
  if (!D || !norm2 || G < 1 || n < 1 || d < 32 || d % 32) return 1;
  const long rows = (long)G * n;
  unsigned blocks;
  if (!sc_grid(rows, 16, blocks)) return 1;
  hipLaunchKernelGGL(row_norm2_kernel, dim3(blocks), dim3(256), 0, stream,
                     reinterpret_cast<const uint16_t*>(D), norm2, rows, d);
  return sc_launched();
}

// Rows row0 .. row0 + n_rows - 1 of the CSR (row_ptr int64 [G, ldp], col int32 [G, cap], val fp32 [G, cap])
// against D bf16 [G, n, d] and norm2 fp32 [G, n]; nactive int32 [G] or null; qsum, count int64 [G, n] and
// skipped int64 [G] are added to; entry_cap fp32 [G, cap] or null.
int sc_active_capacity(const long* row_ptr, const int* col, const float* val, const void* D, const float* norm2,
                       const int* nactive, void* qsum, void* count, void* skipped, float* entry_cap, int G,
                       long n_rows, int n, int d, long ldp, long row0, long cap, hipStream_t stream) {
  if (!row_ptr || !col || !val || !D || !norm2 || !qsum || !count || !skipped) return 1;
  if (G < 1 || n < 1 || d < 32 || d % 32 || n_rows < 0 || row0 < 0 || ldp < row0 + n_rows + 1 || cap < 1) return 1;
  if (n_rows == 0) return 0;
  unsigned blocks;
  if (!sc_grid((long)G * n_rows, IC_ROWS, blocks)) return 1;
  auto kern = d <= 32 * IC_KS_REG ? active_capacity_kernel<true> : active_capacity_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(64 * IC_ROWS), 0, stream, row_ptr, ldp, row0, n_rows, col,
                     val, cap, reinterpret_cast<const uint16_t*>(D), norm2, nactive, G, n, d,
                     reinterpret_cast<unsigned long long*>(qsum), reinterpret_cast<unsigned long long*>(count),
                     reinterpret_cast<unsigned long long*>(skipped), entry_cap);
  return sc_launched();
}

}  // extern "C"
