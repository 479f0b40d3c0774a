// Shared CDNA4 (gfx950) helpers for the sparse-coding kernels.
//
// Everything here is wave64 / MFMA specific: this code is written for MI355X
// only (hipcc --offload-arch=gfx950) and has no other target.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace scamd {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef short i16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------ global-store cache policy
// The eight XCD L2s are write-back and not coherent with each other, so the release at the end of a
// kernel writes every dirty line back before the dependent kernel starts.  An `sc1` store is written
// through: its bytes leave the L2 while the kernel is still running (MI355X_MICROARCH.md, "stores of
// each flavour").  `nt` alone only changes retention.  The values are the `aux` operand of the raw
// buffer stores, which is the only compiler-visible 16-byte store that takes `sc1` (an inline-asm
// store would not be counted in hipcc's vmcnt bookkeeping).  Cache hints only: every policy writes
// the same bits.
enum { ST_PLAIN = 0, ST_NT = 2, ST_SC1 = 16, ST_NT_SC1 = 18 };

// Buffer resource over [base, base + 2^31 - 1) for st_pol's written-through forms: byte offsets are
// 32-bit, so the host keeps write-through off for any output that spans more (ops/store_policy.py).
// `base` must be wave-uniform; the readfirstlanes make that provable (no waterfall loops).
typedef __amdgpu_buffer_rsrc_t rsrc_t;

// A 64-bit value every lane holds, handed on as a provably wave-uniform one (two readfirstlanes).
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ rsrc_t store_rsrc(const void* base) {
  const uint64_t a = uniform_u64(reinterpret_cast<uint64_t>(base));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(a), 0, 0x7FFFFFFF, 0x00020000);
}

// One whole 16-byte or 8-byte store of `v` at base + off under policy POL.  The plain and `nt` forms
// address base + off in 64 bits (any span); the `sc1` forms go through `rs` = store_rsrc(base).
template <int POL, class V>
__device__ __forceinline__ void st_pol(const rsrc_t& rs, void* base, long off, const V& v) {
  static_assert(sizeof(V) == 16 || sizeof(V) == 8, "whole 16-byte or 8-byte pieces only");
  using U = typename std::conditional<sizeof(V) == 16, u32x4_t, u32x2_t>::type;
  const U u = __builtin_bit_cast(U, v);
  if constexpr (POL == ST_PLAIN) {
    *reinterpret_cast<U*>(reinterpret_cast<char*>(base) + off) = u;
  } else if constexpr (POL == ST_NT) {
    __builtin_nontemporal_store(u, reinterpret_cast<U*>(reinterpret_cast<char*>(base) + off));
  } else if constexpr (sizeof(V) == 16) {
    __builtin_amdgcn_raw_buffer_store_b128(u, rs, (int)off, 0, POL);
  } else {
    __builtin_amdgcn_raw_buffer_store_b64(u, rs, (int)off, 0, POL);
  }
}

// Run-time choice between the plain and the written-through store (wave-uniform `wt`).
template <class V>
__device__ __forceinline__ void st_out(bool wt, const rsrc_t& rs, void* base, long off, const V& v) {
  if (wt) st_pol<ST_SC1>(rs, base, off, v);
  else st_pol<ST_PLAIN>(rs, base, off, v);
}

#define SC_LDS(T, p) ((__attribute__((address_space(3))) T*)(p))

__device__ __forceinline__ float bf2f(uint16_t h) {
  return __uint_as_float(((uint32_t)h) << 16);
}

// Round-to-nearest-even f32 -> bf16 (hipcc lowers the cast to v_cvt_pk_bf16_f32,
// which keeps NaN a NaN).
__device__ __forceinline__ uint16_t f2bf(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(uint16_t, b);
}

// DPP lane shuffle of a float (row_shr / row_bcast controls; lanes whose source is outside
// the row read 0, so adding the result is a scan step).
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}

// Inclusive scan within each 16-lane row: lane 15 of a row ends with the row's sum.
__device__ __forceinline__ float row16_scan(float v) {
  v += dpp_f<0x111>(v);  // row_shr:1
  v += dpp_f<0x112>(v);  // row_shr:2
  v += dpp_f<0x114>(v);  // row_shr:4
  v += dpp_f<0x118>(v);  // row_shr:8
  return v;
}

// Wave-wide sum on the DPP path (row scans, row broadcasts, lane 63 read back): six VALU
// adds and a readlane instead of six ds_bpermute round trips.  Uniform result.
__device__ __forceinline__ float wave_sum(float v) {
  v = row16_scan(v);
  v += dpp_f<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
  v += dpp_f<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Wave-wide sum by the xor butterfly: every lane ends with the same bits.  ASCENDING joins the lanes at
// offsets 1, 2, 4, 8, 16, 32, the other order at 32, 16, 8, 4, 2, 1.  The two orders round differently
// in fp32 and fp64, and each caller's order is a contract that its oracle emulates bit for bit: both
// stay, and a caller keeps the one it has.  (Integers: either order, the same bits.)
template <bool ASCENDING, class T>
__device__ __forceinline__ T wave_sum_xor(T v) {
  if constexpr (ASCENDING) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = v + __shfl_xor(v, o, 64);
  } else {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  }
  return v;
}

// LDS hand-off between the lanes of ONE wave (LDS operations of a wave complete in order).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Order-preserving map of an fp32 bit pattern to unsigned integers (larger float -> larger key): a total
// order on all bit patterns, so -0.0 sorts before +0.0 and every NaN has its place.
__device__ __forceinline__ uint32_t order_key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t order_key(float f) { return order_key(__float_as_uint(f)); }

// Block-wide sum for a 256-thread block; `red` must hold >= 4 floats of LDS.
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float r = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return r;
}

// Block-wide sum over NW waves; `red` must hold >= NW floats of LDS.
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) r += red[i];
  __syncthreads();
  return r;
}

// Workgroup barrier for LDS hand-offs only: waits for this wave's LDS ops, not for its
// global stores / loads / LDS-DMAs (a __syncthreads() would drain vmcnt too).
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// block_sum with LDS-only barriers (see lds_barrier); `red` must hold >= NW floats.
template <int NW>
__device__ __forceinline__ float block_sum_lds(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  lds_barrier();
  if (lane == 0) red[w] = v;
  lds_barrier();
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) r += red[i];
  lds_barrier();
  return r;
}

// Two block-wide sums behind ONE LDS-only barrier, for a block's last reduction: `red` (>= 2 NW
// floats) is not reused afterwards, so the barrier that protects a reused scratch is not needed.
// Every thread gets both totals (same summation order as block_sum_lds: bit-identical).
template <int NW>
__device__ __forceinline__ float2 block_sum2_final(float a, float b, float* red) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    red[2 * w] = a;
    red[2 * w + 1] = b;
  }
  lds_barrier();
  float2 r = make_float2(0.f, 0.f);
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    r.x += red[2 * i];
    r.y += red[2 * i + 1];
  }
  return r;
}

// Bijective XCD-aware block remap (MI355X has 8 XCDs, each with its own L2).
// Hardware hands consecutive block ids to different XCDs round-robin; this
// gives each XCD a contiguous run of logical tiles so neighbouring tiles that
// share operand panels hit the same L2.
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (orig >> 3);
}

}  // namespace scamd

// ------------------------------------------------------------------ host side of every entry point
// What an entry point returns after its launches: 0 when they were accepted, 3 otherwise.
static inline int sc_launched() { return hipGetLastError() == hipSuccess ? 0 : 3; }

// blocks = the blocks of `per` items that cover `work`; false when a 1-D grid cannot hold them.
static inline bool sc_grid(long work, long per, unsigned& blocks) {
  const long b = (work + per - 1) / per;
  blocks = (unsigned)b;
  return b <= 0x7fffffffL;
}
