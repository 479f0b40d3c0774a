// Row helpers shared by the kernels that keep one bf16 row of d = 64 P elements per wave in registers
// (sparse_recon.hip, attribution.hip): the lane / element layout, the packed row load, the fp32 axpy and the
// squared norm.  The fp32 orders written here are contracts: the oracles emulate them and the tests compare
// bits.  The skip rule of a CSR row and the live column limit come with code_lists.h.
#pragma once
#include "code_lists.h"

namespace scamd {

constexpr int SR_ROWS = 4;   // rows (waves) per block
constexpr int SR_AHEAD = 4;  // atoms gathered ahead of their use

// Lane l keeps P elements, cut into pieces of V = 8, 4, 2 or 1 elements (the largest that divides P): element
// i = p V + j of the lane is k = 64 V p + V l + j, so one piece is one 16-, 8-, 4- or 2-byte load per lane.
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
  return wave_sum_xor<true>(s);
}

}  // namespace scamd

// Host-side argument check of a launch over rows row0 .. row0 + n_rows - 1 (one wave per (model, row)).
static inline bool sr_bad_rows(const void* row_ptr, const void* col, const void* val, const void* D, const void* x,
                               const void* out, const void* skipped, int G, long n_rows, int n, int d, long ldp,
                               long row0, long cap, long x_stride) {
  if (!row_ptr || !col || !val || !D || !x || !out || !skipped) return true;
  if (G < 1 || n < 1 || d < 64 || d > 1024 || d % 64) return true;
  if (n_rows < 0 || row0 < 0 || ldp < row0 + n_rows + 1 || cap < 0) return true;
  if (x_stride != 0 && x_stride < n_rows * (long)d) return true;
  return ((long)G * n_rows + scamd::SR_ROWS - 1) / scamd::SR_ROWS > 0x7fffffffL;
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
