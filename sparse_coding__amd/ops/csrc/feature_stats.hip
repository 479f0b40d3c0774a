// Per-feature activation statistics of stacked SAE codes (gfx950): column reductions of the bf16 code
// matrix c [G, B, n] the grouped encoder launch writes (B % 128 == 0, n % 128 == 0).
//
// col_moments_kernel: fp32 per-column partials of one row slab,
//   out[g, s, 0..5, j] = #(c != 0), sum c, sum c^2, sum c^3, sum c^4, max c   over rows [s R, (s+1) R)
//   one block per (model, slab, 128-column tile): 16 lanes x 16 B cover the tile's 256 B row segment, the
//   block's 16 row lanes walk the slab 16 rows at a time (eight rows in flight per thread).  Row lanes are
//   folded with two xor shuffles inside a wave and across the four waves through LDS in a fixed order:
//   no atomics, the same bits every run.  c^2 and c^3 of a bf16 value are exact in fp32, c^4 rounds once.
// col_topk_kernel: merges the batch into the running K largest strictly positive codes of every column,
//   top_vals fp32 [G, n, K] / top_rows int64 [G, n, K], ordered by (value descending, row ascending),
//   empty slots (0.0, -1).  One block per (model, 32-column tile) holds the tile's lists in LDS and
//   streams the batch in 128-row chunks (the loads of four chunks are in flight while one is
//   filtered).  Filter: a code must be strictly larger than its column's K-th value at the start of the
//   chunk -- rows arrive in increasing order, so an equal value can never displace a listed one -- and the
//   rare survivors go to per-column LDS queues.  One lane per column then inserts its survivors under the
//   total order (value, row), all columns at once: the result does not depend on the order a queue was
//   filled in.
#include "common.h"

namespace scamd {

constexpr int FS_STATS = 6;

__global__ __launch_bounds__(256) void col_moments_kernel(const uint16_t* __restrict__ c, float* __restrict__ out,
                                                          int B, int n, int R) {
  __shared__ float red[4][FS_STATS][128];
  const int tiles = n >> 7, S = B / R;
  const int tile = blockIdx.x % tiles;
  const int s = (blockIdx.x / tiles) % S;
  const int g = blockIdx.x / (tiles * S);
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const uint16_t* p = c + ((long)g * B + (long)s * R + rl) * n + tile * 128 + cl * 8;
  float cnt[8], s1[8], s2[8], s3[8], s4[8], mx[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    cnt[k] = s1[k] = s2[k] = s3[k] = s4[k] = 0.f;
    mx[k] = -INFINITY;
  }
  auto acc = [&](const u32x4_t q) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t w = q[k >> 1];
      const float v = __uint_as_float((k & 1) ? (w & 0xffff0000u) : (w << 16));
      const float v2 = v * v;
      cnt[k] += v != 0.f ? 1.f : 0.f;
      s1[k] += v;
      s2[k] += v2;
      s3[k] += v2 * v;
      s4[k] += v2 * v2;
      mx[k] = fmaxf(mx[k], v);
    }
  };
  int r = 0;
  for (; r + 128 <= R; r += 128) {  // eight rows in flight
    u32x4_t q[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) q[u] = *reinterpret_cast<const u32x4_t*>(p + (long)(r + 16 * u) * n);
#pragma unroll
    for (int u = 0; u < 8; ++u) acc(q[u]);
  }
  for (; r + 64 <= R; r += 64) {  // four
    const u32x4_t q0 = *reinterpret_cast<const u32x4_t*>(p + (long)r * n);
    const u32x4_t q1 = *reinterpret_cast<const u32x4_t*>(p + (long)(r + 16) * n);
    const u32x4_t q2 = *reinterpret_cast<const u32x4_t*>(p + (long)(r + 32) * n);
    const u32x4_t q3 = *reinterpret_cast<const u32x4_t*>(p + (long)(r + 48) * n);
    acc(q0); acc(q1); acc(q2); acc(q3);
  }
  for (; r < R; r += 16) acc(*reinterpret_cast<const u32x4_t*>(p + (long)r * n));
  // row lanes of a wave (lane bits 4, 5), then the four waves in order
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      cnt[k] += __shfl_xor(cnt[k], o, 64);
      s1[k] += __shfl_xor(s1[k], o, 64);
      s2[k] += __shfl_xor(s2[k], o, 64);
      s3[k] += __shfl_xor(s3[k], o, 64);
      s4[k] += __shfl_xor(s4[k], o, 64);
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o, 64));
    }
    if ((threadIdx.x & 63) < 16) {
      const int col = cl * 8 + k;
      red[w][0][col] = cnt[k];
      red[w][1][col] = s1[k];
      red[w][2][col] = s2[k];
      red[w][3][col] = s3[k];
      red[w][4][col] = s4[k];
      red[w][5][col] = mx[k];
    }
  }
  __syncthreads();
  float* o = out + ((long)g * S + s) * FS_STATS * n + tile * 128;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int idx = threadIdx.x + i * 256, st = idx >> 7, col = idx & 127;
    const float a0 = red[0][st][col], a1 = red[1][st][col], a2 = red[2][st][col], a3 = red[3][st][col];
    o[(long)st * n + col] = st == 5 ? fmaxf(fmaxf(a0, a1), fmaxf(a2, a3)) : ((a0 + a1) + (a2 + a3));
  }
}

constexpr int TK_COLS = 32;     // columns per block
constexpr int TK_CHUNK = 128;   // rows per filter / insert round
constexpr int TK_MAXK = 32;
constexpr int TK_THREADS = 512;
constexpr int TK_CL = TK_COLS / 8;            // column lanes (16 B each)
constexpr int TK_RL = TK_THREADS / TK_CL;     // row lanes
constexpr int TK_U = TK_CHUNK / TK_RL;        // rows of a chunk per thread
constexpr int TK_AHEAD = 4;     // chunks in flight

__global__ __launch_bounds__(TK_THREADS) void col_topk_kernel(const uint16_t* __restrict__ c,
                                                              float* __restrict__ top_vals,
                                                              long* __restrict__ top_rows, int B, int n, int K,
                                                              long row0) {
  __shared__ float lv[TK_MAXK * TK_COLS];          // [k][col]
  __shared__ long lr[TK_MAXK * TK_COLS];           // [k][col]
  __shared__ uint32_t queue[TK_CHUNK * TK_COLS];   // [slot][col]: bf16 bits << 16 | row in chunk
  __shared__ int qcount[2][TK_COLS];               // survivors per column, double-buffered by chunk parity
  const int tiles = n / TK_COLS;
  const int tile = blockIdx.x % tiles, g = blockIdx.x / tiles;
  const int t = threadIdx.x, cl = t % TK_CL, rl = t / TK_CL;
  const long sbase = ((long)g * n + tile * TK_COLS) * K;
  for (int i = t; i < TK_COLS * K; i += TK_THREADS) {
    const int col = i / K, k = i - col * K;
    lv[k * TK_COLS + col] = top_vals[sbase + i];
    lr[k * TK_COLS + col] = top_rows[sbase + i];
  }
  if (t < 2 * TK_COLS) qcount[t / TK_COLS][t % TK_COLS] = 0;
  const uint16_t* p = c + ((long)g * B + rl) * n + tile * TK_COLS + cl * 8;
  const int chunks = B / TK_CHUNK;
  u32x4_t buf[TK_AHEAD][TK_U];
#pragma unroll
  for (int s = 0; s < TK_AHEAD; ++s) {
    if (s < chunks) {
#pragma unroll
      for (int u = 0; u < TK_U; ++u)
        buf[s][u] = *reinterpret_cast<const u32x4_t*>(p + (long)(s * TK_CHUNK + u * TK_RL) * n);
    }
  }
  __syncthreads();
  for (int ch0 = 0; ch0 < chunks; ch0 += TK_AHEAD) {
#pragma unroll
    for (int s = 0; s < TK_AHEAD; ++s) {
      const int ch = ch0 + s;
      if (ch >= chunks) break;
      u32x4_t cur[TK_U];
#pragma unroll
      for (int u = 0; u < TK_U; ++u) cur[u] = buf[s][u];
      if (ch + TK_AHEAD < chunks) {  // (the barriers below wait for LDS only: these loads stay in flight)
#pragma unroll
        for (int u = 0; u < TK_U; ++u)
          buf[s][u] = *reinterpret_cast<const u32x4_t*>(p + (long)((ch + TK_AHEAD) * TK_CHUNK + u * TK_RL) * n);
      }
      float thr[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) thr[k] = lv[(K - 1) * TK_COLS + cl * 8 + k];
      int* qc = qcount[ch & 1];
#pragma unroll
      for (int u = 0; u < TK_U; ++u) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint32_t w = cur[u][k >> 1];
          const uint32_t bits = (k & 1) ? (w & 0xffff0000u) : (w << 16);
          if (__uint_as_float(bits) > thr[k]) {
            const int col = cl * 8 + k;
            const int slot = atomicAdd(&qc[col], 1);  // (< TK_CHUNK: one slot per row of the chunk)
            queue[slot * TK_COLS + col] = bits | (uint32_t)(u * TK_RL + rl);
          }
        }
      }
      lds_barrier();
      if (t < TK_COLS) {  // one lane per column: sorted inserts under (value descending, row ascending)
        const int cnt = qc[t];
        qcount[(ch + 1) & 1][t] = 0;
        const long rbase = row0 + (long)ch * TK_CHUNK;
        for (int i = 0; i < cnt; ++i) {
          const uint32_t e = queue[i * TK_COLS + t];
          const float v = __uint_as_float(e & 0xffff0000u);
          const long row = rbase + (e & 0xffffu);
          int j = K - 1;
          {  // (an empty slot is (0, -1) and v > 0)
            const float ev = lv[j * TK_COLS + t];
            const long er = lr[j * TK_COLS + t];
            if (!(v > ev || (v == ev && row < er))) continue;
          }
          while (j > 0) {
            const float ev = lv[(j - 1) * TK_COLS + t];
            const long er = lr[(j - 1) * TK_COLS + t];
            if (!(v > ev || (v == ev && row < er))) break;
            lv[j * TK_COLS + t] = ev;
            lr[j * TK_COLS + t] = er;
            --j;
          }
          lv[j * TK_COLS + t] = v;
          lr[j * TK_COLS + t] = row;
        }
      }
      lds_barrier();
    }
  }
  for (int i = t; i < TK_COLS * K; i += TK_THREADS) {
    const int col = i / K, k = i - col * K;
    top_vals[sbase + i] = lv[k * TK_COLS + col];
    top_rows[sbase + i] = lr[k * TK_COLS + col];
  }
}

}  // namespace scamd

using namespace scamd;

extern "C" {

// out fp32 [G, S, 6, n]; S slabs of B / S rows each (a multiple of 16).
int sc_col_moments(const void* c, float* out, int G, int B, int n, int S, hipStream_t stream) {
  if (!c || !out || G < 1 || B < 128 || B % 128 || n < 128 || n % 128 || S < 1 || B % S || (B / S) % 16) return 1;
  unsigned blocks;
  if (!sc_grid((long)G * S * (n / 128), 1, blocks)) return 1;
  hipLaunchKernelGGL(col_moments_kernel, dim3(blocks), dim3(256), 0, stream,
                     reinterpret_cast<const uint16_t*>(c), out, B, n, B / S);
  return sc_launched();
}

// top_vals fp32 [G, n, K], top_rows int64 [G, n, K], 1 <= K <= 32; the batch's rows are row0 .. row0 + B - 1.
int sc_col_topk(const void* c, float* top_vals, long* top_rows, int G, int B, int n, int K, long row0,
                hipStream_t stream) {
  if (!c || !top_vals || !top_rows || G < 1 || B < 128 || B % 128 || n < 128 || n % 128 || K < 1 || K > TK_MAXK ||
      row0 < 0)
    return 1;
  unsigned blocks;
  if (!sc_grid((long)G * (n / TK_COLS), 1, blocks)) return 1;
  hipLaunchKernelGGL(col_topk_kernel, dim3(blocks), dim3(TK_THREADS), 0, stream,
                     reinterpret_cast<const uint16_t*>(c), top_vals, top_rows, B, n, K, row0);
  return sc_launched();
}

}  // extern "C"
