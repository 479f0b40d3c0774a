// Dead-feature resampling for stacked SAE dictionaries (gfx950).
//
// row_sqerr_kernel: per-row squared reconstruction error of a pool batch,
//   err[g, off + b] = sum_j r[g, b, j]^2,  r bf16 [G, B, d] (the decoder's residual), err fp32 [G, N]
//   one wave per row, 16-byte loads, fp32 accumulation.
// resample_rows_kernel: re-seeds a ragged per-model list of dictionary rows from pool rows, one wave
//   per (model g, pair j < cnt[g]) with cnt read on the device (no host sync, graph-capturable).
//   For f = dead_idx[g, j] and v = float(rows[src_idx[g, j]]):
//     encoder master row <- u enc_scale[g], u = v / max(|v|, 1e-8) (normalize_src) or v; m, v <- 0
//     decoder (untied)   <- v / max(|v|, 1e-8) if set_decoder;                           m, v <- 0
//     bias[g, f]         <- 0 if zero_bias;                                              m, v <- 0
//   and the bf16 shadows / row norms of the rewritten rows through shadow_row (row_adam.h), the body
//   of sc_shadow_rows: the same reduction order, the same bits.
//   The three bias pointers may be null (sc_resample_dict_rows: a normalised dictionary with no bias,
//   the top-k ensembles): the dictionary goes in the enc* slots with norms given, decoder null.
//   (Anthropic's "Towards Monosemanticity" resampling; reference experiments/huge_batch_size.py:
//   224-250 is the un-normalised, encoder-only case.)
#include "common.h"
#include "row_adam.h"

namespace scamd {

__global__ __launch_bounds__(256) void row_sqerr_kernel(const uint16_t* __restrict__ r, float* __restrict__ err,
                                                        long rows, int B, int d, long N, long off) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const uint16_t* R = r + row * d;
  float ss = 0.f;
  for (int e = lane * 8; e < d; e += 512) {
    const u32x4_t q = *reinterpret_cast<const u32x4_t*>(R + e);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float lo = __uint_as_float(q[k] << 16), hi = __uint_as_float(q[k] & 0xffff0000u);
      ss += lo * lo + hi * hi;
    }
  }
  ss = wave_sum(ss);
  if (lane == 0) err[(row / B) * N + off + row % B] = ss;
}

struct ResampleArgs {
  const int* dead_idx;    // [G][P] rows to rewrite
  const long* src_idx;    // [G][P] pool rows they are seeded from
  const int* cnt;         // [G] pairs in use per model (device)
  int P;
  const uint16_t* rows;   // [N][d] bf16 pool
  long N;
  const float* enc_scale; // [G]
  int normalize_src, set_decoder, zero_bias;
  float *enc, *enc_m, *enc_v;
  uint16_t* enc_shadow;
  float *dec, *dec_m, *dec_v;  // null: tied dictionary
  uint16_t* dec_shadow;
  float *bias, *bias_m, *bias_v;  // [G][n]; all null: no bias
  float* norms;                   // [G][n] row norms of the normalised dictionary
  int G, n, d;
};

template <int NV>
__global__ __launch_bounds__(256) void resample_rows_kernel(ResampleArgs a) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int g = (int)(wave / a.P), j = (int)(wave % a.P);
  if (g >= a.G || j >= a.cnt[g]) return;
  const int f = a.dead_idx[(long)g * a.P + j];
  const long src = a.src_idx[(long)g * a.P + j];
  if (f < 0 || f >= a.n || src < 0 || src >= a.N) return;  // (a malformed list edits nothing)
  const long row = (long)g * a.n + f;
  const long base = row * a.d;
  const uint16_t* S = a.rows + src * a.d;
  float4 sv[NV];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const ushort4 h = *reinterpret_cast<const ushort4*>(S + (i * 64 + lane) * 4);
    sv[i] = make_float4(bf2f(h.x), bf2f(h.y), bf2f(h.z), bf2f(h.w));
    ss += sv[i].x * sv[i].x + sv[i].y * sv[i].y + sv[i].z * sv[i].z + sv[i].w * sv[i].w;
  }
  const bool untied = a.dec != nullptr;
  const bool wdec = untied && a.set_decoder;
  float nrm = 1.f;
  if (a.normalize_src || wdec) nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-8f);
  const float es = a.enc_scale[g];
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int e = (i * 64 + lane) * 4;
    const float4 s = sv[i];
    const float4 un = make_float4(s.x / nrm, s.y / nrm, s.z / nrm, s.w / nrm);
    const float4 u = a.normalize_src ? un : s;
    *reinterpret_cast<float4*>(a.enc + base + e) = make_float4(u.x * es, u.y * es, u.z * es, u.w * es);
    *reinterpret_cast<float4*>(a.enc_m + base + e) = z4;
    *reinterpret_cast<float4*>(a.enc_v + base + e) = z4;
    if (untied) {
      if (wdec) *reinterpret_cast<float4*>(a.dec + base + e) = un;
      *reinterpret_cast<float4*>(a.dec_m + base + e) = z4;
      *reinterpret_cast<float4*>(a.dec_v + base + e) = z4;
    }
  }
  if (lane == 0) {
    if (a.zero_bias && a.bias) a.bias[row] = 0.f;
    if (a.bias_m) a.bias_m[row] = 0.f;
    if (a.bias_v) a.bias_v[row] = 0.f;
  }
  // shadows and norms of the rows that changed, from the masters just written (each lane reads back
  // exactly the elements it stored)
  if (untied) {
    shadow_row(a.enc + base, a.enc_shadow + base, nullptr, a.d, 0, lane);
    if (wdec) shadow_row(a.dec + base, a.dec_shadow + base, a.norms + row, a.d, 1, lane);
  } else {
    shadow_row(a.enc + base, a.enc_shadow + base, a.norms + row, a.d, 1, lane);
  }
}

}  // namespace scamd

using namespace scamd;

extern "C" {

int sc_row_sqerr(const void* r, float* err, int G, int B, int d, long N, long off, hipStream_t stream) {
  if (d % 256 || d < 256 || G < 1 || B < 1 || off < 0 || off + B > N) return 1;
  const long rows = (long)G * B;
  hipLaunchKernelGGL(row_sqerr_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream,
                     reinterpret_cast<const uint16_t*>(r), err, rows, B, d, N, off);
  return sc_launched();
}

static int launch_resample(const ResampleArgs& a, int P, hipStream_t stream) {
  const long blocks = ((long)a.G * P + 3) / 4;
#define SC_RESAMPLE(NVV)                                                                        \
  case NVV:                                                                                     \
    hipLaunchKernelGGL((resample_rows_kernel<NVV>), dim3(blocks), dim3(256), 0, stream, a);     \
    break;
  switch (a.d / 256) {
    SC_RESAMPLE(1) SC_RESAMPLE(2) SC_RESAMPLE(3) SC_RESAMPLE(4) SC_RESAMPLE(6) SC_RESAMPLE(8) SC_RESAMPLE(16)
    default: return 1;
  }
#undef SC_RESAMPLE
  return sc_launched();
}

int sc_resample_rows(const int* dead_idx, const long* src_idx, const int* cnt, int P, const void* rows, long N,
                     const float* enc_scale, int normalize_src, int set_decoder, int zero_bias, float* enc,
                     float* enc_m, float* enc_v, void* enc_shadow, float* dec, float* dec_m, float* dec_v,
                     void* dec_shadow, float* bias, float* bias_m, float* bias_v, float* norms, int G,
                     int rows_per_model, int d, hipStream_t stream) {
  if (d % 256 || d > 4096 || G < 1 || P < 1 || N < 1 || rows_per_model < 1) return 1;
  if (!dead_idx || !src_idx || !cnt || !rows || !enc_scale || !enc || !enc_m || !enc_v || !enc_shadow || !bias ||
      !bias_m || !bias_v || !norms)
    return 1;
  if (dec && (!dec_m || !dec_v || !dec_shadow)) return 1;
  ResampleArgs a;
  a.dead_idx = dead_idx; a.src_idx = src_idx; a.cnt = cnt; a.P = P;
  a.rows = reinterpret_cast<const uint16_t*>(rows); a.N = N; a.enc_scale = enc_scale;
  a.normalize_src = normalize_src; a.set_decoder = set_decoder; a.zero_bias = zero_bias;
  a.enc = enc; a.enc_m = enc_m; a.enc_v = enc_v; a.enc_shadow = reinterpret_cast<uint16_t*>(enc_shadow);
  a.dec = dec; a.dec_m = dec_m; a.dec_v = dec_v; a.dec_shadow = reinterpret_cast<uint16_t*>(dec_shadow);
  a.bias = bias; a.bias_m = bias_m; a.bias_v = bias_v; a.norms = norms;
  a.G = G; a.n = rows_per_model; a.d = d;
  return launch_resample(a, P, stream);
}

// A normalised dictionary with no bias and no separate decoder (the top-k ensembles): row dead_idx[g, j]
// of `dict` <- u scale[g] (u the unit pool row if normalize_src, else the raw row), m, v <- 0, and the
// normalised bf16 shadow / row norm of the row through shadow_row.
int sc_resample_dict_rows(const int* dead_idx, const long* src_idx, const int* cnt, int P, const void* rows, long N,
                          const float* scale, int normalize_src, float* dict, float* dict_m, float* dict_v,
                          void* shadow, float* norms, int G, int rows_per_model, int d, hipStream_t stream) {
  if (d % 256 || d > 4096 || G < 1 || P < 1 || N < 1 || rows_per_model < 1) return 1;
  if (!dead_idx || !src_idx || !cnt || !rows || !scale || !dict || !dict_m || !dict_v || !shadow || !norms) return 1;
  ResampleArgs a;
  a.dead_idx = dead_idx; a.src_idx = src_idx; a.cnt = cnt; a.P = P;
  a.rows = reinterpret_cast<const uint16_t*>(rows); a.N = N; a.enc_scale = scale;
  a.normalize_src = normalize_src; a.set_decoder = 0; a.zero_bias = 0;
  a.enc = dict; a.enc_m = dict_m; a.enc_v = dict_v; a.enc_shadow = reinterpret_cast<uint16_t*>(shadow);
  a.dec = a.dec_m = a.dec_v = nullptr; a.dec_shadow = nullptr;
  a.bias = a.bias_m = a.bias_v = nullptr; a.norms = norms;
  a.G = G; a.n = rows_per_model; a.d = d;
  return launch_resample(a, P, stream);
}

}  // extern "C"
