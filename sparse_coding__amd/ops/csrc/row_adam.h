// Row-wise fused Adam for stacked dictionary parameters (gfx950): the per-row core of the Adam
// kernels (adam.hip).  (A deferred decoder update run by the encoder GEMM after its tiles shared it
// in round 6 -- bit-identical, but slower: scripts/lab/deferred_decoder_adam_r6.patch.)
// Reference semantics: torchopt 0.7.1 `adam` vmapped over the model axis (autoencoders/ensemble.py:
// 94-95, :123, :182-191) with the decoder row normalisation inside the loss (sae_ensemble.py:58-59).
#pragma once
#include "common.h"

namespace scamd {

// Adam bias corrections for 1-based step t, computed on the device so a captured
// HIP graph replays correctly step after step.
__device__ __forceinline__ void bias_corrections(float b1, float b2, int t, float& bc1, float& bc2) {
  bc1 = 1.f - __powf(b1, (float)t);
  bc2 = 1.f - __powf(b2, (float)t);
}

// One row of a bf16 shadow from its fp32 master, one wave: P -> S (row-normalised if norm, the row
// norm to *nrm_out).  The per-row body of shadow_rows_kernel (adam.hip), shared with the resampling
// kernel (resample.hip) so that both reduce the norm in one order and write the same bits.
__device__ __forceinline__ void shadow_row(const float* P, uint16_t* S, float* nrm_out, int d, int norm, int lane) {
  float ss = 0.f;
  for (int e = lane * 4; e < d; e += 256) {
    const float4 v = *reinterpret_cast<const float4*>(P + e);
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  float sc = 1.f;
  if (norm) {
    ss = wave_sum(ss);
    const float nrm = fmaxf(sqrtf(ss), 1e-8f);
    sc = 1.f / nrm;
    if (nrm_out && lane == 0) *nrm_out = nrm;
  }
  for (int e = lane * 4; e < d; e += 256) {
    const float4 v = *reinterpret_cast<const float4*>(P + e);
    ushort4 h;
    h.x = f2bf(v.x * sc);
    h.y = f2bf(v.y * sc);
    h.z = f2bf(v.z * sc);
    h.w = f2bf(v.w * sc);
    *reinterpret_cast<ushort4*>(S + e) = h;
  }
}

// Cache policy of the fp32 master / moment streams (p, m, v: touched once per step, so caching them only
// costs the GEMM operands their place): bit 0 streams the loads, bit 1 the stores (non-temporal).  The
// gradient loads and the bf16 shadow / row-norm stores keep the default policy: the weight gradient has
// just written the one, the next step's GEMMs read the others.
constexpr int POL_NT_LOAD = 1, POL_NT_STORE = 2;
// Bits 2 and 3 (ops/store_policy.py; step tails only): the p / m / v stores, and the bf16 shadow / row-norm
// stores, written through the L2 (`sc1`, common.h st_pol) so that the end of the launch does not have to
// write them back; POL_WT_PMV on top of POL_NT_STORE gives `nt sc1`.  Compile-time like bits 0 and 1, and
// the code without them is left exactly as it was: a run-time branch around the stores changed how the
// compiler fused the update's multiply-adds (other bits, see below).  The written-through forms address a
// whole parameter set with 32-bit byte offsets; the launchers drop the bits for larger sets.
constexpr int POL_WT_PMV = 4, POL_WT_AUX = 8;

template <bool NT>
__device__ __forceinline__ float4 ld_f4(const float* p) {
  if constexpr (NT) {
    const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
  } else {
    return *reinterpret_cast<const float4*>(p);
  }
}

template <bool NT>
__device__ __forceinline__ void st_f4(float* p, const float4& v) {
  if constexpr (NT) {
    __builtin_nontemporal_store(__builtin_bit_cast(f32x4_t, v), reinterpret_cast<f32x4_t*>(p));
  } else {
    *reinterpret_cast<float4*>(p) = v;
  }
}

// One dictionary row of the fused Adam, one wave (d = 256 NV): applies the norm Jacobian (norm rows),
// the Adam update, recomputes the row norm and writes the bf16 shadow (normalised for norm rows).
// GBF: the gradient arrives in bf16 (the weight-gradient GEMM's bf16 epilogue): 1/7 of the HBM bytes
// less to read; the moments, the master and the update arithmetic stay fp32.  nsplit > 1: the
// gradient arrives as split-K partial slabs gstride elements apart (summed here).
template <int NV, bool GBF = false, int POL = 0>
__device__ __forceinline__ void adam_row_core(float* P, const void* G, float* M, float* V, uint16_t* shadow,
                                              float* norms, long row, int norm, int nsplit, long gstride, float lr,
                                              float b1, float b2, float eps, float bc1, float bc2, int lane) {
  constexpr bool NTL = (POL & POL_NT_LOAD) != 0, NTS = (POL & POL_NT_STORE) != 0;
  constexpr bool WTP = (POL & POL_WT_PMV) != 0, WTA = (POL & POL_WT_AUX) != 0;
  constexpr int PMV_POL = (NTS ? ST_NT : ST_PLAIN) | ST_SC1;  // the written-through p / m / v store
  const int d = NV * 256;
  const long base = row * d;
  // NV float4 chunks per lane (d == 256 * NV); compile-time so pv/gv stay in VGPRs.
  const float* P4 = P + base;
  const float* G4 = reinterpret_cast<const float*>(G) + base;
  const uint16_t* GH = reinterpret_cast<const uint16_t*>(G) + base;

  // every load of the row is issued up front (p, g, m, v: 4 NV float4 per lane in flight)
  // so one memory round trip covers the row; the moments do not wait for the norm reductions
  float4 pv[NV], gv[NV], mv_[NV], vv_[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int e = (i * 64 + lane) * 4;
    pv[i] = ld_f4<NTL>(P4 + e);
    if constexpr (GBF) {
      const ushort4 h = *reinterpret_cast<const ushort4*>(GH + e);
      gv[i] = make_float4(bf2f(h.x), bf2f(h.y), bf2f(h.z), bf2f(h.w));
    } else {
      gv[i] = *reinterpret_cast<const float4*>(G4 + e);
    }
    mv_[i] = ld_f4<NTL>(M + base + e);
    vv_[i] = ld_f4<NTL>(V + base + e);
  }
  if (nsplit > 1) {  // split-K partials of the weight-gradient GEMM (few-model shards)
    for (int sp = 1; sp < nsplit; ++sp) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const long e = sp * gstride + (i * 64 + lane) * 4;
        float4 q;
        if constexpr (GBF) {
          const ushort4 h = *reinterpret_cast<const ushort4*>(GH + e);
          q = make_float4(bf2f(h.x), bf2f(h.y), bf2f(h.z), bf2f(h.w));
        } else {
          q = *reinterpret_cast<const float4*>(G4 + e);
        }
        gv[i].x += q.x; gv[i].y += q.y; gv[i].z += q.z; gv[i].w += q.w;
      }
    }
  }
  // Where a sum of products can be fused into multiply-adds in more than one way, the way is written
  // out (`a * b + c * d` is fma(a, b, c * d) or fma(c, d, a * b): two roundings of two different
  // products).  Left to the compiler, the choice moved with the cache policy of the stores -- the
  // streamed-store builds of d >= 512 fused <w, g> the other way round and wrote other bits -- so the
  // forms below are the ones every build took before there was a policy.
  float ss = 0.f, dot = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float4 p = pv[i], g = gv[i];
    ss += __fmaf_rn(p.w, p.w, __fmaf_rn(p.z, p.z, __fmaf_rn(p.x, p.x, p.y * p.y)));
    dot += __fmaf_rn(p.w, g.w, __fmaf_rn(p.z, g.z, __fmaf_rn(p.x, g.x, p.y * g.y)));
  }
  float gs = 1.f, ws = 0.f;
  if (norm) {
    ss = wave_sum(ss);
    dot = wave_sum(dot);
    const float nrm = sqrtf(ss);
    if (nrm > 1e-8f) {
      const float inv = 1.f / nrm;
      gs = inv;                 // g' = (g - w_hat <w_hat, g>) / |w|
      ws = dot * inv * inv * inv;  // w_hat <w_hat,g> / |w| = w <w,g> / |w|^3
    } else {
      gs = 1e8f;                // clamp(min=1e-8) has zero derivative below the floor
      ws = 0.f;
    }
  }
  const float omb1 = 1.f - b1, omb2 = 1.f - b2;
  const float step = lr / bc1, rbc2 = 1.f / bc2;
  float ss2 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int e = (i * 64 + lane) * 4;
    float4 mv = mv_[i];
    float4 vv = vv_[i];
    float* pp = reinterpret_cast<float*>(&pv[i]);
    float* gg = reinterpret_cast<float*>(&gv[i]);
    float* mm = reinterpret_cast<float*>(&mv);
    float* vvv = reinterpret_cast<float*>(&vv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gk = __fmaf_rn(gg[k], gs, -(pp[k] * ws));
      mm[k] = __fmaf_rn(b1, mm[k], omb1 * gk);
      vvv[k] = __fmaf_rn(b2, vvv[k], omb2 * gk * gk);
      pp[k] -= step * mm[k] / (sqrtf(vvv[k] * rbc2) + eps);
    }
    if constexpr (WTP) {
      st_pol<PMV_POL>(store_rsrc(M), M, (base + e) * 4, mv);
      st_pol<PMV_POL>(store_rsrc(V), V, (base + e) * 4, vv);
      st_pol<PMV_POL>(store_rsrc(P), P, (base + e) * 4, pv[i]);
    } else {
      st_f4<NTS>(M + base + e, mv);
      st_f4<NTS>(V + base + e, vv);
      st_f4<NTS>(P + base + e, pv[i]);
    }
  }
  // |w_new|^2, written out like the sums above.  Left as `ss2 += pp[k] * pp[k]` in the update loop, the
  // builds with written-through shadow stores multiplied and added where every build before them had
  // fused.  The form is the one read from those earlier builds' assembly, at every row width: the first
  // two squares as one fused pair, multiply-adds up to the last two, which are rounded and then added.
  {
    const float* w = reinterpret_cast<const float*>(pv);
    ss2 = __fmaf_rn(w[0], w[0], __fmul_rn(w[1], w[1]));
#pragma unroll
    for (int j = 2; j < 4 * NV - 2; ++j) ss2 = __fmaf_rn(w[j], w[j], ss2);
    ss2 = __fadd_rn(ss2, __fmul_rn(w[4 * NV - 2], w[4 * NV - 2]));
    ss2 = __fadd_rn(ss2, __fmul_rn(w[4 * NV - 1], w[4 * NV - 1]));
  }
  float sc = 1.f;
  if (norm) {
    ss2 = wave_sum(ss2);
    const float nrm = fmaxf(sqrtf(ss2), 1e-8f);
    sc = 1.f / nrm;
    if constexpr (WTA) {
      // (a 4-byte value: the relaxed agent-scope store is the compiler's `global_store_dword ... sc1`)
      if (norms && lane == 0) __hip_atomic_store(norms + row, nrm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      if (norms && lane == 0) norms[row] = nrm;
    }
  }
  if (shadow) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = (i * 64 + lane) * 4;
      ushort4 h;
      h.x = f2bf(pv[i].x * sc);
      h.y = f2bf(pv[i].y * sc);
      h.z = f2bf(pv[i].z * sc);
      h.w = f2bf(pv[i].w * sc);
      if constexpr (WTA) st_pol<ST_SC1>(store_rsrc(shadow), shadow, (base + e) * 2, h);
      else *reinterpret_cast<ushort4*>(shadow + base + e) = h;
    }
  }
}

}  // namespace scamd
