// Device-side helpers shared by the gfx950 kernels (included from .hip files only).
#pragma once
#include <hip/hip_runtime.h>

namespace vasr {

// native vectors: a v4f is one ds_read_b128 / global dwordx4, f32x16 the accumulator of a 32x32 MFMA, f16x8 its 16-bit operand
using f32x16 = __attribute__((ext_vector_type(16))) float;
using v4f = __attribute__((ext_vector_type(4))) float;
using v2f = __attribute__((ext_vector_type(2))) float;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;

// orders a wavefront's own LDS writes and reads for the compiler (the LDS pipeline itself keeps them in issue order)
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// XCD-aware remap of a 1-D grid: workgroup i runs on XCD i % 8 (each with a private L2), so consecutive LOGICAL ids --
// neighbours in (m-block, time-tile) order, which share activations or a window's halo -- are dealt to one XCD
__device__ __forceinline__ int xcd_remap(int bid, int n_blocks) {
  const int q = n_blocks / 8, r = n_blocks % 8, xcd = bid % 8, slot = bid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

// Wave-wide unsigned maximum, uniform result: butterfly inside each 16-lane row on DPP (VALU only -- a ds_bpermute
// chain is six dependent LDS round trips at the tail of every wavefront), then the four row maxima through SGPRs.
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#define VASR_DPP(x, ctrl) ((unsigned)__builtin_amdgcn_update_dpp(0, (int)(x), (ctrl), 0xF, 0xF, false))
  v = max(v, VASR_DPP(v, 0xB1));    // quad_perm [1,0,3,2]
  v = max(v, VASR_DPP(v, 0x4E));    // quad_perm [2,3,0,1]
  v = max(v, VASR_DPP(v, 0x141));   // row_half_mirror
  v = max(v, VASR_DPP(v, 0x140));   // row_mirror: every lane of a row now holds the row's maximum
#undef VASR_DPP
  const unsigned a = __builtin_amdgcn_readlane((int)v, 0), b = __builtin_amdgcn_readlane((int)v, 16);
  const unsigned c = __builtin_amdgcn_readlane((int)v, 32), d = __builtin_amdgcn_readlane((int)v, 48);
  return max(max(a, b), max(c, d));
}

// ---- the encoder's activation (vasr_set_activation; codes kAct* in vasr_internal.h) ----
// jasper_activations (nemo/collections/asr/parts/jasper.py:21-25): nn.ReLU, nn.Hardtanh() = clamp(x, -1, 1) and nn.SELU.
// SELU's negative side is lambda * alpha * expm1(x): exp(x) - 1 loses every significant bit near 0 (relative error up to 1
// there; torch's CPU SELU is within 1.2e-7 of float64), so the accurate expm1f, never __expf(x) - 1.
constexpr float kSeluLambda = 1.0507009873554804934193349852946f;
constexpr float kSeluAlpha = 1.6732632423543772848170429916717f;
__device__ __forceinline__ float selu(float v) {
  return v > 0.f ? kSeluLambda * v : (kSeluLambda * kSeluAlpha) * expm1f(v);
}
// act: 0 ReLU, 1 Hardtanh, 2 SELU (uniform across the launch)
__device__ __forceinline__ float activate(float v, int act) {
  if (act == 2) return selu(v);
  if (act == 1) return fminf(fmaxf(v, -1.f), 1.f);
  return v > 0.f ? v : 0.f;
}

// ---- the GEMM epilogues' residual + activation (encoder_pw*.hip, encoder_fused.hip), after the BN affine ----
// EPI = epilogue_kind (vasr_internal.h): 0 = residual added, ReLU or nothing (relu flag); 1 = a clamp to uniform bounds --
// Hardtanh [-1, 1], ReLU [0, inf), nothing (relu flag clear); 2 = SELU; under 1 and 2 the residual is added or (res_max)
// combined by max, a uniform select.  Built once per kernel; RES = the launch has a residual tensor.  The throughput and
// latency GEMMs give the same bits because both call this.
template <int EPI>
struct Epilogue {
  bool relu, res_max;
  float lo, hi;   // kind 1: the clamp; kind 0: lo = the ReLU floor of the float4 form (0, or -inf for nothing)
  __device__ __forceinline__ Epilogue(int relu_flag, int act, int res_max_flag) : relu(relu_flag & 1), res_max(res_max_flag) {
    lo = relu ? (EPI == 1 && act == 1 ? -1.f : 0.f) : -__builtin_inff();
    hi = (relu && act == 1) ? 1.f : __builtin_inff();
  }
  // one element (edge tiles, the fp32 GEMM); r is dereferenced only under RES
  template <bool RES>
  __device__ __forceinline__ float apply(float v, const float* __restrict__ r) const {
    if constexpr (EPI != 0) {
      if constexpr (RES) v = res_max ? fmaxf(v, *r) : v + *r;
      return EPI == 1 ? fminf(fmaxf(v, lo), hi) : selu(v);
    } else {
      if constexpr (RES) v += *r;
      return relu ? fmaxf(v, 0.f) : v;   // (relu flag clear: a NaN stays a NaN)
    }
  }
  // a float4 row piece (interior tiles): straight-line, ReLU as a maximum with the uniform floor.  NOT the scalar form's
  // arithmetic when the relu flag is clear: max(NaN, -inf) is -inf.  The two are kept apart, each as it always was.
  template <bool RES = false>
  __device__ __forceinline__ v4f apply4(v4f v, const v4f& r = v4f{}) const {
    if constexpr (EPI != 0) {
      if constexpr (RES) v = res_max ? __builtin_elementwise_max(v, r) : v + r;
      if constexpr (EPI == 1) return __builtin_elementwise_min(__builtin_elementwise_max(v, v4f{lo, lo, lo, lo}), v4f{hi, hi, hi, hi});
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = selu(v[e]);
      return v;
    } else {
      if constexpr (RES) v += r;
      return __builtin_elementwise_max(v, v4f{lo, lo, lo, lo});
    }
  }
};

__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// largest |y| over an utterance's VALID output frames (t < ylen; ylen = 0 without a table), as fp32 bits: a lane's share
// of what amax_publish() stores for the split of the next kF16x2 consumer of y
struct AmaxTracker {
  int ylen;
  unsigned ymax = 0;
  __device__ __forceinline__ void track(float v, int t) {
    const unsigned u = abs_bits(v);
    ymax = (t < ylen && u > ymax) ? u : ymax;
  }
  __device__ __forceinline__ void track4(v4f v, int t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) track(v[e], t + e);
  }
};

// ---- per-utterance maxima (AmaxTab, vasr_internal.h) ----
// Producer side: every wavefront of the producing launch owns ONE slot per utterance it touches and stores its maximum
// there with a plain store (slot < n, n set by the launcher).  Round 2 first used one atomicMax per wavefront into 8
// words per utterance: 32 768 device-scope atomics per depthwise launch land in a handful of cache lines of one memory
// channel and retire at ~1 per ns -- +30 us on a 25 us kernel.  Plain stores to distinct words cost nothing measurable.
__device__ __forceinline__ void amax_publish(unsigned* tab, int stride, int b, int slot, unsigned lane_max, int lane) {
  const unsigned m = wave_max_u32(lane_max);
  if (lane == 0) tab[(int64_t)b * stride + slot] = m;
}
// Consumer side: a wavefront reduces the n slots of utterance b itself (n * 4 bytes from L2, coalesced; no barrier).
__device__ __forceinline__ unsigned amax_read(const unsigned* __restrict__ tab, int stride, int n, int b, int lane) {
  const unsigned* p = tab + (int64_t)b * stride;
  unsigned m = 0;
  for (int i = lane; i < n; i += 64) m = max(m, p[i]);
  return wave_max_u32(m);
}

// The same reduction in two halves, eight slots per lane in flight: amax_request() issues the loads of the first 512
// slots (one per channel of a depthwise layer) and returns; the caller requests whatever else it needs next (a GEMM
// workgroup: its first rows and weight fragments) and calls amax_collect() when it needs the value -- s_waitcnt counts in
// order, so waiting for these OLDER loads leaves the younger ones in flight.  The serial form was four to eight dependent
// round trips to L2 (2-3 us) at the head of every GEMM workgroup, before its first row was even requested.  (Clamped, not
// predicated: a slot read twice does not change a maximum, and the loads stay unconditional.)
__device__ __forceinline__ void amax_request(const unsigned* __restrict__ tab, int stride, int n, int b, int lane,
                                             unsigned (&v)[8]) {
  const unsigned* p = tab + (int64_t)b * stride;
  const int last = max(n, 1) - 1;   // (a table always has a slot 0; n <= 0 does not occur for a published table)
#pragma unroll
  for (int u = 0; u < 8; ++u) v[u] = p[min(64 * u + lane, last)];
}
__device__ __forceinline__ unsigned amax_collect(const unsigned* __restrict__ tab, int stride, int n, int b, int lane,
                                                 const unsigned (&v)[8]) {
  unsigned m = 0;
#pragma unroll
  for (int u = 0; u < 8; ++u) m = max(m, v[u]);
  if (n > 512) {   // several time tiles per channel (long recordings): the rest in further trips
    const unsigned* p = tab + (int64_t)b * stride;
    for (int i0 = 512; i0 < n; i0 += 512) {
      unsigned w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) w[u] = p[min(i0 + 64 * u + lane, n - 1)];
#pragma unroll
      for (int u = 0; u < 8; ++u) m = max(m, w[u]);
    }
  }
  return wave_max_u32(m);
}

// power-of-two scale (and its inverse) that puts a maximum of magnitude `amax_bits` (fp32 bit pattern of |x|) into
// [2^14, 2^15): the fp16 planes then have 18 octaves of full 22-bit precision below the maximum
__device__ __forceinline__ void f16_scale(unsigned amax_bits, float* scale, float* inv) {
  int e = (int)(amax_bits >> 23);
  e = e < 16 ? 16 : (e > 254 ? 254 : e);
  *scale = __uint_as_float((unsigned)(268 - e) << 23);   // 2^(141 - e)
  *inv = __uint_as_float((unsigned)(e - 14) << 23);      // 2^(e - 141)
}

}  // namespace vasr
