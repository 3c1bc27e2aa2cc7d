// Scoring of classification logits on the device: what the reference's evaluation of a speech classifier computes per row.
//   class_scores : metrics.classification_accuracy (nemo/collections/asr/metrics.py:66-99: logits.topk + a comparison), the
//                  nn.CrossEntropyLoss(reduction='none') behind CrossEntropyLossNM / EvalLoss (helpers.py:215-288), and the
//                  top-k classes with their logits and softmax probabilities.
//
// One wavefront per row, four rows per workgroup -- the access pattern of classify.hip's pool / linear kernels: lane l takes
// c = l, l + 64, ... of the row's C classes, then a butterfly.  No LDS, no threshold on C.
//   * ONE total order on a row's classes, as a 64-bit key that is larger for the class that comes first: the upper half orders
//     the values (NaN above every number, -0 == +0), the lower half puts the LOWER class index first among equal values.  Keys
//     of one row are distinct, so "the next class" is always well defined.
//   * rank[b]: the number of classes whose key exceeds the target's -- top-k correctness for every k at once.
//   * top-k: k selection passes, each the maximum key below the previous pick's.
//   * loss[b] = (m + logf(sum_c expf(x_c - m))) - x_target with m the row maximum; prob = expf(x - logsumexp).  The sum runs
//     in eight accumulators per lane (class c goes to accumulator (c / 64) % 8 of lane c % 64), merged pairwise, then the
//     butterfly: at most (ceil(C / 512) - 1) + 3 + 6 roundings on any path, no more than ceil(log2 C) for C <= 1536.
// Every reduction has one fixed order that depends on C alone, so a row's bits do not depend on the batch it is in.  No atomics.
// Built without packed-FP32 vectorisation and without FP64 (Makefile): the kernel runs next to the MFMA
// GEMMs of other streams.
#include <math.h>
#include <stdint.h>

#include "vasr_internal.h"

namespace vasr {

namespace {

constexpr unsigned long long kNoPick = ~0ull;   // above every key: a key's lower half is at most 0xfffffffe

// larger = earlier in the order.  Value part: NaN -> all ones; otherwise the usual monotone map of IEEE bits with -0 folded
// onto +0.  Index part: 0xfffffffe - c, so the lower index wins among equal values.
__device__ __forceinline__ unsigned long long order_key(float x, int c) {
  uint32_t u;
  if (x != x) {
    u = 0xffffffffu;
  } else {
    const uint32_t bits = x == 0.f ? 0u : __float_as_uint(x);
    u = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  }
  return ((unsigned long long)u << 32) | (unsigned long long)(0xfffffffeu - (uint32_t)c);
}

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_sum_int(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// grid ((batch + 3) / 4): four rows per workgroup, a wavefront each.  All branches below are uniform over the wavefront.
__global__ __launch_bounds__(256) void class_scores_kernel(const float* __restrict__ logits, int batch, int classes,
                                                           const int64_t* __restrict__ targets, int k,
                                                           int32_t* __restrict__ topk_idx, float* __restrict__ topk_val,
                                                           float* __restrict__ topk_prob, int32_t* __restrict__ rank,
                                                           float* __restrict__ loss) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= batch) return;
  const float* x = logits + b * classes;

  int t = -1;                      // the target, or -1: none given / outside [0, C)
  if (targets) {
    const int64_t tt = targets[b];
    if (tt >= 0 && tt < classes) t = (int)tt;
  }

  float lse = 0.f;
  if ((loss && t >= 0) || (topk_prob && k > 0)) {
    float m = -INFINITY;
    for (int c = lane; c < classes; c += 64) m = fmaxf(m, x[c]);
    m = wave_max(m);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f;
    for (int c = lane; c < classes; c += 512) {
      a0 += expf(x[c] - m);
      if (c + 64 < classes) a1 += expf(x[c + 64] - m);
      if (c + 128 < classes) a2 += expf(x[c + 128] - m);
      if (c + 192 < classes) a3 += expf(x[c + 192] - m);
      if (c + 256 < classes) a4 += expf(x[c + 256] - m);
      if (c + 320 < classes) a5 += expf(x[c + 320] - m);
      if (c + 384 < classes) a6 += expf(x[c + 384] - m);
      if (c + 448 < classes) a7 += expf(x[c + 448] - m);
    }
    const float s = wave_sum(((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)));
    lse = m + logf(s);
  }

  if (targets) {
    if (t < 0) {
      if (lane == 0) {
        if (rank) rank[b] = -1;
        if (loss) loss[b] = 0.f;
      }
    } else {
      const float xt = x[t];
      if (rank) {
        const unsigned long long kt = order_key(xt, t);
        int before = 0;
        for (int c = lane; c < classes; c += 64) before += order_key(x[c], c) > kt ? 1 : 0;
        before = wave_sum_int(before);
        if (lane == 0) rank[b] = before;
      }
      if (loss && lane == 0) loss[b] = lse - xt;
    }
  }

  unsigned long long prev = kNoPick;
  for (int j = 0; j < k; ++j) {
    unsigned long long best = 0ull;          // below every key: a key's lower half is at least 0xfffffffe - 65535
    for (int c = lane; c < classes; c += 64) {
      const unsigned long long kc = order_key(x[c], c);
      if (kc < prev && kc > best) best = kc;
    }
    best = wave_max_key(best);
    if (best == 0ull) break;                 // (k <= C and distinct keys: a class is always left)
    prev = best;
    if (lane == 0) {
      const int c = (int)(0xfffffffeu - (uint32_t)(best & 0xffffffffull));
      const float v = x[c];
      const int64_t o = b * k + j;
      if (topk_idx) topk_idx[o] = c;
      if (topk_val) topk_val[o] = v;
      if (topk_prob) topk_prob[o] = expf(v - lse);
    }
  }
}

}  // namespace

int launch_class_scores(const float* logits, int batch, int classes, const int64_t* targets, int k, int32_t* topk_idx,
                        float* topk_val, float* topk_prob, int32_t* rank, float* loss, hipStream_t st) {
  if (batch <= 0 || classes <= 0 || classes > kClassScoresMaxClasses || k < 0 || k > kClassScoresMaxK || k > classes)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(class_scores_kernel, dim3((unsigned)(((int64_t)batch + 3) / 4)), dim3(256), 0, st, logits, batch, classes,
                     targets, k, topk_idx, topk_val, topk_prob, rank, loss);
  return (int)hipGetLastError();
}

}  // namespace vasr
