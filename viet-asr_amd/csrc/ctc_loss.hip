// The CTC forward score on the device: what the reference's evaluation reports as Evaluation_Loss for the ASR path.
//   ctc_loss : nn.CTCLoss(blank, reduction='none', zero_infinity=False) per row, as CTCLossNM builds it
//              (nemo/collections/asr/losses.py), forward only: -log P(target | log-probs), i.e. minus the forced score of a
//              transcript.  No alignment, no gradient.
//
// One workgroup of 256 lanes per row; the T-step recursion is the serial chain, rows run side by side.
//   * The extended sequence e has S = 2 L + 1 states (blank, y1, blank, ..., yL, blank).  Lane l owns the states
//     s = l, l + 256, l + 512, ... ("slots"): 4 slots per lane while 2 * tgt_width + 1 <= 1024, 33 slots (8448 states, enough
//     for tgt_width 4096) above.  The two instantiations run the same per-state code.
//   * A state's own alpha stays in a register; the alpha vector is double-buffered in LDS (S + 2 floats each: two -inf entries
//     in front stand for the states -1 and -2, so the reads of s - 1 and s - 2 need no branch) only so that a lane can read its
//     neighbours' values.  One barrier per frame.
//   * A state's emission index e_s and whether it may take alpha(s - 2) are fixed for the row and kept in registers; each lane
//     loads its own logp[t + 2][e_s] two frames ahead, so a step does not wait on memory and num_classes has no limit.
//   * The formula, per state and frame t >= 1 (include/vasr.h):
//         x0 = alpha(t-1, s), x1 = alpha(t-1, s-1), x2 = alpha(t-1, s-2) where e_s != blank and e_s != e_(s-2), else absent
//         m = the largest of them; lse = m == -inf ? -inf : m + logf((expf(x0 - m) + expf(x1 - m)) + expf(x2 - m))
//         alpha(t, s) = lse + logp[t][e_s]
//     an absent term is -inf: expf(-inf) adds an exact zero, so the two-term and the three-term sums have the same bits.
//     alpha(0, 0) = logp[0][blank], alpha(0, 1) = logp[0][y1], -inf elsewhere;
//     loss = -lse(alpha(T-1, S-1), alpha(T-1, S-2)).  Nothing is reduced across states but those last two.
// A state's value depends on its three predecessors alone, so a row's bits do not depend on the batch, on `frames`, on
// `tgt_width` or on which instantiation ran it.  Every loop is bounded by the row's clamped lengths; no atomics, no workspace.
// Built without packed-FP32 vectorisation and without FP64 (Makefile): the kernel runs next to the MFMA
// GEMMs of other streams.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "vasr_internal.h"

namespace vasr {

namespace {

constexpr int kLanes = kCtcLossLanes;

// the order is part of the interface: s, s - 1, s - 2
__device__ __forceinline__ float lse3(float x0, float x1, float x2) {
  float m = x0;
  if (x1 > m) m = x1;
  if (x2 > m) m = x2;
  if (m == -INFINITY) return -INFINITY;
  return m + logf((expf(x0 - m) + expf(x1 - m)) + expf(x2 - m));
}

// floats of LDS for rows of tgt_width ids: two buffers of (2 * tgt_width + 1) states + the two entries in front
__host__ __device__ inline int ctc_lds_ld(int tgt_width) { return 2 * tgt_width + 3; }

template <int NS>
__global__ __launch_bounds__(kLanes) void ctc_loss_kernel(const float* __restrict__ logp, const int32_t* __restrict__ frames_in,
                                                         int64_t frames, int classes, int blank,
                                                         const int32_t* __restrict__ tgt, int tgt_width,
                                                         const int32_t* __restrict__ tgt_len, float* __restrict__ loss) {
  static_assert(NS >= 1 && NS <= 64, "the skip flags are one bit per slot");
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const float quiet_nan = __int_as_float(0x7fc00000);
  const int fl = frames_in[b], tl = tgt_len[b];
  if (fl < 0 || tl < 0) {          // never a plausible number (uniform over the workgroup)
    if (tid == 0) loss[b] = quiet_nan;
    return;
  }
  const int T = (int64_t)fl < frames ? fl : (int)frames;
  const int L = tl < tgt_width ? tl : tgt_width;
  const int S = 2 * L + 1;
  const int32_t* y = tgt + b * (int64_t)tgt_width;

  // emission index and skip flag of every owned state; the ids inside the row's length are checked on the way
  int e[NS];
  unsigned long long skip = 0ull;
  int bad = 0;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = tid + k * kLanes;
    e[k] = blank;
    if (s < S && (s & 1)) {
      const int id = y[(s - 1) >> 1];
      if (id < 0 || id >= classes || id == blank) {
        bad = 1;
      } else {
        e[k] = id;
        if (s >= 3 && y[(s - 3) >> 1] != id) skip |= 1ull << k;
      }
    }
  }
  bad = __syncthreads_or(bad);
  if (bad) {
    if (tid == 0) loss[b] = quiet_nan;
    return;
  }
  if (T == 0 || T < L) {           // no frame: 0 for the empty target, otherwise no path; fewer frames than ids: no path
    if (tid == 0) loss[b] = (T == 0 && L == 0) ? 0.f : INFINITY;
    return;
  }

  const int ld = ctc_lds_ld(tgt_width);
  float* buf_a = reinterpret_cast<float*>(lds_raw);
  float* buf_b = buf_a + ld;       // state s of a buffer sits at [s + 2]; S + 2 <= ld
  if (tid < 2) {
    buf_a[tid] = -INFINITY;
    buf_b[tid] = -INFINITY;
  }

  const float* row = logp + b * frames * (int64_t)classes;
  // p[k] = logp[t][e_s] of the owned states, for a frame t < T
  auto fetch = [&](int t, float (&p)[NS]) {
    if (t < T) {
      const float* fr = row + (int64_t)t * classes;
#pragma unroll
      for (int k = 0; k < NS; ++k)
        if (tid + k * kLanes < S) p[k] = fr[e[k]];
    }
  };

  float a[NS], p0[NS], p1[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) a[k] = p0[k] = p1[k] = -INFINITY;
  fetch(0, p0);
  fetch(1, p1);
#pragma unroll
  for (int k = 0; k < NS; ++k) {   // frame 0
    const int s = tid + k * kLanes;
    if (s < S) {
      a[k] = s < 2 ? p0[k] : -INFINITY;
      buf_a[s + 2] = a[k];
    }
  }
  fetch(2, p0);
  __syncthreads();

  // one frame: prev -> cur with this frame's emissions p, which are then replaced by those of frame t_next
  auto step = [&](const float* prev, float* cur, float (&p)[NS], int t_next) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int s = tid + k * kLanes;
      if (s < S) {
        const float x1 = prev[s + 1];
        const float x2 = ((skip >> k) & 1ull) ? prev[s] : -INFINITY;
        a[k] = lse3(a[k], x1, x2) + p[k];
        cur[s + 2] = a[k];
      }
    }
    fetch(t_next, p);
    __syncthreads();
  };

  int t = 1;
  for (; t + 1 < T; t += 2) {
    step(buf_a, buf_b, p1, t + 2);
    step(buf_b, buf_a, p0, t + 3);
  }
  const float* fin = buf_a;
  if (t < T) {
    step(buf_a, buf_b, p1, T);     // (nothing left to fetch)
    fin = buf_b;
  }
  // S - 2 = -1 for the empty target: the -inf entry in front
  if (tid == 0) loss[b] = -lse3(fin[S + 1], fin[S], -INFINITY);
}

}  // namespace

int launch_ctc_loss(const float* logp, const int32_t* frames_in, int batch, int64_t frames, int classes, int blank,
                    const int32_t* tgt, int tgt_width, const int32_t* tgt_len, float* loss, hipStream_t st) {
  if (batch <= 0 || frames < 0 || classes < 2 || blank < 0 || blank >= classes || tgt_width < 0 || tgt_width > kCtcLossMaxWidth)
    return (int)hipErrorInvalidValue;
  const size_t bytes = (size_t)2 * ctc_lds_ld(tgt_width) * sizeof(float);
  if (2 * tgt_width + 1 <= kLanes * kCtcLossNarrowSlots) {
    hipLaunchKernelGGL(ctc_loss_kernel<kCtcLossNarrowSlots>, dim3(batch), dim3(kLanes), bytes, st, logp, frames_in, frames, classes,
                       blank, tgt, tgt_width, tgt_len, loss);
    return (int)hipGetLastError();
  }
  static_assert(kLanes * kCtcLossWideSlots >= 2 * kCtcLossMaxWidth + 1, "the wide kernel holds every state of the widest row");
  if (bytes > 60 * 1024) {         // (the kernel's few static bytes count towards the 64 KB a launch gets unasked)
    static std::atomic<uint64_t> lds_opted{0};   // per device (dyn_lds_opt_in); the largest carve-up is asked for once
    const hipError_t attr = dyn_lds_opt_in(reinterpret_cast<const void*>(ctc_loss_kernel<kCtcLossWideSlots>),
                                           (int)((size_t)2 * ctc_lds_ld(kCtcLossMaxWidth) * sizeof(float)), lds_opted);
    if (attr != hipSuccess) return (int)attr;
  }
  hipLaunchKernelGGL(ctc_loss_kernel<kCtcLossWideSlots>, dim3(batch), dim3(kLanes), bytes, st, logp, frames_in, frames, classes,
                     blank, tgt, tgt_width, tgt_len, loss);
  return (int)hipGetLastError();
}

}  // namespace vasr
