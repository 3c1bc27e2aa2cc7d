// Forced (Viterbi) CTC alignment on the device: the best single path of a transcript through a row's log-probs, and from it
// the frames every token occupies.  The trellis of ctc_loss.hip with max in place of log-sum-exp.
//   ctc_align : per row the score of the best path, the state of every frame, and per token [start, end) and the sum of its
//               log-probs.  include/vasr.h has the formula and the conventions; they are the interface.
//
// One workgroup of 256 lanes per row, lane l owning the states l, l + 256, ... -- 4 or 33 slots per lane, the mapping, the
// clamping and the id checks of ctc_loss_kernel<NS>.
//   * Forward.  A state's delta stays in a register; the delta vector is double-buffered in LDS behind two -inf entries;
//     emissions are fetched two frames ahead; one barrier per frame.  Only comparisons and float32 additions: nothing to
//     contract, no transcendental function.
//         best = x0, bp = 0;  if (x1 > best) best = x1, bp = 1;  if (x2 > best) best = x2, bp = 2;  delta = best + logp[t][e_s]
//   * Back-pointers: 2 bits per (frame, state), packed by the lane that owns the states -- no cross-lane traffic -- and stored
//     to the caller's workspace with plain vector stores, one coalesced line per frame:
//         4 slots : one byte per lane                                   -> 256 bytes per frame
//         33 slots: two 32-bit words per lane (slots 0-15, 16-31), and one word of lane 0 for slot 32, whose only state is
//                   8192, padded to 16 bytes                            -> 2064 bytes per frame
//     Frame t of row b sits at (b * frames + t) * bytes-per-frame; frame 0 has no back-pointer and its place stays unwritten
//     and unread.
//   * Back-trace: T dependent look-ups, none of them a trip to memory.  The back-pointers of a block of frames (64 or 16) are
//     loaded by all lanes, coalesced, 16 bytes per lane and load, and staged in LDS -- where the delta buffers were; lane 0
//     walks the block while the loads of the block before it are in flight in the other lanes' registers (and its own).  The
//     walker leaves s(t) of the block in LDS, from where all lanes write d_path, and the first and last frame of every token
//     in two LDS arrays.
//   * After the last barrier lanes j, j + 256, ... write start / end and sum logp[t][y_j] over their token's frames, ascending,
//     one lane per token.  No atomics.
// A state's value and back-pointer depend on its three predecessors alone: a row's outputs do not depend on the batch, on
// `frames`, on `tgt_width` or on which instantiation ran it.  Every loop is bounded by the row's clamped lengths.
// Built without packed-FP32 vectorisation and without FP64 (Makefile).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "vasr_internal.h"

namespace vasr {

namespace {

constexpr int kLanes = kCtcLossLanes;

// 32-bit words of back-pointers per frame, and frames per staged block of the back-trace
template <int NS> struct AlignShape;
template <> struct AlignShape<kCtcLossNarrowSlots> {
  static constexpr int kFrameWords = kCtcAlignNarrowFrameBytes / 4;
  static constexpr int kBlock = kCtcAlignNarrowBlock;
};
template <> struct AlignShape<kCtcLossWideSlots> {
  static constexpr int kFrameWords = kCtcAlignWideFrameBytes / 4;
  static constexpr int kBlock = kCtcAlignWideBlock;
};
static_assert(kCtcLossNarrowSlots == 4 && kCtcAlignNarrowFrameBytes == kLanes, "a byte holds a lane's four back-pointers");
static_assert(kCtcLossWideSlots == 33 && kLanes * 32 + 1 >= 2 * kCtcLossMaxWidth + 1 && kCtcAlignWideFrameBytes == 8 * kLanes + 16,
              "two words hold a lane's slots 0..31; slot 32 has the one state 8192, lane 0's");
static_assert(kCtcAlignNarrowFrameBytes % 16 == 0 && kCtcAlignWideFrameBytes % 16 == 0, "blocks are staged 16 bytes at a time");

// floats of one delta buffer for rows of tgt_width ids: 2 * tgt_width + 1 states + the two entries in front
__host__ __device__ inline int align_lds_ld(int tgt_width) { return 2 * tgt_width + 3; }

// bytes of dynamic LDS: [the two delta buffers | a staged block + its states] [first frame][last frame + 1] of every token
template <int NS>
__host__ __device__ inline int align_lds_front(int tgt_width) {
  const int fwd = 2 * align_lds_ld(tgt_width) * 4;
  const int back = (AlignShape<NS>::kBlock * AlignShape<NS>::kFrameWords + AlignShape<NS>::kBlock) * 4;
  return ((fwd > back ? fwd : back) + 15) & ~15;
}
template <int NS>
__host__ __device__ inline size_t align_lds_bytes(int tgt_width) {
  return (size_t)align_lds_front<NS>(tgt_width) + (size_t)2 * tgt_width * 4;
}

template <int NS>
__global__ __launch_bounds__(kLanes) void ctc_align_kernel(const float* __restrict__ logp, const int32_t* __restrict__ frames_in,
                                                          int64_t frames, int classes, int blank,
                                                          const int32_t* __restrict__ tgt, int tgt_width,
                                                          const int32_t* __restrict__ tgt_len, float* __restrict__ score_out,
                                                          int32_t* __restrict__ start_out, int32_t* __restrict__ end_out,
                                                          float* __restrict__ tok_out, int32_t* __restrict__ path_out,
                                                          uint32_t* __restrict__ ws) {
  static_assert(NS >= 1 && NS <= 64, "the skip flags are one bit per slot");
  constexpr int kFW = AlignShape<NS>::kFrameWords;
  constexpr int kFB = AlignShape<NS>::kBlock;
  constexpr int kStageVecs = (kFB * kFW / 4 + kLanes - 1) / kLanes;     // 16-byte loads per lane and block
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const float quiet_nan = __int_as_float(0x7fc00000);
  int32_t* start_row = start_out + b * (int64_t)tgt_width;
  int32_t* end_row = end_out + b * (int64_t)tgt_width;
  float* tok_row = tok_out ? tok_out + b * (int64_t)tgt_width : nullptr;
  int32_t* path_row = path_out ? path_out + b * frames : nullptr;

  // a row with nothing to report: the score, and every other entry unfilled
  auto unfilled = [&](float score) {
    if (tid == 0) score_out[b] = score;
    for (int j = tid; j < tgt_width; j += kLanes) {
      start_row[j] = -1;
      end_row[j] = -1;
      if (tok_row) tok_row[j] = 0.f;
    }
    if (path_row)
      for (int64_t t = tid; t < frames; t += kLanes) path_row[t] = -1;
  };

  const int fl = frames_in[b], tl = tgt_len[b];
  if (fl < 0 || tl < 0) {          // never a plausible number (uniform over the workgroup)
    unfilled(quiet_nan);
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
    unfilled(quiet_nan);
    return;
  }
  if (T == 0 || T < L) {           // no frame: 0 for the empty target, otherwise no path; fewer frames than ids: no path
    unfilled((T == 0 && L == 0) ? 0.f : -INFINITY);
    return;
  }

  const int ld = align_lds_ld(tgt_width);
  float* buf_a = reinterpret_cast<float*>(lds_raw);
  float* buf_b = buf_a + ld;       // state s of a buffer sits at [s + 2]; S + 2 <= ld
  if (tid < 2) {
    buf_a[tid] = -INFINITY;
    buf_b[tid] = -INFINITY;
  }

  const float* row = logp + b * frames * (int64_t)classes;
  uint32_t* ws_row = ws + b * frames * (int64_t)kFW;
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

  // one frame t: prev -> cur with this frame's emissions p, which are then replaced by those of frame t_next; the frame's
  // back-pointers go to the workspace.  The order is part of the interface: s, s - 1, s - 2, a later one wins only strictly.
  auto step = [&](const float* prev, float* cur, float (&p)[NS], int t, int t_next) {
    uint32_t w[(NS + 15) / 16] = {};
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int s = tid + k * kLanes;
      if (s < S) {
        const float x1 = prev[s + 1];
        const float x2 = ((skip >> k) & 1ull) ? prev[s] : -INFINITY;
        float best = a[k];
        uint32_t bp = 0u;
        if (x1 > best) { best = x1; bp = 1u; }
        if (x2 > best) { best = x2; bp = 2u; }
        a[k] = best + p[k];
        cur[s + 2] = a[k];
        w[k >> 4] |= bp << (2 * (k & 15));
      }
    }
    uint32_t* fw = ws_row + (int64_t)t * kFW;
    if constexpr (NS == kCtcLossNarrowSlots) {
      reinterpret_cast<uint8_t*>(fw)[tid] = (uint8_t)w[0];
    } else {
      fw[tid] = w[0];
      fw[kLanes + tid] = w[1];
      if (tid == 0) fw[2 * kLanes] = w[2];
    }
    fetch(t_next, p);
    __syncthreads();
  };

  int t = 1;
  for (; t + 1 < T; t += 2) {
    step(buf_a, buf_b, p1, t, t + 2);
    step(buf_b, buf_a, p0, t + 1, t + 3);
  }
  const float* fin = buf_a;
  if (t < T) {
    step(buf_a, buf_b, p1, t, T);  // (nothing left to fetch)
    fin = buf_b;
  }
  // the final state: S - 1 unless S - 2 is strictly better (S - 2 = -1 for the empty target: the -inf entry in front)
  const float last = fin[S + 1], before = fin[S];
  const bool second = before > last;
  const float score = second ? before : last;
  // every lane has read the deltas, and the workgroup's back-pointer stores are visible to it: the buffers become the stage
  __syncthreads();
  if (score == -INFINITY) {        // no path (uniform: every lane read the same two values)
    unfilled(-INFINITY);
    return;
  }

  uint32_t* stage = reinterpret_cast<uint32_t*>(lds_raw);          // [kFB][kFW]
  int32_t* states = reinterpret_cast<int32_t*>(stage + kFB * kFW);   // [kFB]: s(t) of the staged block
  int32_t* first = reinterpret_cast<int32_t*>(lds_raw + align_lds_front<NS>(tgt_width));   // [tgt_width]
  int32_t* stop = first + tgt_width;                                                       // [tgt_width]
  // (a path visits every token state, so the walk writes all of these; the zeros keep the sums below inside the row whatever
  // the walk did; the walker's first store comes behind the loop's first barrier)
  for (int j = tid; j < L; j += kLanes) first[j] = stop[j] = 0;

  // the 16-byte pieces of block q that hold frames 1 .. T - 1 (the workspace is 16-byte aligned, and so is every frame)
  uint4 held[kStageVecs];
  auto load_block = [&](int q) {
    const int64_t at = (int64_t)q * kFB;
    const int64_t lo = (q == 0 ? 1 : at) * (kFW / 4);
    const int64_t hi = (at + kFB < T ? at + kFB : (int64_t)T) * (kFW / 4);
    const uint4* src = reinterpret_cast<const uint4*>(ws_row);
#pragma unroll
    for (int i = 0; i < kStageVecs; ++i) {
      const int64_t v = at * (kFW / 4) + tid + i * kLanes;
      held[i] = (v >= lo && v < hi) ? src[v] : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto store_block = [&]() {
#pragma unroll
    for (int i = 0; i < kStageVecs; ++i) {
      const int v = tid + i * kLanes;
      if (v < kFB * (kFW / 4)) reinterpret_cast<uint4*>(stage)[v] = held[i];
    }
  };

  int s_cur = second ? S - 2 : S - 1, s_later = -1;               // lane 0's walk
  const int blocks = (T - 1) / kFB + 1;                             // T >= 1 here
  load_block(blocks - 1);
  for (int q = blocks - 1; q >= 0; --q) {
    store_block();
    __syncthreads();
    if (q > 0) load_block(q - 1);                                   // in flight during the walk
    const int t_lo = q * kFB, t_hi = T - t_lo > kFB ? t_lo + kFB : T;
    if (tid == 0) {
      for (int tt = t_hi - 1; tt >= t_lo; --tt) {
        const uint32_t* fw = stage + (tt - t_lo) * kFW;
        int bp = 0;
        if (tt > 0) {
          const int lane = s_cur & (kLanes - 1), k = s_cur / kLanes;
          if constexpr (NS == kCtcLossNarrowSlots) {
            bp = (reinterpret_cast<const uint8_t*>(fw)[lane] >> (2 * k)) & 3;
          } else {
            const uint32_t word = k < 32 ? fw[(k >> 4) * kLanes + lane] : fw[2 * kLanes];
            bp = (word >> (2 * (k & 15))) & 3;
          }
        }
        states[tt - t_lo] = s_cur;
        if (s_cur & 1) {
          const int j = s_cur >> 1;
          if (s_cur != s_later) stop[j] = tt + 1;
          if (tt == 0 || bp != 0) first[j] = tt;
        }
        s_later = s_cur;
        s_cur -= bp;
      }
    }
    __syncthreads();
    if (path_row)
      for (int i = tid; i < t_hi - t_lo; i += kLanes) path_row[t_lo + i] = states[i];
  }

  if (tid == 0) score_out[b] = score;
  if (path_row)
    for (int64_t tt = T + tid; tt < frames; tt += kLanes) path_row[tt] = -1;
  for (int j = tid; j < tgt_width; j += kLanes) {
    int t0 = -1, t1 = -1;
    float sum = 0.f;
    if (j < L) {
      t0 = first[j];
      t1 = stop[j];
      if (tok_row) {
        const float* col = row + y[j];
        sum = col[(int64_t)t0 * classes];
        for (int tt = t0 + 1; tt < t1; ++tt) sum += col[(int64_t)tt * classes];
      }
    }
    start_row[j] = t0;
    end_row[j] = t1;
    if (tok_row) tok_row[j] = sum;
  }
}

}  // namespace

size_t ctc_align_workspace_bytes(int batch, int64_t frames, int tgt_width) {
  const size_t per_frame = 2 * tgt_width + 1 <= kLanes * kCtcLossNarrowSlots ? kCtcAlignNarrowFrameBytes : kCtcAlignWideFrameBytes;
  size_t rows = 0, bytes = 0;
  if (__builtin_mul_overflow((size_t)batch, (size_t)frames, &rows) || __builtin_mul_overflow(rows, per_frame, &bytes) ||
      __builtin_add_overflow(bytes, (size_t)kCtcAlignWorkspaceAlign, &bytes))
    return SIZE_MAX;
  return bytes;
}

int launch_ctc_align(const float* logp, const int32_t* frames_in, int batch, int64_t frames, int classes, int blank,
                     const int32_t* tgt, int tgt_width, const int32_t* tgt_len, float* score, int32_t* start, int32_t* end,
                     float* tok_logp, int32_t* path, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (batch <= 0 || frames < 0 || classes < 2 || blank < 0 || blank >= classes || tgt_width < 0 || tgt_width > kCtcLossMaxWidth ||
      !workspace || workspace_bytes < ctc_align_workspace_bytes(batch, frames, tgt_width))
    return (int)hipErrorInvalidValue;
  // the first aligned address: the size asked for leaves room for it
  const uintptr_t base = (reinterpret_cast<uintptr_t>(workspace) + (kCtcAlignWorkspaceAlign - 1)) & ~(uintptr_t)(kCtcAlignWorkspaceAlign - 1);
  uint32_t* ws = reinterpret_cast<uint32_t*>(base);
  if (2 * tgt_width + 1 <= kLanes * kCtcLossNarrowSlots) {
    hipLaunchKernelGGL(ctc_align_kernel<kCtcLossNarrowSlots>, dim3(batch), dim3(kLanes), align_lds_bytes<kCtcLossNarrowSlots>(tgt_width),
                       st, logp, frames_in, frames, classes, blank, tgt, tgt_width, tgt_len, score, start, end, tok_logp, path, ws);
    return (int)hipGetLastError();
  }
  const size_t bytes = align_lds_bytes<kCtcLossWideSlots>(tgt_width);
  if (bytes > 60 * 1024) {         // (the kernel's few static bytes count towards the 64 KB a launch gets unasked)
    static std::atomic<uint64_t> lds_opted{0};   // per device (dyn_lds_opt_in); the largest carve-up is asked for once
    const hipError_t attr = dyn_lds_opt_in(reinterpret_cast<const void*>(ctc_align_kernel<kCtcLossWideSlots>),
                                           (int)align_lds_bytes<kCtcLossWideSlots>(kCtcLossMaxWidth), lds_opted);
    if (attr != hipSuccess) return (int)attr;
  }
  hipLaunchKernelGGL(ctc_align_kernel<kCtcLossWideSlots>, dim3(batch), dim3(kLanes), bytes, st, logp, frames_in, frames, classes, blank,
                     tgt, tgt_width, tgt_len, score, start, end, tok_logp, path, ws);
  return (int)hipGetLastError();
}

}  // namespace vasr
