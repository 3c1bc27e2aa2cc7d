// Leading / trailing silence trim on the device: AudioSegment(trim=True) -> librosa.effects.trim(samples, top_db)
// (nemo/collections/asr/parts/segment.py:19-32; librosa < 0.10, third-party arithmetic restated from its published form,
// parity unpinned).  include/vasr.h (vasr_trim_silence_f32) has the semantics; three launches, no atomics, no host sync:
//   1. trim_chunk_energy_kernel: the sum of squares of every hop-sized chunk of the reflect-padded row.  Frame f is the
//      chunks f .. f + frame_length / hop - 1, so each sample is read once.  A chunk belongs to a group of `lanes` lanes of
//      one wavefront (a power of two, 4 samples per lane and trip); lane `sub` of the group adds the samples at chunk positions
//      4 sub + 4 lanes i + {0, 1, 2, 3} in that order, then the group adds its lanes in a butterfly.  The samples go in as
//      16-byte (float) / 8-byte (int16) vectors where the four are inside the row and the address is aligned, one by one
//      through the mirror otherwise -- the SAME additions in the SAME order either way, in float64, where a float32 square
//      is exact: a chunk's sum does not depend on the row's alignment, on `ld_in` or on the batch.
//   2. trim_bounds_kernel: one workgroup per row.  Frame energies from the chunk sums (ascending chunk order), the row's
//      maximum, then the first and last frame with max(amin, mse) > max(amin, ref) * 10^(-top_db / 10).
//   3. trim_copy_kernel: out[b][t] = in[b][start + t] for t < len_out, zero up to ld_out; vectors where both addresses allow.
//
// Split at silences (vasr_split_silence_f32): librosa.effects.split on the same flags, plus two rules of an ASR front end --
// pauses shorter than m frames are bridged, runs longer than M frames are cut at their quietest frame.  Two launches:
//   1. trim_chunk_energy_kernel, the launch above: the same additions in the same order.
//   2. split_kernel: one workgroup per row.  The row's threshold as trim_bounds_kernel forms it; then tiles of 256 frames in
//      ascending order: a wavefront ballot of the flags gives every frame its last non-silent predecessor and every opening
//      frame (non-silent, none of the m frames before it is) its ordinal, the wavefronts' totals go through LDS and the
//      carry over the tiles is workgroup-uniform.  A run's end is one behind the predecessor of the NEXT opening frame
//      (the last run ends behind the row's last non-silent frame), so one ascending pass finds both edges; the runs go to
//      the workspace.  Then tiles of 256 runs: a run of at most M frames is one segment; longer ones are cut one after the
//      other by the whole workgroup (arg-min of the frame sums over s + ceil(M / 2) .. s + M, lowest index among equals:
//      a wavefront butterfly, then four candidates through LDS), and a run's output index is its ordinal plus the pieces
//      the cuts in front of it have added, which every lane picks up as the workgroup-uniform loop passes its own run.
// Gather (vasr_gather_segments_f32): the trim's shifted copy with a (row, start, length) descriptor per output row.
#include <cstdint>

#include "vasr_internal.h"

namespace vasr {

namespace {

constexpr int kTrimBlock = 256;
constexpr int kTrimCopyPerThread = 16;     // elements per thread of the copy: a tile is 4096 elements
constexpr double kTrimAmin = 1e-10;        // librosa.power_to_db's amin

__device__ inline double trim_value(float v) { return (double)v; }
__device__ inline double trim_value(short v) { return (double)v * (1.0 / 32768.0); }   // segment.py:61-74, exact

template <typename T> struct TrimVec;
template <> struct TrimVec<float> { using type = float4; };
template <> struct TrimVec<short> { using type = short4; };

// numpy's `reflect`: periodic mirroring with period 2 (n - 1), no repeated edge sample; n >= 1, any i
__device__ inline int64_t trim_mirror(int64_t i, int64_t n) {
  if (n == 1) return 0;
  const int64_t period = 2 * (n - 1);
  int64_t m = i % period;
  if (m < 0) m += period;
  return m < n ? m : period - m;
}

__device__ inline int64_t trim_row_length(const int64_t* __restrict__ len, int b, int64_t ld_in) {
  const int64_t n = len[b];
  return n < 0 ? 0 : (n > ld_in ? ld_in : n);
}

// the float64 sum of frame f: its chunks in ascending order -- the ONE form every decision here uses
__device__ inline double trim_frame_sum(const double* __restrict__ cs, int64_t f, int R) {
  double s = 0.0;
  for (int j = 0; j < R; ++j) s += cs[f + j];
  return s;
}

// max(amin, ref) * factor of a row of F frames, ref the loudest frame's mse; s_max: kTrimBlock doubles of LDS.  Ends on a barrier.
__device__ inline double trim_row_threshold(const double* __restrict__ cs, int64_t F, int R, double fl, double factor,
                                            double* s_max) {
  const int tid = threadIdx.x;
  double mx = 0.0;                                    // energies are sums of squares: >= 0
  for (int64_t f = tid; f < F; f += kTrimBlock) {
    const double s = trim_frame_sum(cs, f, R);
    mx = s > mx ? s : mx;
  }
  s_max[tid] = mx;
  __syncthreads();
  for (int o = kTrimBlock / 2; o >= 1; o >>= 1) {
    if (tid < o) s_max[tid] = s_max[tid + o] > s_max[tid] ? s_max[tid + o] : s_max[tid];
    __syncthreads();
  }
  const double ref = s_max[0] / fl;
  return (ref > kTrimAmin ? ref : kTrimAmin) * factor;
}

__device__ inline bool trim_non_silent(double frame_sum, double fl, double thr) {
  const double mse = frame_sum / fl;
  return (mse > kTrimAmin ? mse : kTrimAmin) > thr;
}

// grid (ceil(max_chunks / (256 / lanes)), min(B, 65535)), block 256; chunk [B][max_chunks] f64
template <typename T>
__global__ __launch_bounds__(kTrimBlock) void trim_chunk_energy_kernel(const T* __restrict__ in, int64_t ld_in,
                                                                        const int64_t* __restrict__ len, int batch,
                                                                        int frame_length, int hop, int lanes, int64_t max_chunks,
                                                                        double* __restrict__ chunk) {
  using V = typename TrimVec<T>::type;
  const int tid = threadIdx.x;
  const int sub = tid % lanes;
  const int64_t c = (int64_t)blockIdx.x * (kTrimBlock / lanes) + tid / lanes;
  const int pad = frame_length / 2, R = frame_length / hop;
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    const int64_t n = trim_row_length(len, b, ld_in);
    const int64_t nchunks = n / hop + R;              // frames + R - 1
    double acc = 0.0;
    if (c < nchunks && n > 0) {
      const T* x = in + (int64_t)b * ld_in;
      const int64_t i0 = c * hop - pad;               // row index of the chunk's first sample, before mirroring
      for (int pos = sub * 4; pos < hop; pos += lanes * 4) {
        const int64_t i = i0 + pos;
        if (pos + 4 <= hop && i >= 0 && i + 4 <= n && (reinterpret_cast<uintptr_t>(x + i) % sizeof(V)) == 0) {
          const V v = *reinterpret_cast<const V*>(x + i);
          const double a0 = trim_value(v.x), a1 = trim_value(v.y), a2 = trim_value(v.z), a3 = trim_value(v.w);
          acc += a0 * a0;
          acc += a1 * a1;
          acc += a2 * a2;
          acc += a3 * a3;
        } else {
          for (int j = 0; j < 4 && pos + j < hop; ++j) {
            const double a = trim_value(x[trim_mirror(i + j, n)]);
            acc += a * a;
          }
        }
      }
    }
    for (int o = lanes >> 1; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if (sub == 0 && c < nchunks) chunk[(int64_t)b * max_chunks + c] = acc;
  }
}

// grid (B), block 256
__global__ __launch_bounds__(kTrimBlock) void trim_bounds_kernel(const double* __restrict__ chunk, int64_t max_chunks,
                                                                  const int64_t* __restrict__ len, int64_t ld_in,
                                                                  int frame_length, int hop, double factor,
                                                                  int64_t* __restrict__ len_out, int64_t* __restrict__ start_out,
                                                                  int64_t* __restrict__ start_ws) {
  __shared__ double s_max[kTrimBlock];
  __shared__ int64_t s_first[kTrimBlock], s_last[kTrimBlock];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int R = frame_length / hop;
  const int64_t n = trim_row_length(len, b, ld_in);
  const int64_t F = 1 + n / hop;
  const double* cs = chunk + (int64_t)b * max_chunks;
  const double fl = (double)frame_length;

  const double thr = trim_row_threshold(cs, F, R, fl, factor, s_max);

  int64_t first = F, last = -1;
  for (int64_t f = tid; f < F; f += kTrimBlock) {
    if (trim_non_silent(trim_frame_sum(cs, f, R), fl, thr)) {      // the same additions as above: the same bits
      first = f < first ? f : first;
      last = f;
    }
  }
  s_first[tid] = first;
  s_last[tid] = last;
  __syncthreads();
  for (int o = kTrimBlock / 2; o >= 1; o >>= 1) {
    if (tid < o) {
      s_first[tid] = s_first[tid + o] < s_first[tid] ? s_first[tid + o] : s_first[tid];
      s_last[tid] = s_last[tid + o] > s_last[tid] ? s_last[tid + o] : s_last[tid];
    }
    __syncthreads();
  }
  if (tid == 0) {
    int64_t start = 0, end = 0;
    if (s_last[0] >= 0) {
      start = s_first[0] * hop;
      end = (s_last[0] + 1) * hop;
      end = end > n ? n : end;
    }
    len_out[b] = end - start;
    start_ws[b] = start;
    if (start_out) start_out[b] = start;
  }
}

// one workgroup's tile [t0, t0 + 4096) of one output row: dst[t] = src[t] for t < m, zero up to ld_out.  src[0 .. m) is readable
template <typename T>
__device__ inline void trim_copy_tile(const T* __restrict__ src, T* __restrict__ dst, int64_t m, int64_t ld_out, int64_t t0) {
  using V = typename TrimVec<T>::type;
  const int tid = threadIdx.x;
  const bool vec = (reinterpret_cast<uintptr_t>(src) % sizeof(V)) == 0 && (reinterpret_cast<uintptr_t>(dst) % sizeof(V)) == 0;
  if (vec) {                                          // wave-uniform: one row per workgroup and trip
    for (int k = 0; k < kTrimCopyPerThread / 4; ++k) {
      const int64_t t = t0 + ((int64_t)k * kTrimBlock + tid) * 4;
      if (t + 4 <= m) {
        *reinterpret_cast<V*>(dst + t) = *reinterpret_cast<const V*>(src + t);
      } else if (t + 4 <= ld_out && t >= m) {
        V z;
        z.x = z.y = z.z = z.w = T(0);
        *reinterpret_cast<V*>(dst + t) = z;
      } else {
        for (int j = 0; j < 4 && t + j < ld_out; ++j) dst[t + j] = t + j < m ? src[t + j] : T(0);
      }
    }
  } else {
    for (int k = 0; k < kTrimCopyPerThread; ++k) {
      const int64_t t = t0 + (int64_t)k * kTrimBlock + tid;
      if (t < ld_out) dst[t] = t < m ? src[t] : T(0);
    }
  }
}

// grid (ceil(ld_out / 4096), min(B, 65535)), block 256
template <typename T>
__global__ __launch_bounds__(kTrimBlock) void trim_copy_kernel(const T* __restrict__ in, int64_t ld_in, int batch,
                                                                const int64_t* __restrict__ len_out,
                                                                const int64_t* __restrict__ start_ws, T* __restrict__ out,
                                                                int64_t ld_out) {
  const int64_t t0 = (int64_t)blockIdx.x * (kTrimBlock * kTrimCopyPerThread);
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    const int64_t m = len_out[b];                     // start + m <= the row's length <= ld_in <= ld_out
    trim_copy_tile<T>(in + (int64_t)b * ld_in + start_ws[b], out + (int64_t)b * ld_out, m, ld_out, t0);
  }
}

// grid (ceil(ld_out / 4096), min(S, 65535)), block 256.  A descriptor that does not lie inside its row, or is longer than
// ld_out, gives a row of zeros: nothing is read for it.
template <typename T>
__global__ __launch_bounds__(kTrimBlock) void gather_segments_kernel(const T* __restrict__ in, int64_t ld_in, int batch,
                                                                      const int32_t* __restrict__ row,
                                                                      const int64_t* __restrict__ start,
                                                                      const int64_t* __restrict__ len, int64_t segments,
                                                                      T* __restrict__ out, int64_t ld_out) {
  const int64_t t0 = (int64_t)blockIdx.x * (kTrimBlock * kTrimCopyPerThread);
  for (int64_t s = blockIdx.y; s < segments; s += gridDim.y) {
    int64_t r = row[s], st = start[s], m = len[s];
    const bool ok = r >= 0 && r < batch && st >= 0 && m >= 0 && m <= ld_in && st <= ld_in - m && m <= ld_out;
    if (!ok) r = st = m = 0;
    trim_copy_tile<T>(in + r * ld_in + st, out + s * ld_out, m, ld_out, t0);
  }
}

constexpr int kSplitWaves = kTrimBlock / 64;

// grid (B), block 256; runs [B][max_runs][2] i64 (frames), bounds [B][max_segments][2] i64 (samples), count [B]
__global__ __launch_bounds__(kTrimBlock) void split_kernel(const double* __restrict__ chunk, int64_t max_chunks,
                                                            const int64_t* __restrict__ len, int64_t ld_in, int frame_length,
                                                            int hop, double factor, int min_silence, int max_frames,
                                                            int64_t* runs, int64_t max_runs, int64_t* __restrict__ bounds,
                                                            int64_t max_segments, int64_t* __restrict__ count) {
  __shared__ double s_max[kTrimBlock];
  __shared__ int64_t s_wave_last[2][kSplitWaves];     // per tile parity: a wavefront's last non-silent frame, or -1
  __shared__ int s_wave_open[2][kSplitWaves];         // and the runs it opens
  __shared__ double s_cut_sum[2][kSplitWaves];        // per cut parity: a wavefront's arg-min candidate
  __shared__ int64_t s_cut_at[2][kSplitWaves];
  __shared__ int64_t s_run[kTrimBlock][2];            // a tile of runs
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid % 64, wave = tid / 64;
  const int R = frame_length / hop;
  const int64_t n = trim_row_length(len, b, ld_in);
  const int64_t F = n > 0 ? 1 + n / hop : 0;          // a row without samples has no segment
  const double* cs = chunk + (int64_t)b * max_chunks;
  const double fl = (double)frame_length;
  int64_t* rr = runs + (int64_t)b * max_runs * 2;
  int64_t* bb = bounds + (int64_t)b * max_segments * 2;

  const double thr = trim_row_threshold(cs, F, R, fl, factor, s_max);

  // runs: ascending tiles of frames; last_ns and n_runs are workgroup-uniform
  int64_t last_ns = -1, n_runs = 0;
  int parity = 0;
  for (int64_t f0 = 0; f0 < F; f0 += kTrimBlock, parity ^= 1) {
    const int64_t f = f0 + tid;
    const bool flag = f < F && trim_non_silent(trim_frame_sum(cs, f, R), fl, thr);
    const unsigned long long mask = __ballot(flag);
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    if (lane == 0) s_wave_last[parity][wave] = mask ? f0 + wave * 64 + (63 - __clzll((long long)mask)) : -1;
    __syncthreads();
    int64_t prev = below ? f0 + wave * 64 + (63 - __clzll((long long)below)) : -1;   // the last non-silent frame in front of f
    for (int w = wave - 1; w >= 0 && prev < 0; --w) prev = s_wave_last[parity][w];
    if (prev < 0) prev = last_ns;
    const bool opens = flag && (prev < 0 || f - prev > min_silence);
    const unsigned long long omask = __ballot(opens);
    if (lane == 0) s_wave_open[parity][wave] = __popcll(omask);
    __syncthreads();
    int64_t k = n_runs + __popcll(omask & ((1ull << lane) - 1ull));
    for (int w = 0; w < kSplitWaves; ++w) {
      const int o = s_wave_open[parity][w];
      if (w < wave) k += o;
      n_runs += o;
    }
    if (opens) {                                      // k < max_runs: two runs are at least two frames apart
      rr[2 * k] = f;
      if (k > 0) rr[2 * k - 1] = prev + 1;            // the run in front of this one ends behind its last non-silent frame
    }
    for (int w = kSplitWaves - 1; w >= 0; --w) {
      const int64_t l = s_wave_last[parity][w];
      if (l >= 0) {
        last_ns = l;
        break;
      }
    }
  }
  if (tid == 0 && n_runs > 0) rr[2 * n_runs - 1] = last_ns + 1;
  __syncthreads();                                    // the runs are in memory for the whole workgroup

  // segments: ascending tiles of runs; `total` is workgroup-uniform
  const int64_t M = max_frames;
  int64_t total = 0;
  int cut_parity = 0;
  for (int64_t k0 = 0; k0 < n_runs; k0 += kTrimBlock) {
    const int64_t k = k0 + tid;
    int64_t s = 0, e = 0;
    if (k < n_runs) {
      s = rr[2 * k];
      e = rr[2 * k + 1];
    }
    const bool is_long = M > 0 && e - s > M;
    int64_t at = total + tid;                         // this run's last segment, if no run of the tile up to it is cut
    const int tile = (int)(n_runs - k0 < kTrimBlock ? n_runs - k0 : kTrimBlock);
    if (__syncthreads_or(is_long)) {                  // also keeps s_run of the tile before from being overwritten early
      s_run[tid][0] = s;
      s_run[tid][1] = is_long ? e : s;                // a run that is not cut: skipped below
      __syncthreads();
      int64_t added = 0;
      for (int t = 0; t < tile; ++t) {
        int64_t cs0 = s_run[t][0];
        const int64_t ce = s_run[t][1];
        while (ce - cs0 > M) {                        // workgroup-uniform
          double best = 0.0;
          int64_t best_at = -1;
          for (int64_t f = cs0 + (M + 1) / 2 + tid; f <= cs0 + M; f += kTrimBlock) {     // f < ce <= F
            const double v = trim_frame_sum(cs, f, R);
            if (best_at < 0 || v < best) {            // ascending f: the lowest index among equals stays
              best = v;
              best_at = f;
            }
          }
          for (int o = 32; o >= 1; o >>= 1) {
            const double v = __shfl_xor(best, o);
            const long long a = __shfl_xor((long long)best_at, o);
            if (a >= 0 && (best_at < 0 || v < best || (v == best && a < best_at))) {
              best = v;
              best_at = a;
            }
          }
          if (lane == 0) {
            s_cut_sum[cut_parity][wave] = best;
            s_cut_at[cut_parity][wave] = best_at;
          }
          __syncthreads();
          best_at = -1;
          for (int w = 0; w < kSplitWaves; ++w) {
            const double v = s_cut_sum[cut_parity][w];
            const int64_t a = s_cut_at[cut_parity][w];
            if (a >= 0 && (best_at < 0 || v < best || (v == best && a < best_at))) {
              best = v;
              best_at = a;
            }
          }
          cut_parity ^= 1;
          const int64_t o = total + t + added;
          if (tid == 0 && o < max_segments) {
            const int64_t x0 = cs0 * hop, x1 = best_at * hop;
            bb[2 * o] = x0 < n ? x0 : n;
            bb[2 * o + 1] = x1 < n ? x1 : n;
          }
          cs0 = best_at;
          ++added;
        }
        if (t == tid) {                               // what is left of this lane's run is its last segment, behind every
          s = cs0;                                    // piece cut off so far
          at += added;
        }
      }
      total += added;
    }
    if (k < n_runs && at < max_segments) {
      const int64_t x0 = s * hop, x1 = e * hop;
      bb[2 * at] = x0 < n ? x0 : n;
      bb[2 * at + 1] = x1 < n ? x1 : n;
    }
    total += tile;
  }
  if (tid == 0) count[b] = total;
}

int64_t trim_max_chunks(int64_t ld_in, int frame_length, int hop) { return ld_in / hop + frame_length / hop; }

constexpr size_t kTrimWorkspaceAlign = 256;
size_t trim_round_up(size_t v) { return (v + kTrimWorkspaceAlign - 1) / kTrimWorkspaceAlign * kTrimWorkspaceAlign; }

}  // namespace

size_t trim_workspace_bytes(int batch, int64_t ld_in, int frame_length, int hop) {
  const unsigned __int128 chunks = (unsigned __int128)batch * (unsigned __int128)trim_max_chunks(ld_in, frame_length, hop);
  const unsigned __int128 total = chunks * sizeof(double) + trim_round_up((size_t)batch * sizeof(int64_t)) + kTrimWorkspaceAlign;
  return total > (unsigned __int128)SIZE_MAX ? SIZE_MAX : (size_t)total;
}

template <typename T>
static void launch_trim_chunk_energy(const T* in, int64_t ld_in, const int64_t* len, int batch, int frame_length, int hop,
                                     double* chunk, hipStream_t st) {
  const int64_t max_chunks = trim_max_chunks(ld_in, frame_length, hop);
  int lanes = 1;
  while (lanes < 64 && lanes * 4 < hop) lanes *= 2;
  const int per_block = kTrimBlock / lanes;
  const unsigned rows = (unsigned)(batch < 65535 ? batch : 65535);
  hipLaunchKernelGGL(trim_chunk_energy_kernel<T>, dim3((unsigned)((max_chunks + per_block - 1) / per_block), rows),
                     dim3(kTrimBlock), 0, st, in, ld_in, len, batch, frame_length, hop, lanes, max_chunks, chunk);
}

template <typename T>
void launch_trim_silence(const T* in, int64_t ld_in, const int64_t* len, int batch, double factor, int frame_length, int hop,
                         T* out, int64_t ld_out, int64_t* len_out, int64_t* start, void* workspace, hipStream_t st) {
  const uintptr_t base = (reinterpret_cast<uintptr_t>(workspace) + kTrimWorkspaceAlign - 1) / kTrimWorkspaceAlign * kTrimWorkspaceAlign;
  int64_t* start_ws = reinterpret_cast<int64_t*>(base);
  double* chunk = reinterpret_cast<double*>(base + trim_round_up((size_t)batch * sizeof(int64_t)));
  const int64_t max_chunks = trim_max_chunks(ld_in, frame_length, hop);
  const unsigned rows = (unsigned)(batch < 65535 ? batch : 65535);
  launch_trim_chunk_energy<T>(in, ld_in, len, batch, frame_length, hop, chunk, st);
  hipLaunchKernelGGL(trim_bounds_kernel, dim3((unsigned)batch), dim3(kTrimBlock), 0, st, chunk, max_chunks, len, ld_in,
                     frame_length, hop, factor, len_out, start, start_ws);
  if (ld_out > 0) {
    const int tile = kTrimBlock * kTrimCopyPerThread;
    hipLaunchKernelGGL(trim_copy_kernel<T>, dim3((unsigned)((ld_out + tile - 1) / tile), rows), dim3(kTrimBlock), 0, st, in,
                       ld_in, batch, len_out, start_ws, out, ld_out);
  }
}

template void launch_trim_silence<float>(const float*, int64_t, const int64_t*, int, double, int, int, float*, int64_t, int64_t*,
                                         int64_t*, void*, hipStream_t);
template void launch_trim_silence<short>(const short*, int64_t, const int64_t*, int, double, int, int, short*, int64_t, int64_t*,
                                         int64_t*, void*, hipStream_t);

// a row of F frames has at most ceil(F / 2) runs: two opening frames are at least two frames apart
static int64_t split_max_runs(int64_t ld_in, int hop) { return (ld_in / hop + 1) / 2 + 1; }

size_t split_workspace_bytes(int batch, int64_t ld_in, int frame_length, int hop) {
  const unsigned __int128 chunks = (unsigned __int128)batch * (unsigned __int128)trim_max_chunks(ld_in, frame_length, hop);
  const unsigned __int128 runs = (unsigned __int128)batch * (unsigned __int128)split_max_runs(ld_in, hop) * 2 * sizeof(int64_t);
  const unsigned __int128 total = chunks * sizeof(double) + runs + 2 * kTrimWorkspaceAlign;
  return total > (unsigned __int128)SIZE_MAX ? SIZE_MAX : (size_t)total;
}

template <typename T>
void launch_split_silence(const T* in, int64_t ld_in, const int64_t* len, int batch, double factor, int frame_length, int hop,
                          int min_silence, int max_frames, int64_t* bounds, int64_t max_segments, int64_t* count,
                          void* workspace, hipStream_t st) {
  const uintptr_t base = (reinterpret_cast<uintptr_t>(workspace) + kTrimWorkspaceAlign - 1) / kTrimWorkspaceAlign * kTrimWorkspaceAlign;
  const int64_t max_runs = split_max_runs(ld_in, hop);
  int64_t* runs = reinterpret_cast<int64_t*>(base);
  double* chunk = reinterpret_cast<double*>(base + trim_round_up((size_t)batch * (size_t)max_runs * 2 * sizeof(int64_t)));
  launch_trim_chunk_energy<T>(in, ld_in, len, batch, frame_length, hop, chunk, st);
  hipLaunchKernelGGL(split_kernel, dim3((unsigned)batch), dim3(kTrimBlock), 0, st, chunk, trim_max_chunks(ld_in, frame_length, hop),
                     len, ld_in, frame_length, hop, factor, min_silence, max_frames, runs, max_runs, bounds, max_segments, count);
}

template void launch_split_silence<float>(const float*, int64_t, const int64_t*, int, double, int, int, int, int, int64_t*, int64_t,
                                          int64_t*, void*, hipStream_t);
template void launch_split_silence<short>(const short*, int64_t, const int64_t*, int, double, int, int, int, int, int64_t*, int64_t,
                                          int64_t*, void*, hipStream_t);

template <typename T>
void launch_gather_segments(const T* in, int64_t ld_in, int batch, const int32_t* row, const int64_t* start, const int64_t* len,
                            int64_t segments, T* out, int64_t ld_out, hipStream_t st) {
  const int tile = kTrimBlock * kTrimCopyPerThread;
  const unsigned rows = (unsigned)(segments < 65535 ? segments : 65535);
  hipLaunchKernelGGL(gather_segments_kernel<T>, dim3((unsigned)((ld_out + tile - 1) / tile), rows), dim3(kTrimBlock), 0, st, in,
                     ld_in, batch, row, start, len, segments, out, ld_out);
}

template void launch_gather_segments<float>(const float*, int64_t, int, const int32_t*, const int64_t*, const int64_t*, int64_t,
                                            float*, int64_t, hipStream_t);
template void launch_gather_segments<short>(const short*, int64_t, int, const int32_t*, const int64_t*, const int64_t*, int64_t,
                                            short*, int64_t, hipStream_t);

}  // namespace vasr
