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

  double mx = 0.0;                                    // energies are sums of squares: >= 0
  for (int64_t f = tid; f < F; f += kTrimBlock) {
    double s = 0.0;
    for (int j = 0; j < R; ++j) s += cs[f + j];
    mx = s > mx ? s : mx;
  }
  s_max[tid] = mx;
  __syncthreads();
  for (int o = kTrimBlock / 2; o >= 1; o >>= 1) {
    if (tid < o) s_max[tid] = s_max[tid + o] > s_max[tid] ? s_max[tid + o] : s_max[tid];
    __syncthreads();
  }
  const double ref = s_max[0] / fl;
  const double thr = (ref > kTrimAmin ? ref : kTrimAmin) * factor;

  int64_t first = F, last = -1;
  for (int64_t f = tid; f < F; f += kTrimBlock) {
    double s = 0.0;
    for (int j = 0; j < R; ++j) s += cs[f + j];       // the same additions as above: the same bits
    const double mse = s / fl;
    if ((mse > kTrimAmin ? mse : kTrimAmin) > thr) {
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

// grid (ceil(ld_out / 4096), min(B, 65535)), block 256
template <typename T>
__global__ __launch_bounds__(kTrimBlock) void trim_copy_kernel(const T* __restrict__ in, int64_t ld_in, int batch,
                                                                const int64_t* __restrict__ len_out,
                                                                const int64_t* __restrict__ start_ws, T* __restrict__ out,
                                                                int64_t ld_out) {
  using V = typename TrimVec<T>::type;
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * (kTrimBlock * kTrimCopyPerThread);
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    const int64_t m = len_out[b];                     // start + m <= the row's length <= ld_in <= ld_out
    const T* src = in + (int64_t)b * ld_in + start_ws[b];
    T* dst = out + (int64_t)b * ld_out;
    const bool vec = (reinterpret_cast<uintptr_t>(src) % sizeof(V)) == 0 && (reinterpret_cast<uintptr_t>(dst) % sizeof(V)) == 0;
    if (vec) {                                        // wave-uniform: one row per workgroup and trip
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
void launch_trim_silence(const T* in, int64_t ld_in, const int64_t* len, int batch, double factor, int frame_length, int hop,
                         T* out, int64_t ld_out, int64_t* len_out, int64_t* start, void* workspace, hipStream_t st) {
  const uintptr_t base = (reinterpret_cast<uintptr_t>(workspace) + kTrimWorkspaceAlign - 1) / kTrimWorkspaceAlign * kTrimWorkspaceAlign;
  int64_t* start_ws = reinterpret_cast<int64_t*>(base);
  double* chunk = reinterpret_cast<double*>(base + trim_round_up((size_t)batch * sizeof(int64_t)));
  const int64_t max_chunks = trim_max_chunks(ld_in, frame_length, hop);
  int lanes = 1;
  while (lanes < 64 && lanes * 4 < hop) lanes *= 2;
  const int per_block = kTrimBlock / lanes;
  const unsigned rows = (unsigned)(batch < 65535 ? batch : 65535);
  hipLaunchKernelGGL(trim_chunk_energy_kernel<T>, dim3((unsigned)((max_chunks + per_block - 1) / per_block), rows),
                     dim3(kTrimBlock), 0, st, in, ld_in, len, batch, frame_length, hop, lanes, max_chunks, chunk);
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

}  // namespace vasr
