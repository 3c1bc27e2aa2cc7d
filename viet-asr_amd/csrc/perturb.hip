// Audio perturbation on the device: the arithmetic of AudioAugmentor's perturbations (nemo/collections/asr/parts/perturb.py)
// on a padded batch.  include/vasr.h has the semantics (vasr_mean_square_f32, vasr_noise_plan_f64, vasr_mix_f32,
// vasr_convolve_prepare_f32, vasr_convolve_f32); no atomics, no host synchronisation, no handle.
//   mean square: ms_chunk_kernel sums the squares of every 4096-sample chunk of a row in float64 (a float32 square is exact
//     there): thread `tid` adds the samples at chunk positions 4 tid + 1024 i + {0, 1, 2, 3} in that order, the 256 threads
//     are added in a binary tree through LDS; ms_final_kernel adds a row's chunks the same way (thread tid: chunks tid,
//     tid + 256, ...; then the tree) and divides by n.  The order is fixed by the chunk grid alone, which starts at the row's
//     first sample: the bits do not depend on the batch, ld_in or the alignment (vector and scalar loads add the same terms).
//   plan: noise_plan_kernel, one thread per row, float64.
//   mix: mix_kernel, one pass, 16 elements per thread as four vectors; out = gain * x[t + shift] + scale * v[(start + t) mod N].
//   convolution: uniformly partitioned overlap-save, transform length N = 2048, partitions of Lp = 1024 taps, L = 1024 outputs
//     per workgroup.  The partitions are taken in PAIRS: a complex transform carries two real segments, z = seg(2q) +
//     i seg(2q + 1), and the prepared spectrum of pair q is that of g = h(2q) - i h(2q + 1) (times 1 / N), so that
//     Re(z * g) = seg(2q) * h(2q) + seg(2q + 1) * h(2q + 1): one forward transform per TWO partitions and no untangling of
//     the halves.  The forward transform is decimation in frequency (natural order in, bit-reversed out), the products and the
//     accumulation across pairs happen in bit-reversed order in registers (the spectra were produced by the same function, so
//     they are in that order too), the one inverse transform is decimation in time with conjugated twiddles (bit-reversed in,
//     natural out): no permutation pass.  Each pass does three radix-2 stages on eight elements in registers, 2048 = 8 * 8 *
//     8 * 4: four LDS round trips per transform.  LDS: 2112 float2 of data (one pad slot per 32) + 1024 float2 twiddles = 25 KB.
//     The prepare call copies the host-built twiddle table in front of the spectra (one hipMemcpyAsync from host memory).
#include <cmath>
#include <cstdint>
#include <vector>

#include "vasr_internal.h"

namespace vasr {

namespace {

constexpr int kPtBlock = 256;
constexpr int kMsPerThread = kMsChunk / kPtBlock;          // 16
constexpr int kMixTile = 4096;

__device__ inline int64_t pt_row_length(const int64_t* __restrict__ len, int b, int64_t ld) {
  const int64_t n = len[b];
  return n < 0 ? 0 : (n > ld ? ld : n);
}

// the sum of s[0 .. 256) in a fixed binary tree; every thread returns s[0].  Ends on a barrier; s is free again after it.
__device__ inline double pt_tree_sum(double* s, double v) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int o = kPtBlock / 2; o >= 1; o >>= 1) {
    if (tid < o) s[tid] = s[tid] + s[tid + o];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

// grid (max_chunks, min(B, 65535)), block 256; partial [B][max_chunks] f64, every entry written
__global__ __launch_bounds__(kPtBlock) void ms_chunk_kernel(const float* __restrict__ in, int64_t ld_in,
                                                             const int64_t* __restrict__ len, int batch, int64_t max_chunks,
                                                             double* __restrict__ partial) {
  __shared__ double s_sum[kPtBlock];
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * kMsChunk;
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    const int64_t n = pt_row_length(len, b, ld_in);
    const float* x = in + (int64_t)b * ld_in;
    double acc = 0.0;
    for (int i = 0; i < kMsPerThread / 4; ++i) {
      const int64_t t = t0 + (int64_t)i * (kPtBlock * 4) + tid * 4;
      if (t + 4 <= n && (reinterpret_cast<uintptr_t>(x + t) % sizeof(float4)) == 0) {
        const float4 v = *reinterpret_cast<const float4*>(x + t);
        const double a0 = v.x, a1 = v.y, a2 = v.z, a3 = v.w;
        acc += a0 * a0;
        acc += a1 * a1;
        acc += a2 * a2;
        acc += a3 * a3;
      } else {
        for (int j = 0; j < 4; ++j) {
          if (t + j < n) {
            const double a = x[t + j];
            acc += a * a;
          }
        }
      }
    }
    const double total = pt_tree_sum(s_sum, acc);
    if (tid == 0) partial[(int64_t)b * max_chunks + blockIdx.x] = total;
  }
}

// grid (B), block 256
__global__ __launch_bounds__(kPtBlock) void ms_final_kernel(const double* __restrict__ partial, int64_t max_chunks,
                                                             const int64_t* __restrict__ len, int64_t ld_in,
                                                             double* __restrict__ ms) {
  __shared__ double s_sum[kPtBlock];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t n = pt_row_length(len, b, ld_in);
  const int64_t chunks = (n + kMsChunk - 1) / kMsChunk;
  double acc = 0.0;
  for (int64_t c = tid; c < chunks; c += kPtBlock) acc += partial[(int64_t)b * max_chunks + c];
  const double total = pt_tree_sum(s_sum, acc);
  if (tid == 0) ms[b] = n > 0 ? total / (double)n : 0.0;
}

// grid (ceil(B / 256)), block 256.  NoisePerturbation.perturb in float64 and product form; no contraction: the start is the
// reference's chain of roundings
__global__ __launch_bounds__(kPtBlock) void noise_plan_kernel(const int64_t* __restrict__ len, const double* __restrict__ ms_x,
                                                               const int32_t* __restrict__ row, const double* __restrict__ snr_db,
                                                               const double* __restrict__ u, int batch,
                                                               const int64_t* __restrict__ noise_len,
                                                               const double* __restrict__ ms_v, int noise_rows, double cap,
                                                               double sample_rate, float* __restrict__ scale,
                                                               int64_t* __restrict__ start) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * kPtBlock + threadIdx.x;
  if (b >= batch) return;
  const int r = row[b];
  float sc = 0.0f;
  int64_t st = 0;
  if (r >= 0 && r < noise_rows) {
    const int64_t n = len[b] < 0 ? 0 : len[b];
    const int64_t N = noise_len[r] < 0 ? 0 : noise_len[r];
    const double mx = ms_x[b], mv = ms_v[r];
    double s;
    if (!(mx > 0.0)) {
      s = mx != mx ? mx : 0.0;                           // zero energy: nothing is added (a NaN stays one)
    } else if (mv == 0.0) {
      s = cap;
    } else {
      s = sqrt(mx / mv) * pow(10.0, -snr_db[b] / 20.0);
      s = s < cap ? s : (s != s ? s : cap);
    }
    sc = (float)s;
    if (N > n) {
      const double dur = (double)N / sample_rate - (double)n / sample_rate;
      const double t = dur * u[b];                       // random.uniform(0.0, dur): 0.0 + dur * random()
      st = (int64_t)rint(t * sample_rate);               // round(): half to even
      st = st < 0 ? 0 : (st > N - n ? N - n : st);
    }
  }
  scale[b] = sc;
  start[b] = st;
}

struct MixArgs {
  const float* in;
  int64_t ld_in;
  const int64_t* len;
  int batch;
  const float* gain;
  const int64_t* shift;
  const float* add;
  int64_t ld_add;
  int add_rows;
  const int64_t* add_len;
  const int32_t* add_row;
  const float* scale;
  const int64_t* start;
  float* out;
  int64_t ld_out;
};

// grid (ceil(ld_out / 4096), min(B, 65535)), block 256
__global__ __launch_bounds__(kPtBlock) void mix_kernel(const MixArgs a) {
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * kMixTile;
  for (int b = blockIdx.y; b < a.batch; b += gridDim.y) {
    const int64_t n = pt_row_length(a.len, b, a.ld_in);
    const float* x = a.in + (int64_t)b * a.ld_in;
    float* o = a.out + (int64_t)b * a.ld_out;
    const float g = a.gain ? a.gain[b] : 1.0f;
    int64_t sh = a.shift ? a.shift[b] : 0;
    if (sh > n || sh < -n) sh = 0;
    float sc = 0.0f;
    const float* v = nullptr;
    int64_t N = 0, st = 0;
    if (a.add) {
      const int r = a.add_row[b];
      sc = a.scale[b];
      if (r >= 0 && r < a.add_rows && sc != 0.0f) {
        N = pt_row_length(a.add_len, r, a.ld_add);
        v = a.add + (int64_t)r * a.ld_add;
        st = a.start ? a.start[b] : 0;
      }
      if (N > 0) {
        st %= N;
        st = st < 0 ? st + N : st;
      } else {
        sc = 0.0f;                                       // no addend: it is never read
      }
    }
    const bool wrap = st + n > N;
    for (int k = 0; k < kMixTile / (kPtBlock * 4); ++k) {
      const int64_t t = t0 + ((int64_t)k * kPtBlock + tid) * 4;
      if (t >= a.ld_out) continue;
      float xv[4], y[4];
      const int64_t xs = t + sh;
      if (t + 4 <= n && xs >= 0 && xs + 4 <= n && (reinterpret_cast<uintptr_t>(x + xs) % sizeof(float4)) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(x + xs);
        xv[0] = q.x, xv[1] = q.y, xv[2] = q.z, xv[3] = q.w;
      } else {
        for (int j = 0; j < 4; ++j) xv[j] = (t + j < n && xs + j >= 0 && xs + j < n) ? x[xs + j] : 0.0f;
      }
      for (int j = 0; j < 4; ++j) y[j] = g == 1.0f ? xv[j] : ((t + j < n && xs + j >= 0 && xs + j < n) ? g * xv[j] : 0.0f);
      if (sc != 0.0f) {
        float vv[4];
        if (!wrap && t + 4 <= n && (reinterpret_cast<uintptr_t>(v + st + t) % sizeof(float4)) == 0) {
          const float4 q = *reinterpret_cast<const float4*>(v + st + t);
          vv[0] = q.x, vv[1] = q.y, vv[2] = q.z, vv[3] = q.w;
        } else {
          for (int j = 0; j < 4; ++j) vv[j] = t + j < n ? v[wrap ? (st + t + j) % N : st + t + j] : 0.0f;
        }
        for (int j = 0; j < 4; ++j) y[j] = t + j < n ? fmaf(sc, vv[j], y[j]) : 0.0f;
      }
      if (t + 4 <= a.ld_out && (reinterpret_cast<uintptr_t>(o + t) % sizeof(float4)) == 0) {
        float4 q;
        q.x = y[0], q.y = y[1], q.z = y[2], q.w = y[3];
        *reinterpret_cast<float4*>(o + t) = q;
      } else {
        for (int j = 0; j < 4 && t + j < a.ld_out; ++j) o[t + j] = y[j];
      }
    }
  }
}

// ---- the transform ----
// The twiddle factors W[k] = exp(-2 pi i k / N), k < N / 2, are built on the host in float64, rounded once to float32 (the way
// audio.sinc_table is built) and copied to the head of the spectra buffer by the prepare call: spectra[0 .. N / 2) is the table,
// the partition spectra follow.

constexpr int kConvLds = kConvN + kConvN / 32;             // one pad slot per 32 elements
__device__ inline int conv_slot(int i) { return i + (i >> 5); }

__device__ inline float2 cmul(float2 a, float2 b) {
  return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}

// K radix-2 stages on the 2^K elements base + j * stride of group g, in registers.  Forward (decimation in frequency): spans
// stride << (K - 1) down to stride, (a, b) -> (a + b, (a - b) w); inverse (decimation in time): spans stride up to stride <<
// (K - 1), (a, b) -> (a + conj(w) b, a - conj(w) b), the exact inverse of the forward stage up to the factor 2.  w = W^(position
// inside the span * N / (2 span)).  stride is a power of two.
template <int K, bool INV>
__device__ inline void fft_pass(float2* __restrict__ s, const float2* __restrict__ tw, int stride, int g) {
  constexpr int M = 1 << K;
  const int lo = g & (stride - 1), hi = g / stride;
  const int base = hi * (stride << K) + lo;
  float2 v[M];
#pragma unroll
  for (int j = 0; j < M; ++j) v[j] = s[conv_slot(base + j * stride)];
#pragma unroll
  for (int t = 0; t < K; ++t) {
    const int sj = INV ? (1 << t) : (1 << (K - 1 - t));
    const int span = sj * stride;
    const int tstep = (kConvN / 2) / span;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      if (j & sj) continue;
      float2 w = tw[(lo + (j & (sj - 1)) * stride) * tstep];
      const float2 p = v[j], q = v[j + sj];
      if (!INV) {
        v[j] = make_float2(p.x + q.x, p.y + q.y);
        v[j + sj] = cmul(make_float2(p.x - q.x, p.y - q.y), w);
      } else {
        w.y = -w.y;
        const float2 r = cmul(q, w);
        v[j] = make_float2(p.x + r.x, p.y + r.y);
        v[j + sj] = make_float2(p.x - r.x, p.y - r.y);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < M; ++j) s[conv_slot(base + j * stride)] = v[j];
}

// both begin behind the caller's barrier and end on one
__device__ inline void conv_fft_forward(float2* s, const float2* tw) {
  const int tid = threadIdx.x;
  fft_pass<3, false>(s, tw, 256, tid);
  __syncthreads();
  fft_pass<3, false>(s, tw, 32, tid);
  __syncthreads();
  fft_pass<3, false>(s, tw, 4, tid);
  __syncthreads();
  fft_pass<2, false>(s, tw, 1, tid);
  fft_pass<2, false>(s, tw, 1, tid + kPtBlock);
  __syncthreads();
}

__device__ inline void conv_fft_inverse(float2* s, const float2* tw) {
  const int tid = threadIdx.x;
  fft_pass<2, true>(s, tw, 1, tid);
  fft_pass<2, true>(s, tw, 1, tid + kPtBlock);
  __syncthreads();
  fft_pass<3, true>(s, tw, 4, tid);
  __syncthreads();
  fft_pass<3, true>(s, tw, 32, tid);
  __syncthreads();
  fft_pass<3, true>(s, tw, 256, tid);
  __syncthreads();
}

__device__ inline void conv_load_twiddles(float2* s_tw, const float2* __restrict__ table) {
  for (int i = threadIdx.x; i < kConvN / 2; i += kPtBlock) s_tw[i] = table[i];
}

// grid (pairs, R), block 256; spectra: the twiddle table, then [R][pairs][N] float2, every entry written
__global__ __launch_bounds__(kPtBlock) void convolve_prepare_kernel(const float* __restrict__ ir, int64_t ld_ir,
                                                                     const int64_t* __restrict__ ir_len, int pairs,
                                                                     float2* __restrict__ spectra) {
  __shared__ float2 s_data[kConvLds];
  __shared__ float2 s_tw[kConvN / 2];
  const int tid = threadIdx.x, q = blockIdx.x, r = blockIdx.y;
  conv_load_twiddles(s_tw, spectra);
  int64_t m = pt_row_length(ir_len, r, ld_ir);
  m = m < 1 ? 1 : m;
  const float* h = ir + (int64_t)r * ld_ir;
  const int64_t k0 = (int64_t)2 * q * kConvTaps, k1 = k0 + kConvTaps;
  constexpr float inv_n = 1.0f / (float)kConvN;            // a power of two: exact
  for (int i = tid; i < kConvN; i += kPtBlock) {
    const float a = (i < kConvTaps && k0 + i < m) ? h[k0 + i] : 0.0f;
    const float c = (i < kConvTaps && k1 + i < m) ? h[k1 + i] : 0.0f;
    s_data[conv_slot(i)] = make_float2(a * inv_n, -(c * inv_n));
  }
  __syncthreads();
  conv_fft_forward(s_data, s_tw);
  float2* out = spectra + kConvN / 2 + ((int64_t)r * pairs + q) * kConvN;
  for (int i = tid; i < kConvN; i += kPtBlock) out[i] = s_data[conv_slot(i)];
}

// grid (ceil(ld_out / L), min(B, 65535)), block 256
__global__ __launch_bounds__(kPtBlock) void convolve_kernel(const float* __restrict__ in, int64_t ld_in,
                                                             const int64_t* __restrict__ len, int batch,
                                                             const int32_t* __restrict__ ir_row,
                                                             const int64_t* __restrict__ ir_len,
                                                             const float2* __restrict__ spectra, int R, int64_t ld_ir, int pairs,
                                                             float* __restrict__ out, int64_t ld_out,
                                                             int64_t* __restrict__ len_out) {
  __shared__ float2 s_data[kConvLds];
  __shared__ float2 s_tw[kConvN / 2];
  constexpr int kPer = kConvN / kPtBlock;                  // 8 spectrum bins per thread
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * kConvOut;
  conv_load_twiddles(s_tw, spectra);
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    const int64_t n = pt_row_length(len, b, ld_in);
    const float* x = in + (int64_t)b * ld_in;
    float* o = out + (int64_t)b * ld_out;
    const int r = ir_row[b];
    const bool copy = r < 0 || r >= R;
    int64_t m = 1;
    if (!copy) {
      m = pt_row_length(ir_len, r, ld_ir);
      m = m < 1 ? 1 : m;
    }
    const int64_t lo = n == 0 ? 0 : n + m - 1;             // <= ld_in + ld_ir - 1 <= ld_out
    if (blockIdx.x == 0 && tid == 0) len_out[b] = lo;
    if (copy || t0 >= lo) {                                // workgroup-uniform
      for (int k = 0; k < kConvOut / kPtBlock; ++k) {
        const int64_t t = t0 + k * kPtBlock + tid;
        if (t < ld_out) o[t] = (copy && t < n) ? x[t] : 0.0f;
      }
      continue;
    }
    const int row_pairs = (int)(((m + kConvTaps - 1) / kConvTaps + 1) / 2);
    float2 acc[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) acc[k] = make_float2(0.0f, 0.0f);
    for (int q = 0; q < row_pairs; ++q) {
      // segment of partition p: x[t0 - p Lp - (Lp - 1) + i], i < N; the circular product's positions Lp - 1 .. Lp - 1 + L - 1
      // are the block's outputs
      const int64_t s0 = t0 - (int64_t)2 * q * kConvTaps - (kConvTaps - 1), s1 = s0 - kConvTaps;
      if (s0 + kConvN <= 0) break;                         // this pair and every later one lie in front of the row
      if (s1 >= n) continue;                               // both segments lie behind it
      __syncthreads();                                     // the pair before has been read
      for (int i = tid; i < kConvN; i += kPtBlock) {
        const int64_t i0 = s0 + i, i1 = s1 + i;
        const float a = (i0 >= 0 && i0 < n) ? x[i0] : 0.0f;
        const float c = (i1 >= 0 && i1 < n) ? x[i1] : 0.0f;
        s_data[conv_slot(i)] = make_float2(a, c);
      }
      __syncthreads();
      conv_fft_forward(s_data, s_tw);
      const float2* G = spectra + kConvN / 2 + ((int64_t)r * pairs + q) * kConvN;
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        const int i = k * kPtBlock + tid;
        const float2 z = s_data[conv_slot(i)], gq = G[i];
        acc[k].x = fmaf(z.x, gq.x, fmaf(-z.y, gq.y, acc[k].x));
        acc[k].y = fmaf(z.x, gq.y, fmaf(z.y, gq.x, acc[k].y));
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) s_data[conv_slot(k * kPtBlock + tid)] = acc[k];
    __syncthreads();
    conv_fft_inverse(s_data, s_tw);
    for (int k = 0; k < kConvOut / kPtBlock; ++k) {
      const int i = k * kPtBlock + tid;
      const int64_t t = t0 + i;
      if (t < ld_out) o[t] = t < lo ? s_data[conv_slot(kConvTaps - 1 + i)].x : 0.0f;
    }
    __syncthreads();                                       // the next row stages into s_data
  }
}

constexpr size_t kPtAlign = 256;

}  // namespace

size_t mean_square_workspace_bytes(int batch, int64_t ld_in) {
  const unsigned __int128 chunks = (unsigned __int128)batch * (unsigned __int128)((ld_in + kMsChunk - 1) / kMsChunk);
  const unsigned __int128 total = chunks * sizeof(double) + kPtAlign;
  return total > (unsigned __int128)SIZE_MAX ? SIZE_MAX : (size_t)total;
}

void launch_mean_square(const float* in, int64_t ld_in, const int64_t* len, int batch, double* ms, void* workspace,
                        hipStream_t st) {
  double* partial = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(workspace) + kPtAlign - 1) / kPtAlign * kPtAlign);
  const int64_t max_chunks = (ld_in + kMsChunk - 1) / kMsChunk;
  const unsigned rows = (unsigned)(batch < 65535 ? batch : 65535);
  if (max_chunks > 0)
    hipLaunchKernelGGL(ms_chunk_kernel, dim3((unsigned)max_chunks, rows), dim3(kPtBlock), 0, st, in, ld_in, len, batch, max_chunks,
                       partial);
  hipLaunchKernelGGL(ms_final_kernel, dim3((unsigned)batch), dim3(kPtBlock), 0, st, partial, max_chunks, len, ld_in, ms);
}

void launch_noise_plan(const int64_t* len, const double* ms_x, const int32_t* row, const double* snr_db, const double* u,
                       int batch, const int64_t* noise_len, const double* ms_v, int noise_rows, double cap, int sample_rate,
                       float* scale, int64_t* start, hipStream_t st) {
  hipLaunchKernelGGL(noise_plan_kernel, dim3((unsigned)((batch + kPtBlock - 1) / kPtBlock)), dim3(kPtBlock), 0, st, len, ms_x, row,
                     snr_db, u, batch, noise_len, ms_v, noise_rows, cap, (double)sample_rate, scale, start);
}

void launch_mix(const float* in, int64_t ld_in, const int64_t* len, int batch, const float* gain, const int64_t* shift,
                const float* add, int64_t ld_add, int add_rows, const int64_t* add_len, const int32_t* add_row,
                const float* scale, const int64_t* start, float* out, int64_t ld_out, hipStream_t st) {
  if (ld_out <= 0) return;
  const MixArgs a{in, ld_in, len, batch, gain, shift, add, ld_add, add_rows, add_len, add_row, scale, start, out, ld_out};
  const unsigned rows = (unsigned)(batch < 65535 ? batch : 65535);
  hipLaunchKernelGGL(mix_kernel, dim3((unsigned)((ld_out + kMixTile - 1) / kMixTile), rows), dim3(kPtBlock), 0, st, a);
}

int convolve_pairs(int64_t ld_ir) { return (int)(((ld_ir + kConvTaps - 1) / kConvTaps + 1) / 2); }

size_t convolve_spectra_bytes(int R, int64_t ld_ir) {
  return ((size_t)R * (size_t)convolve_pairs(ld_ir) * kConvN + kConvN / 2) * sizeof(float2);
}

static std::vector<float> convolve_twiddles() {
  std::vector<float> t(kConvN);
  const double step = -2.0 * 3.14159265358979323846 / kConvN;
  for (int k = 0; k < kConvN / 2; ++k) {
    t[2 * k] = (float)std::cos(step * k);
    t[2 * k + 1] = (float)std::sin(step * k);
  }
  return t;
}

int launch_convolve_prepare(const float* ir, int64_t ld_ir, const int64_t* ir_len, int R, void* spectra, hipStream_t st) {
  static const std::vector<float> table = convolve_twiddles();      // lives as long as the library: the copy may be deferred
  const hipError_t e = hipMemcpyAsync(spectra, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  const int pairs = convolve_pairs(ld_ir);
  hipLaunchKernelGGL(convolve_prepare_kernel, dim3((unsigned)pairs, (unsigned)R), dim3(kPtBlock), 0, st, ir, ld_ir, ir_len, pairs,
                     reinterpret_cast<float2*>(spectra));
  return 0;
}

void launch_convolve(const float* in, int64_t ld_in, const int64_t* len, int batch, const int32_t* ir_row, const int64_t* ir_len,
                     const void* spectra, int R, int64_t ld_ir, float* out, int64_t ld_out, int64_t* len_out, hipStream_t st) {
  const unsigned rows = (unsigned)(batch < 65535 ? batch : 65535);
  hipLaunchKernelGGL(convolve_kernel, dim3((unsigned)((ld_out + kConvOut - 1) / kConvOut), rows), dim3(kPtBlock), 0, st, in, ld_in,
                     len, batch, ir_row, ir_len, reinterpret_cast<const float2*>(spectra), R, ld_ir, convolve_pairs(ld_ir), out,
                     ld_out, len_out);
}

}  // namespace vasr
