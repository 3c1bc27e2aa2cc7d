// The speech-classification path for gfx950: CropOrPadSpectrogramAugmentation (reference
// nemo/collections/asr/audio_preprocessing.py:666-738) and JasperDecoderForClassification (jasper.py:257-319).
//
//   * crop_pad_kernel: out[b][f][t] = in[b][f][t + off[b]] when the row is wider than audio_length, else the row between
//                      left = (audio_length - T) / 2 zero frames and the rest on the right (the odd frame goes right); a plain copy,
//                      so every value is bit-equal to the one it was cut from.  It writes every column of the stored range: the
//                      fused path hands it the encoder's padded-pitch input buffer and gets zeros behind audio_length.
//   * pool_kernel:     one wavefront per (utterance, channel) row, the access pattern of encoder_se.hip's row sums: lane l takes
//                      t = l, l + 64, ... of the row's `frames` columns in turn, then a butterfly -- mean (the sum divided by
//                      frames) or maximum over EXACTLY those columns, never the pitch padding behind them.
//   * linear_kernel:   one wavefront per (utterance, class): logits[k] = bias[k] + sum_c W[k][c] * pooled[c], lane l walking
//                      c = l, l + 64, ... with fmaf, then the butterfly.
//   * softmax_kernel:  one workgroup per utterance, in place: max, exp(x - max), sum, divide (F.softmax(dim=-1)).
// Every reduction has one fixed order that depends on the row's shape alone, so a row's bits do not depend on the batch it is in.
// No atomics.  Built without packed-FP32 vectorisation and without FP64 (Makefile): these kernels run next
// to the MFMA GEMMs of other streams.
#include <math.h>

#include "vasr_internal.h"
#include "vasr_device.h"

namespace vasr {

namespace {

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// grid (column tiles of 256, feat, batch).  Row b is `frames` wide, or (wav_len: row-independent mode) as wide as an unbatched
// call on wav_len[b] samples makes it, 1 + wav_len[b] / hop, capped at frames.  The offset is clamped into the row, so no read
// leaves [0, width) whatever the caller's array holds.
__global__ __launch_bounds__(256) void crop_pad_kernel(const float* __restrict__ in, int64_t ld_in, int feat, int frames,
                                                       const int64_t* __restrict__ wav_len, int hop, int audio_length,
                                                       const int64_t* __restrict__ off, float* __restrict__ out,
                                                       int64_t ld_out, int store_cols, int64_t* __restrict__ out_len) {
  const int b = blockIdx.z, f = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (f == 0 && t == 0 && out_len) out_len[b] = audio_length;   // length * 0 + audio_length (:710)
  if (t >= store_cols) return;
  int width = frames;
  if (wav_len) {
    const int64_t own = 1 + wav_len[b] / hop;
    width = own < frames ? (int)(own > 0 ? own : 0) : frames;
  }
  int src;
  if (width > audio_length) {
    int64_t o = off ? off[b] : 0;
    const int64_t hi = width - audio_length;
    o = o < 0 ? 0 : (o > hi ? hi : o);
    src = t + (int)o;
  } else {
    src = t - (audio_length - width) / 2;
  }
  float v = 0.f;
  if (t < audio_length && src >= 0 && src < width) v = in[((int64_t)b * feat + f) * ld_in + src];
  out[((int64_t)b * feat + f) * ld_out + t] = v;
}

// grid (channels / 4, batch): four rows per workgroup, a wavefront each
__global__ __launch_bounds__(256) void pool_kernel(const float* __restrict__ x, int64_t ld, int channels, int frames,
                                                   int pool_max, float* __restrict__ pooled) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= channels) return;
  const float* xr = x + ((int64_t)b * channels + c) * ld;
  float acc;
  if (pool_max) {
    acc = -INFINITY;
    for (int t = lane; t < frames; t += 64) acc = fmaxf(acc, xr[t]);
    acc = wave_max(acc);
  } else {
    acc = 0.f;
    for (int t = lane; t < frames; t += 64) acc += xr[t];
    acc = wave_sum(acc) / (float)frames;
  }
  if (lane == 0) pooled[(int64_t)b * channels + c] = acc;
}

// grid (classes / 4, batch): four classes per workgroup, a wavefront each; the utterance's pooled vector staged in LDS
__global__ __launch_bounds__(256) void linear_kernel(const float* __restrict__ pooled, const float* __restrict__ w,
                                                     const float* __restrict__ bias, int channels, int classes,
                                                     float* __restrict__ out) {
  __shared__ float p[kClassifyMaxChannels];
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  for (int c = threadIdx.x; c < channels; c += 256) p[c] = pooled[(int64_t)b * channels + c];
  __syncthreads();
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= classes) return;
  const float* wr = w + (int64_t)k * channels;
  float acc = 0.f;
  for (int c = lane; c < channels; c += 64) acc = fmaf(wr[c], p[c], acc);
  acc = wave_sum(acc);
  if (lane == 0) out[(int64_t)b * classes + k] = acc + bias[k];
}

// grid (batch): thread i takes classes i, i + 256, ...; the four wavefronts' partial results meet in LDS in wavefront order
__global__ __launch_bounds__(256) void softmax_kernel(float* __restrict__ x, int classes) {
  __shared__ float part[4];
  float* r = x + (int64_t)blockIdx.x * classes;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float m = -INFINITY;
  for (int k = threadIdx.x; k < classes; k += 256) m = fmaxf(m, r[k]);
  m = wave_max(m);
  if (lane == 0) part[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
  __syncthreads();
  float s = 0.f;
  for (int k = threadIdx.x; k < classes; k += 256) {
    const float e = expf(r[k] - m);
    r[k] = e;
    s += e;
  }
  s = wave_sum(s);
  if (lane == 0) part[wave] = s;
  __syncthreads();
  s = (part[0] + part[1]) + (part[2] + part[3]);
  for (int k = threadIdx.x; k < classes; k += 256) r[k] = r[k] / s;
}

}  // namespace

int launch_crop_or_pad(const float* in, int64_t ld_in, int batch, int feat, int frames, const int64_t* wav_len, int hop,
                       int audio_length, const int64_t* off, float* out, int64_t ld_out, int store_cols, int64_t* out_len,
                       hipStream_t st) {
  if (batch <= 0 || batch > 65535 || feat <= 0 || feat > 65535 || frames <= 0 || audio_length <= 0 || frames > ld_in ||
      store_cols < audio_length || store_cols > ld_out || (wav_len && hop <= 0))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(crop_pad_kernel, dim3((store_cols + 255) / 256, feat, batch), dim3(256), 0, st, in, ld_in, feat, frames,
                     wav_len, hop, audio_length, off, out, ld_out, store_cols, out_len);
  return (int)hipGetLastError();
}

int launch_classifier(const ClassifyLaunch& a, hipStream_t st) {
  if (a.batch <= 0 || a.batch > 65535 || a.channels <= 0 || a.channels > kClassifyMaxChannels || a.classes <= 0 ||
      a.frames <= 0 || a.frames > a.ld)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(pool_kernel, dim3((a.channels + 3) / 4, a.batch), dim3(256), 0, st, a.x, a.ld, a.channels, a.frames,
                     a.pool_max, a.pooled);
  hipLaunchKernelGGL(linear_kernel, dim3((a.classes + 3) / 4, a.batch), dim3(256), 0, st, a.pooled, a.w, a.bias, a.channels,
                     a.classes, a.out);
  if (a.softmax) hipLaunchKernelGGL(softmax_kernel, dim3(a.batch), dim3(256), 0, st, a.out, a.classes);
  return (int)hipGetLastError();
}

}  // namespace vasr
