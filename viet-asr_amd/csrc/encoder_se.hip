// Squeeze-and-excitation of a JasperBlock (reference nemo/collections/asr/parts/jasper.py:152-168 SqueezeExcite, :223-253
// where the block puts it) for gfx950: y = x * sigmoid(W2 relu(W1 mean_t(x)))[b][c], W1 [H][C], W2 [C][H], no bias.
//
// Three small launches on the tensor a GEMM has just stored:
//   * se_sum_kernel:   one wavefront per (utterance, channel) row sums x[t] over t < len_b -- the row's own frames at that
//                      layer, never the padding (the reference's AdaptiveAvgPool1d averages the whole
//                      tensor width, which equals this whenever the row is as long as the tensor, e.g. every batch-1 call);
//   * se_mlp_kernel:   one workgroup per utterance: mean = sum / len, the two bias-free linear layers, ReLU and sigmoid in fp32;
//   * se_scale_kernel: y = act(x * s) (or y += x * s for the panes of a dense residual) over the stored columns, zero from
//                      zero_lens[b] on, and republishes the maxima table (AmaxTab) of the rescaled tensor for the fp16-split
//                      GEMM that reads it next.
// Every reduction has one fixed order that depends on the row's length alone -- lane l of a row's wavefront adds t = l,
// l + 64, ... in turn, then a butterfly; a hidden unit's dot product walks c the same way; an output's walks j in order --
// so results are run-to-run identical and do not depend on the batch a row is in or on the tensor's pitch.  No atomics.
// Built without packed-FP32 vectorisation and without FP64 (Makefile): these kernels run next to
// the MFMA GEMMs of other streams.
#include "vasr_internal.h"
#include "vasr_device.h"

namespace vasr {

namespace {

constexpr int kSeMaxChannels = 1024;

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void se_sum_kernel(const float* __restrict__ x, int64_t ld, int64_t bs, int channels,
                                                     int frames, const int32_t* __restrict__ lens, float* __restrict__ sums) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= channels) return;
  int n = lens[b];
  n = n < frames ? n : frames;
  const float* xr = x + (int64_t)b * bs + (int64_t)c * ld;
  float acc = 0.f;
  for (int t = lane; t < n; t += 64) acc += xr[t];
  acc = wave_sum(acc);
  if (lane == 0) sums[(int64_t)b * channels + c] = acc;
}

__global__ __launch_bounds__(256) void se_mlp_kernel(const float* __restrict__ sums, const int32_t* __restrict__ lens,
                                                     int frames, int channels, int hidden, const float* __restrict__ w1,
                                                     const float* __restrict__ w2, float* __restrict__ scale) {
  __shared__ float mean[kSeMaxChannels];
  __shared__ float hid[kSeMaxChannels];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int n = lens[b];
  n = n < frames ? n : frames;
  const float len = (float)(n > 0 ? n : 1);   // (an empty row sums to 0: its mean is 0)
  for (int c = threadIdx.x; c < channels; c += 256) mean[c] = sums[(int64_t)b * channels + c] / len;
  __syncthreads();
  for (int j = wave; j < hidden; j += 4) {
    const float* wr = w1 + (int64_t)j * channels;
    float acc = 0.f;
    for (int c = lane; c < channels; c += 64) acc = fmaf(wr[c], mean[c], acc);
    acc = wave_sum(acc);
    if (lane == 0) hid[j] = acc > 0.f ? acc : 0.f;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < channels; c += 256) {
    const float* wr = w2 + (int64_t)c * hidden;
    float acc = 0.f;
    for (int j = 0; j < hidden; ++j) acc = fmaf(wr[j], hid[j], acc);
    scale[(int64_t)b * channels + c] = 1.f / (1.f + expf(-acc));
  }
}

// x and y may be the same tensor (in place); accumulate 1: y += x * s, 2: y = max(y, x * s) (residual_mode "max"), instead
// of y = x * s
__global__ __launch_bounds__(256) void se_scale_kernel(const float* x, float* y, int64_t ld, int64_t bs, int channels,
                                                       int store_cols, const float* __restrict__ scale,
                                                       const int32_t* __restrict__ zero_lens, int relu, int act, int accumulate,
                                                       unsigned* __restrict__ amax, int amax_stride,
                                                       const int32_t* __restrict__ lens_y, int frames) {
  const int b = blockIdx.y;
  int zl = zero_lens ? zero_lens[b] : store_cols;
  zl = zl < store_cols ? zl : store_cols;
  int ny = lens_y ? lens_y[b] : frames;
  ny = ny < frames ? ny : frames;
  unsigned m = 0;
  for (int r = blockIdx.x; r < channels; r += gridDim.x) {
    const float s = scale[(int64_t)b * channels + r];
    const float* xr = x + (int64_t)b * bs + (int64_t)r * ld;
    float* yr = y + (int64_t)b * bs + (int64_t)r * ld;
    for (int t = threadIdx.x; t < store_cols; t += blockDim.x) {
      float v = 0.f;
      if (t < zl) {
        v = xr[t] * s;
        if (accumulate == 2) v = fmaxf(v, yr[t]);
        else if (accumulate) v += yr[t];
        if (relu) v = activate(v, act);
      }
      yr[t] = v;
      if (t < ny) m = max(m, abs_bits(v));
    }
  }
  if (amax) amax_publish(amax, amax_stride, b, blockIdx.x * 4 + (threadIdx.x >> 6), m, threadIdx.x & 63);
}

}  // namespace

bool se_supported(int channels, int hidden) {
  return channels > 0 && channels <= kSeMaxChannels && hidden > 0 && hidden <= kSeMaxChannels;
}

int launch_se(const SeLaunch& a, hipStream_t st) {
  if (!se_supported(a.channels, a.hidden) || a.store_cols > a.ld) return (int)hipErrorInvalidValue;
  const int64_t bs = a.bs ? a.bs : (int64_t)a.channels * a.ld;
  const int gx = a.channels < 64 ? a.channels : 64;
  if (a.amax_y && a.amax_y->p && gx * 4 > a.amax_y->stride) return (int)hipErrorInvalidValue;
  VASR_LAUNCH_PART(true, false, se_sum_kernel, dim3((a.channels + 3) / 4, a.batch), dim3(256), 0, st, a.x, a.ld, bs,
                   a.channels, a.frames, a.lens, a.sums);
  VASR_LAUNCH_PART(false, false, se_mlp_kernel, dim3(a.batch), dim3(256), 0, st, a.sums, a.lens, a.frames, a.channels,
                   a.hidden, a.w1, a.w2, a.scale);
  unsigned* tab = a.amax_y ? a.amax_y->p : nullptr;
  if (tab) a.amax_y->n = gx * 4;
  VASR_LAUNCH_PART(false, true, se_scale_kernel, dim3(gx, a.batch), dim3(256), 0, st, a.x, a.y, a.ld, bs, a.channels,
                   a.store_cols, a.scale, a.zero_lens, a.relu, a.act, a.accumulate, tab, a.amax_y ? a.amax_y->stride : 0,
                   a.lens_y, a.frames);
  return (int)hipGetLastError();
}

}  // namespace vasr
