// GroupNorm of a JasperBlock's convolution outputs (reference nemo/collections/asr/parts/jasper.py:385-391: nn.GroupNorm for
// normalization_mode "group" / "instance" / "layer") for gfx950: y = gamma[c] * (x - mu[b][g]) * rstd[b][g] + beta[c], mu and
// the biased variance over the group's channels x the row's own frames t < len_b, rstd = 1 / sqrt(var + 1e-5).
//
// Three small launches on the tensor a GEMM has just stored raw (scale 1, shift 0, no activation):
//   * norm_row_kernel:   one wavefront per (utterance, stored channel) row: the row mean, then M2 = sum (x - mean)^2 over
//                        t < len_b in a second pass over the same (L2-resident) row -- the centred two-pass form;
//   * norm_group_kernel: one wavefront per (utterance, norm group): the group mean as the mean of its rows' means (every row
//                        of an utterance has the same count), then M2 = sum_c M2_c + n * (mean_c - mean)^2 -- an exact merge
//                        of centred moments, never E[x^2] - E[x]^2 -- walking the group's channels in pre-shuffle order;
//   * norm_apply_kernel: y = act(gamma * (x - mu) * rstd + beta (+ add)) over the stored columns, zero from zero_lens[b] on
//                        (a row of length 0: zero throughout), and republishes the maxima table (AmaxTab) of the result for
//                        the fp16-split GEMM that reads it next.
// A grouped block stores its channels already shuffled (the split GEMM's epilogue, the block-diagonal form's permuted rows),
// while the reference normalizes BEFORE its GroupShuffle: a stored channel's norm group and its gamma / beta are those of its
// pre-shuffle channel -- `group_of` maps every stored channel to its group, `members` lists the stored channels of group g
// in pre-shuffle order, and gamma / beta come permuted (NormLaunch, built at finalize).
// Every reduction has one fixed order that depends on the row's length alone -- lane l of a wavefront adds t = l, l + 64,
// ... in turn, then a butterfly; a group walks its members the same way -- so results are run-to-run identical and do not
// depend on the batch a row is in or on the tensor's pitch.  No atomics.  Statistics in fp32, no FP64; built without
// packed-FP32 vectorisation (Makefile): these kernels run next to the MFMA GEMMs of other streams.
#include "vasr_internal.h"
#include "vasr_device.h"

namespace vasr {

namespace {

constexpr float kGroupNormEps = 1e-5f;   // nn.GroupNorm's default

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int row_frames(const int32_t* lens, int b, int frames) {
  int n = lens[b];
  n = n < frames ? n : frames;
  return n > 0 ? n : 0;
}

__global__ __launch_bounds__(256) void norm_row_kernel(const float* __restrict__ x, int64_t ld, int64_t bs, int channels,
                                                       int frames, const int32_t* __restrict__ lens,
                                                       float* __restrict__ row_mean, float* __restrict__ row_m2) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= channels) return;
  const int n = row_frames(lens, b, frames);
  const float* xr = x + (int64_t)b * bs + (int64_t)c * ld;
  float acc = 0.f;
  for (int t = lane; t < n; t += 64) acc += xr[t];
  const float mean = n > 0 ? wave_sum(acc) / (float)n : 0.f;
  float m2 = 0.f;
  for (int t = lane; t < n; t += 64) {
    const float d = xr[t] - mean;
    m2 = fmaf(d, d, m2);
  }
  m2 = wave_sum(m2);
  if (lane == 0) {
    row_mean[(int64_t)b * channels + c] = mean;
    row_m2[(int64_t)b * channels + c] = m2;
  }
}

__global__ __launch_bounds__(256) void norm_group_kernel(const float* __restrict__ row_mean, const float* __restrict__ row_m2,
                                                         int channels, int groups, int frames, const int32_t* __restrict__ lens,
                                                         const int32_t* __restrict__ members, float eps,
                                                         float* __restrict__ g_mean, float* __restrict__ g_rstd) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= groups) return;
  const int n = row_frames(lens, b, frames);
  const int cpg = channels / groups;
  const int32_t* mem = members + (int64_t)g * cpg;
  const float* mr = row_mean + (int64_t)b * channels;
  const float* m2r = row_m2 + (int64_t)b * channels;
  float acc = 0.f;
  for (int k = lane; k < cpg; k += 64) acc += mr[mem[k]];
  const float mean = wave_sum(acc) / (float)cpg;
  float m2 = 0.f;
  for (int k = lane; k < cpg; k += 64) {
    const int c = mem[k];
    const float d = mr[c] - mean;
    m2 += fmaf((float)n * d, d, m2r[c]);
  }
  m2 = wave_sum(m2);
  const float var = n > 0 ? m2 / ((float)n * (float)cpg) : 0.f;
  if (lane == 0) {
    g_mean[(int64_t)b * groups + g] = mean;
    g_rstd[(int64_t)b * groups + g] = 1.f / sqrtf(var + eps);
  }
}

// x and y may be the same tensor (in place); add (optional, [B][channels][ld_add], may equal y) is added before the activation
__global__ __launch_bounds__(256) void norm_apply_kernel(const float* x, float* y, const float* add, int64_t ld, int64_t bs,
                                                         int64_t ld_add,
                                                         int channels, int groups, int store_cols, int frames,
                                                         const int32_t* __restrict__ lens,
                                                         const int32_t* __restrict__ group_of, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ g_mean,
                                                         const float* __restrict__ g_rstd,
                                                         const int32_t* __restrict__ zero_lens, int relu, int act,
                                                         unsigned* __restrict__ amax, int amax_stride,
                                                         const int32_t* __restrict__ lens_y) {
  const int b = blockIdx.y;
  int zl = zero_lens ? zero_lens[b] : store_cols;
  zl = zl < store_cols ? zl : store_cols;
  if (row_frames(lens, b, frames) == 0) zl = 0;   // no frames: no statistics, zeros rather than beta or NaN
  int ny = lens_y ? lens_y[b] : frames;
  ny = ny < frames ? ny : frames;
  unsigned m = 0;
  for (int r = blockIdx.x; r < channels; r += gridDim.x) {
    const int g = group_of[r];
    const float mu = g_mean[(int64_t)b * groups + g];
    const float a = gamma[r] * g_rstd[(int64_t)b * groups + g];
    const float be = beta[r];
    const float* xr = x + (int64_t)b * bs + (int64_t)r * ld;
    float* yr = y + (int64_t)b * bs + (int64_t)r * ld;
    const float* ar = add ? add + ((int64_t)b * channels + r) * ld_add : nullptr;
    for (int t = threadIdx.x; t < store_cols; t += blockDim.x) {
      float v = 0.f;
      if (t < zl) {
        v = fmaf(xr[t] - mu, a, be);
        if (ar) v += ar[t];
        if (relu) v = activate(v, act);
      }
      yr[t] = v;
      if (t < ny) m = max(m, abs_bits(v));
    }
  }
  if (amax) amax_publish(amax, amax_stride, b, blockIdx.x * 4 + (threadIdx.x >> 6), m, threadIdx.x & 63);
}

}  // namespace

bool norm_supported(int channels, int groups) {
  return channels > 0 && groups > 0 && groups <= channels && channels % groups == 0;
}

int launch_norm(const NormLaunch& a, hipStream_t st) {
  if (!norm_supported(a.channels, a.groups) || a.store_cols > a.ld || (a.add && a.store_cols > a.ld_add)) return (int)hipErrorInvalidValue;
  const int64_t bs = a.bs ? a.bs : (int64_t)a.channels * a.ld;
  const int gx = a.channels < 64 ? a.channels : 64;
  if (a.amax_y && a.amax_y->p && gx * 4 > a.amax_y->stride) return (int)hipErrorInvalidValue;
  VASR_LAUNCH_PART(true, false, norm_row_kernel, dim3((a.channels + 3) / 4, a.batch), dim3(256), 0, st, a.x, a.ld, bs,
                   a.channels, a.frames, a.lens, a.row_mean, a.row_m2);
  VASR_LAUNCH_PART(false, false, norm_group_kernel, dim3((a.groups + 3) / 4, a.batch), dim3(256), 0, st, a.row_mean,
                   a.row_m2, a.channels, a.groups, a.frames, a.lens, a.members, kGroupNormEps, a.g_mean, a.g_rstd);
  unsigned* tab = a.amax_y ? a.amax_y->p : nullptr;
  if (tab) a.amax_y->n = gx * 4;
  VASR_LAUNCH_PART(false, true, norm_apply_kernel, dim3(gx, a.batch), dim3(256), 0, st, a.x, a.y, a.add, a.ld, bs,
                   a.add ? a.ld_add : a.ld, a.channels, a.groups, a.store_cols, a.frames, a.lens, a.group_of, a.gamma, a.beta, a.g_mean, a.g_rstd,
                   a.zero_lens, a.relu, a.act, tab, a.amax_y ? a.amax_y->stride : 0, a.lens_y);
  return (int)hipGetLastError();
}

}  // namespace vasr
