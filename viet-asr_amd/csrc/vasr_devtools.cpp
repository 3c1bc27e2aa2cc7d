// What libvasr_hip_dev.so adds to the product library (include/vasr_devtools.h): the kernel-selection switches read from the
// environment, isolated-layer launches, the weight packers and the buffer plan of an encoder pass.  Compiled into the devtools
// build only (Makefile SRCS_DEV).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "vasr_devtools.h"
#include "vasr_model.h"   // vasr_plan_buffers: the one devtools entry point that needs the handle's insides

using namespace vasr;

// The devtools build's kernel-selection switches (vasr_internal.h DevSwitches): the environment is read HERE, once per
// process, and nowhere else; a value outside a switch's documented set aborts instead of silently meaning "default".
const vasr::DevSwitches& vasr::dev_switches() {
  static const DevSwitches sw = [] {
    DevSwitches s;
    auto num = [](const char* name, int dflt, std::initializer_list<int> allowed) {
      const char* e = getenv(name);
      if (!e) return dflt;
      const int v = atoi(e);
      for (int a : allowed) if (a == v) return v;
      fprintf(stderr, "vasr (devtools build): %s=%s is not a documented value -- refusing to guess\n", name, e);
      abort();
      return dflt;   // (not reached)
    };
    s.pw3_tile = num("VASR_PW3_TILE", 0, {0, 1, 2, 3, 4, 5});
    s.pw_lat = num("VASR_PW_LAT", 1, {0, 1});
    s.dw_pair = num("VASR_DW_PAIR", 1, {0, 1}) != 0;
    s.dw_mfma = num("VASR_DW_MFMA", 1, {0, 1}) != 0;
    s.dw_upw = num("VASR_DW_UPW", 0, {0, 1, 2, 3, 4, 5, 6, 7, 8});
    s.fused = num("VASR_FUSED", 1, {0, 1}) != 0;
    s.fused_min_tiles = getenv("VASR_FUSED_MIN_TILES") ? atoi(getenv("VASR_FUSED_MIN_TILES")) : 0;
    s.fused_tile = num("VASR_FUSED_TILE", 0, {0, 64, 128});
    s.fused_waves = num("VASR_FUSED_WAVES", 0, {0, 8, 16});
    s.fused_residual = num("VASR_NO_FUSED_RESIDUAL", 0, {0, 1}) == 0;
    s.beam_group = num("VASR_BEAM_GROUP", -1, {-1, 0, 1, 4});
    s.no_grouped = num("VASR_NO_GROUPED", 0, {0, 1}) != 0;
    if (const char* e = getenv("VASR_BUF_ROTATE")) {
      const std::string v(e);
      if (v != "pingpong" && v != "inplace") {
        fprintf(stderr, "vasr (devtools build): VASR_BUF_ROTATE=%s is not a documented value -- refusing to guess\n", e);
        abort();
      }
      s.buf_inplace = v == "inplace";
    }
    return s;
  }();
  return sw;
}

extern "C" {

int vasr_fused_tile_choice(int64_t tiles128, int compute_units) { return vasr::fused_tile_choice(tiles128, compute_units); }
int vasr_fused_waves_choice(int kernel, int dual, int tile_cols) {
  return vasr::fused_waves_choice(kernel, dual != 0, tile_cols, vasr::dev_switches().fused_waves);
}
int vasr_resample_form(double ratio, int nwin, int num_table, int* p, int* q) {
  if (!(ratio > 0.0) || nwin < 2 || num_table < 1 || (int)((ratio < 1.0 ? ratio : 1.0) * num_table) < 1)
    return fail(VASR_ERR_INVALID, "invalid ratio / table for resampling");   // what vasr_resample_f32 refuses
  return vasr::resample_form(ratio, nwin, num_table, p, q);
}

static __global__ void dev_noop_kernel() {}

int vasr_profile_bracket_overhead(vasr_stream stream, int n, double* out_us) {
  if (n < 1 || n > 4096 || !out_us) return fail(VASR_ERR_INVALID, "bad argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::vector<hipEvent_t> ev(2 * (size_t)n);
  for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
  for (int i = 0; i < n; ++i) {   // same shape as ProfScope: record, launch, record -- back to back on one stream
    HIP_TRY(hipEventRecord(ev[2 * i], st));
    hipLaunchKernelGGL(dev_noop_kernel, dim3(1), dim3(64), 0, st);
    HIP_TRY(hipEventRecord(ev[2 * i + 1], st));
  }
  HIP_TRY(hipEventSynchronize(ev.back()));
  std::vector<float> t(n);
  for (int i = 0; i < n; ++i) HIP_TRY(hipEventElapsedTime(&t[i], ev[2 * i], ev[2 * i + 1]));
  for (auto& e : ev) (void)hipEventDestroy(e);
  std::sort(t.begin(), t.end());
  *out_us = 1e3 * (double)t[n / 2];
  return 0;
}

int vasr_bench_depthwise(const float* d_x, const float* d_w, const int32_t* d_lens, int batch, int channels,
                         int64_t frames, int kernel, float* d_y, vasr_stream stream) {
  if (!d_x || !d_w || !d_lens || !d_y) return fail(VASR_ERR_INVALID, "bad argument");
  const int64_t ld = pad_frames(frames);
  (void)launch_depthwise(d_x, ld, (int)frames, d_w, d_lens, d_lens, batch, channels, kernel, 1, 1, kernel / 2, d_y, ld,
                         static_cast<hipStream_t>(stream));
  return check_launch("bench_depthwise");
}

int vasr_bench_depthwise_layer(const float* d_x, const float* d_w, const int32_t* d_lens_in, const int32_t* d_lens_out, int batch,
                               int channels, int64_t frames_in, int kernel, int stride, int dilation, float* d_y,
                               uint32_t* d_amax, int amax_stride, vasr_stream stream) {
  if (!d_x || !d_w || !d_lens_in || !d_lens_out || !d_y || batch < 1 || channels < 1 || frames_in < 1 ||
      frames_in > 0x7fffff00 || kernel < 1 || stride < 1 || dilation < 1)
    return fail(VASR_ERR_INVALID, "bad argument");
  if (stride > 1 && dilation > 1) return fail(VASR_ERR_INVALID, "only stride OR dilation may be greater than 1");
  const int pad = dilation > 1 ? (dilation * kernel) / 2 - 1 : kernel / 2;   // get_same_padding (jasper.py:60-65)
  const int64_t span = frames_in + 2 * pad - (int64_t)dilation * (kernel - 1) - 1;
  if (span < 0) return fail(VASR_ERR_INVALID, "no output frame");
  const int64_t ldx = pad_frames(frames_in), ldy = pad_frames(span / stride + 1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  AmaxTab ay{d_amax, amax_stride, 0};
  if (launch_depthwise(d_x, ldx, (int)frames_in, d_w, d_lens_in, d_lens_out, batch, channels, kernel, stride, dilation, pad,
                       d_y, ldy, st, d_amax ? &ay : nullptr))
    return fail(VASR_ERR_INVALID, "maxima table too small");
  // slots past the ones the launch used read as zero for the caller
  if (d_amax && ay.n < amax_stride)
    HIP_TRY(hipMemset2DAsync(d_amax + ay.n, (size_t)amax_stride * 4, 0, (size_t)(amax_stride - ay.n) * 4, batch, st));
  return check_launch("bench_depthwise_layer");
}

int vasr_depthwise_mfma_table_size(int kernel, int dilation) { return depthwise_mfma_table_size(kernel, dilation); }

int vasr_pack_depthwise_taps(const float* h_w, int channels, int kernel, int dilation, uint32_t* h_table, float* h_inv) {
  const int tsz = depthwise_mfma_table_size(kernel, dilation);
  if (!h_w || !h_table || !h_inv || channels <= 0 || !tsz) return fail(VASR_ERR_INVALID, "bad argument / shape not covered");
  for (int c = 0; c < channels; ++c)
    h_inv[c] = pack_depthwise_taps_f16x2(h_w + (size_t)c * kernel, kernel, dilation, tsz, h_table + (size_t)c * tsz);
  return 0;
}

int vasr_bench_depthwise_mfma(const float* d_x, const uint32_t* d_taps, const float* d_tap_inv, const int32_t* d_lens,
                              int batch, int channels, int64_t frames, int kernel, int dilation, float* d_y,
                              uint32_t* d_amax, int amax_stride, vasr_stream stream) {
  if (!d_x || !d_taps || !d_tap_inv || !d_lens || !d_y || !d_amax) return fail(VASR_ERR_INVALID, "bad argument");
  const int64_t ld = pad_frames(frames);
  if (amax_stride < 256 || amax_stride < depthwise_amax_slots(channels, ld)) return fail(VASR_ERR_INVALID, "maxima table too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  AmaxTab ax{d_amax, amax_stride, 0}, ay{d_amax + (size_t)batch * amax_stride, amax_stride, 0};
  launch_amax(d_x, ld, channels, (int)frames, d_lens, batch, &ax, st);
  const int e = launch_depthwise_mfma(d_x, ld, d_taps, d_tap_inv, d_lens, d_lens, ax, batch, channels, kernel, dilation,
                                      d_y, ld, &ay, st);
  if (e > 0) return fail(VASR_ERR_HIP, "depthwise (MFMA): %s", hipGetErrorString((hipError_t)e));
  if (e < 0) return fail(VASR_ERR_UNSUPPORTED, "no Toeplitz instantiation for kernel %d dilation %d", kernel, dilation);
  if (ay.n < amax_stride)
    HIP_TRY(hipMemset2DAsync(d_amax + (size_t)batch * amax_stride + ay.n, (size_t)amax_stride * 4, 0,
                             (size_t)(amax_stride - ay.n) * 4, batch, st));
  if (ax.n < amax_stride)
    HIP_TRY(hipMemset2DAsync(d_amax + ax.n, (size_t)amax_stride * 4, 0, (size_t)(amax_stride - ax.n) * 4, batch, st));
  return check_launch("bench_depthwise_mfma");
}

int vasr_pack_pointwise(const float* h_w, int cout, int cin, int m_pad, float* h_out) {
  if (!h_w || !h_out || cout <= 0 || cin % 8 || m_pad % 32 || m_pad < cout) return fail(VASR_ERR_INVALID, "bad argument");
  pack_pointwise_weights(h_w, cout, cin, m_pad, h_out);
  return 0;
}

int vasr_conv_gemm_weights(const float* h_w, int cout, int cin, int kernel, float* h_out) {
  if (!h_w || !h_out || cout <= 0 || cin <= 0 || kernel <= 0) return fail(VASR_ERR_INVALID, "bad argument");
  pack_conv_gemm_weights(h_w, cout, cin, kernel, h_out);
  return 0;
}

int vasr_bench_pointwise(const float* d_x, const float* d_wt, const float* d_scale, const float* d_shift, int batch,
                         int cin, int cout, int64_t frames, float* d_y, vasr_stream stream) {
  // in_channels % 64 like vasr_load_weight: the K % 32 tile (128 x 256) assumes a 256-frame pitch pad_frames() no longer gives
  if (!d_x || !d_wt || !d_scale || !d_shift || !d_y || cout % 128 || cin % 64)
    return fail(VASR_ERR_INVALID, "bad argument");
  const int64_t ld = pad_frames(frames);
  PwArgs a = pw_args(d_wt, d_scale, d_shift, cout, cin, d_x, d_y, ld, frames, batch);
  a.relu = 1;
  launch_pointwise(a, static_cast<hipStream_t>(stream));
  return check_launch("bench_pointwise");
}

int vasr_bench_mfma_sustained(int gemm_mode, int workgroups, int steps, float* d_sink, double* flops, vasr_stream stream) {
  if (workgroups < 1 || steps < 1 || !d_sink || !flops) return fail(VASR_ERR_INVALID, "bad argument");
  if (gemm_mode != 1 && gemm_mode != 3) return fail(VASR_ERR_INVALID, "gemm mode %d has no 16-bit MFMA stream (1 = bf16x3, 3 = f16x2)", gemm_mode);
  *flops = launch_mfma_sustained(gemm_mode, workgroups, steps, d_sink, static_cast<hipStream_t>(stream));
  return check_launch("mfma_sustained");
}

int vasr_pack_pointwise_bf16x3(const float* h_w, int cout, int cin, int m_pad, uint16_t* h_out) {
  if (!h_w || !h_out || cout <= 0 || cin % 16 || m_pad % 32 || m_pad < cout) return fail(VASR_ERR_INVALID, "bad argument");
  pack_pointwise_weights_bf16x3(h_w, cout, cin, m_pad, h_out);
  return 0;
}

int vasr_pack_pointwise_f16x2(const float* h_w, int cout, int cin, int m_pad, uint16_t* h_out, float* inv_scale) {
  if (!h_w || !h_out || !inv_scale || cout <= 0 || cin % 16 || m_pad % 32 || m_pad < cout)
    return fail(VASR_ERR_INVALID, "bad argument");
  *inv_scale = pack_pointwise_weights_f16x2(h_w, cout, cin, m_pad, h_out);
  return 0;
}

int vasr_bench_pointwise_f16x2(const float* d_x, const uint16_t* d_w16, float w_inv_scale, const float* d_scale,
                               const float* d_shift, int batch, int cin, int cout, int64_t frames, float* d_y,
                               uint32_t* d_amax, int amax_stride, vasr_stream stream) {
  if (!d_x || !d_w16 || !d_scale || !d_shift || !d_y || !d_amax || !pointwise_split_supported(cout, cin, 0))
    return fail(VASR_ERR_INVALID, "bad argument");
  const int64_t ld = pad_frames(frames);
  if (amax_stride < 256 || amax_stride < pointwise_amax_slots(cout, ld)) return fail(VASR_ERR_INVALID, "maxima table too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  AmaxTab ax{d_amax, amax_stride, 0};
  launch_amax(d_x, ld, cin, (int)frames, nullptr, batch, &ax, st);
  PwArgs a = pw_args(d_w16, d_scale, d_shift, cout, cin, d_x, d_y, ld, frames, batch);
  a.relu = 1;
  a.amax_x = ax; a.w_inv_scale = w_inv_scale;
  a.amax_y = AmaxTab{d_amax + (size_t)batch * amax_stride, amax_stride, 0};   // second table: maxima of y
  int n_y = 0;
  const int e = launch_pointwise_split(a, 2, st, &n_y);
  if (e) return fail(VASR_ERR_HIP, "pointwise GEMM: %s", hipGetErrorString((hipError_t)e));
  // slots past the ones the launch used read as zero for the caller
  if (n_y < amax_stride)
    HIP_TRY(hipMemset2DAsync(d_amax + (size_t)batch * amax_stride + n_y, (size_t)amax_stride * 4, 0,
                             (size_t)(amax_stride - n_y) * 4, batch, st));
  if (ax.n < amax_stride)
    HIP_TRY(hipMemset2DAsync(d_amax + ax.n, (size_t)amax_stride * 4, 0, (size_t)(amax_stride - ax.n) * 4, batch, st));
  return check_launch("bench_pointwise_f16x2");
}

int vasr_bench_pointwise_bf16x3(const float* d_x, const uint16_t* d_w3, const float* d_scale, const float* d_shift,
                                int batch, int cin, int cout, int64_t frames, float* d_y, vasr_stream stream) {
  if (!d_x || !d_w3 || !d_scale || !d_shift || !d_y || !pointwise_split_supported(cout, cin, 0))
    return fail(VASR_ERR_INVALID, "bad argument");
  const int64_t ld = pad_frames(frames);
  PwArgs a = pw_args(d_w3, d_scale, d_shift, cout, cin, d_x, d_y, ld, frames, batch);
  a.relu = 1;
  const int e = launch_pointwise_split(a, 0, static_cast<hipStream_t>(stream));
  if (e) return fail(VASR_ERR_HIP, "pointwise GEMM: %s", hipGetErrorString((hipError_t)e));
  return check_launch("bench_pointwise_bf16x3");
}

int vasr_bench_groupnorm(const float* d_x, const int32_t* d_lens, int batch, int channels, int64_t frames, int norm_groups,
                         int shuffle, const float* h_gamma, const float* h_beta, int relu, float* d_y, vasr_stream stream) {
  if (!d_x || !d_lens || !d_y || !h_gamma || !h_beta || batch < 1 || frames < 1 || shuffle < 1 || channels % shuffle ||
      !norm_supported(channels, norm_groups))
    return fail(VASR_ERR_INVALID, "bad argument");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t ld = pad_frames(frames);
  const NormTables t = norm_tables(h_gamma, h_beta, channels, norm_groups, shuffle);
  char* buf = nullptr;
  const size_t nc = (size_t)channels, ws = (size_t)2 * batch * (channels + norm_groups);
  HIP_TRY(hipMalloc(&buf, (4 * nc + ws) * 4));
  float* f = reinterpret_cast<float*>(buf);
  int32_t* i32 = reinterpret_cast<int32_t*>(buf);
  NormLaunch a{};
  a.x = d_x; a.y = d_y; a.add = nullptr; a.ld = ld; a.ld_add = ld; a.bs = 0;
  a.channels = channels; a.groups = norm_groups; a.batch = batch; a.frames = (int)frames; a.store_cols = (int)ld;
  a.lens = d_lens; a.gamma = f; a.beta = f + nc; a.group_of = i32 + 2 * nc; a.members = i32 + 3 * nc;
  a.row_mean = f + 4 * nc; a.row_m2 = a.row_mean + (size_t)batch * channels;
  a.g_mean = a.row_m2 + (size_t)batch * channels; a.g_rstd = a.g_mean + (size_t)batch * norm_groups;
  a.zero_lens = d_lens; a.relu = relu;
  hipError_t e = hipMemcpyAsync(buf, t.gamma.data(), nc * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(buf + nc * 4, t.beta.data(), nc * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(buf + 2 * nc * 4, t.group_of.data(), nc * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(buf + 3 * nc * 4, t.members.data(), nc * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = (hipError_t)launch_norm(a, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(buf);
  if (e != hipSuccess) return fail(VASR_ERR_HIP, "bench_groupnorm: %s", hipGetErrorString(e));
  return 0;
}

// include/vasr_devtools.h.  An unfinalized handle is planned on a host-side shadow: the same checks and build_encoder, with
// upload() allocating nothing; the pass itself is run_encoder's dry form, so the plan is made by the code that runs.
int vasr_plan_buffers(vasr_handle* h, int batch, int64_t samples, int64_t mel_frames, int32_t* out, int cap) {
  if (!h || !h->has_encoder || batch <= 0 || (samples <= 0 && mel_frames <= 0) || cap < 0 || (cap > 0 && !out))
    return fail(VASR_ERR_INVALID, "bad argument");
  if (samples > 0 && !(h->has_frontend && h->has_decoder))
    return fail(VASR_ERR_STATE, "a plan by samples is the transcribe path's: the handle needs a front end and a CTC head");
  if (h->profiling) return fail(VASR_ERR_STATE, "profiling is active");
  std::unique_ptr<vasr_handle> shadow;
  vasr_handle* e = h;
  if (!h->finalized) {
    shadow.reset(new vasr_handle(*h));
    e = shadow.get();
    e->plan_only = true;
    int rc;
    if ((rc = check_encoder(e)) || (rc = build_encoder(e))) return rc;
    e->weights.clear();
  }
  PlanRec rec;
  char* base = reinterpret_cast<char*>(uintptr_t{1} << 40);   // (no memory behind it: a dry pass only compares addresses)
  const int64_t T = samples > 0 ? vasr_mel_frames(e, samples) : mel_frames;
  if (samples > 0) {   // transcribe_any: every slice of the batch through transcribe_part
    const int n = n_slices(e, batch);
    for (int i = 0; i < n; ++i) {
      const int nb = slice_bounds(batch, i + 1, n) - slice_bounds(batch, i, n);
      const WsPlan p = plan_ws(e, nb, T);
      AmaxTab enc_amax{};
      const int32_t* own_frames = nullptr;
      if (int rc = run_encoder(e, reinterpret_cast<float*>(base + p.melp), p.Tp0, T, reinterpret_cast<int64_t*>(base + p.seq), nb,
                               reinterpret_cast<float*>(base + p.encp), p.Tp1, nullptr, base, p, nullptr, &enc_amax,
                               reinterpret_cast<const int64_t*>(base), &own_frames, true, &rec))
        return rc;
    }
  } else {             // vasr_encoder_f32: port tensors outside the workspace
    const WsPlan p = plan_ws(e, batch, T);
    const bool in_place = port_input_in_place(e);
    float* port_in = reinterpret_cast<float*>(base + p.total + 256);
    float* port_out = reinterpret_cast<float*>(base + p.total + 512);
    if (int rc = run_encoder(e, in_place ? port_in : reinterpret_cast<float*>(base + p.melp), in_place ? T : p.Tp0, T,
                             reinterpret_cast<int64_t*>(base + p.seq), batch, port_out, p.T1, nullptr, base, p, nullptr, nullptr,
                             nullptr, nullptr, false, &rec))
      return rc;
  }
  const int n = (int)(rec.v.size() / 5);
  if (out) std::copy_n(rec.v.begin(), (size_t)std::min(n, cap) * 5, out);
  return n;
}

int vasr_bench_ctc_head(const float* d_logits, int batch, int64_t frames, int num_classes, float* d_logp, int64_t* d_pred,
                        vasr_stream stream) {
  if (!d_logits || batch < 1 || frames < 1 || frames > 0x7fffff00 || num_classes < 1 || num_classes > 128 || (!d_logp && !d_pred))
    return fail(VASR_ERR_INVALID, "bench_ctc_head: batch %d, frames %lld, num_classes %d (1..128), logp %s, pred %s", batch,
                (long long)frames, num_classes, d_logp ? "given" : "NULL", d_pred ? "given" : "NULL");
  const int64_t ld = pad_frames(frames);
  launch_logsoftmax_argmax(d_logits, ld, (int64_t)num_classes * ld, batch, (int)frames, num_classes, d_logp, d_pred,
                           static_cast<hipStream_t>(stream));
  return check_launch("bench_ctc_head");
}

}  // extern "C"
