/* vasr_devtools.h -- measurement and development entry points of libvasr_hip_dev.so (built with -DVASR_DEVTOOLS).
 *
 * NOT part of the drop-in boundary (include/vasr.h): isolated-layer launches for roofline measurements, the host-side
 * weight packers the tests use to feed them, and the bracket-overhead probe.  The same build is the only one that reads
 * the VASR_* kernel-selection switches from the environment (VASR_DW_*, VASR_PW3_TILE, VASR_FUSED*, VASR_NO_*, ...: A/B
 * switches for tests/test_gpu_parity.py::test_alternate_kernel_paths_match_goldens and tools/); the product library
 * libvasr_hip.so exports none of these symbols and ignores those variables. */
#ifndef VASR_DEVTOOLS_H_
#define VASR_DEVTOOLS_H_
#include "vasr.h"
#ifdef __cplusplus
extern "C" {
#endif

/* What one event bracket adds to a bracketed launch: median elapsed time (microseconds) of n brackets around an empty
 * kernel, recorded back to back on `stream` exactly like the profiled launches.  A bracket measures "previous kernel
 * done -> this kernel done", i.e. the kernel plus its dispatch gap; bench.py reports class times both raw and with
 * launches x this value removed (the latter is what rocprofv3 --kernel-trace reports as kernel duration). */
VASR_API int vasr_profile_bracket_overhead(vasr_stream stream, int n, double* out_us);
/* The form a 256-channel separable sub-block takes (csrc/vasr_internal.h fused_tile_choice; pure host arithmetic): 128 / 64 =
 * the fused depthwise + pointwise kernel on tiles of that many frames, 0 = two kernels.  tiles128 = batch x padded frames / 128. */
VASR_API int vasr_fused_tile_choice(int64_t tiles128, int compute_units);
/* Wavefronts per workgroup (8 or 16) the fused kernel is launched with for a sub-block of depthwise kernel 33 | 39, with
 * (dual != 0) or without the folded residual, on tiles of tile_cols = 128 | 64 frames: VASR_FUSED_WAVES where it is set and the
 * form exists (the 128-frame tile), else the library's default (csrc/encoder_fused.hip fused_waves_choice; pure host arithmetic). */
VASR_API int vasr_fused_waves_choice(int kernel, int dual, int tile_cols);
/* Where one encoder pass puts its tensors (csrc/vasr_host.h BufRotation, through run_encoder's dry form; pure host arithmetic, no
 * device is touched).  h: a handle with its weights loaded, finalized or not (not finalized: the plan of a device of 256
 * compute units).  samples > 0: the pass of vasr_transcribe_greedy_*
 * on `batch` clips of that many samples (every slice of vasr_set_slices in turn); else the pass of vasr_encoder_f32 on
 * mel_frames frames.  Returns the number of launches (negative: a VASR_ERR_* code) and fills out[5 * i ...] of the first `cap`
 * with (kind, dst, src, src2, res): kind 0 = copy of a block input into the dense-residual pane buffer, 1 = depthwise -> D,
 * 2 = a sub-block's GEMM, 3 = fused depthwise + pointwise, 4 = a residual-branch GEMM, 5 = squeeze-and-excitation,
 * 6 = GroupNorm (5, 6 and a max-mode 4 work in place); buffers 0-3 = the rotation buffers, 4 = D, 5 = the pane buffer,
 * 6 = the encoder's input, 7 = its output, -1 = none.  VASR_BUF_ROTATE=pingpong|inplace picks the rotation. */
VASR_API int vasr_plan_buffers(vasr_handle* h, int batch, int64_t samples, int64_t mel_frames, int32_t* out, int cap);
/* The kernel vasr_resample_f32 runs a ratio on (csrc/audio.hip resample_form, which launch_resample itself calls; pure host
 * arithmetic): 2 = integer up-sampling (ratio p / 1, 2 <= p <= 16), 1 = the phase kernel (p / q with a denominator up to 1000
 * found within 1e-12 and wing tables within 60 KB of LDS), 0 = the generic per-output gather.  *p / *q (either may be NULL) receive
 * the ratio in lowest terms, 0 / 0 where none was found.  VASR_ERR_INVALID for the arguments vasr_resample_f32 refuses. */
VASR_API int vasr_resample_form(double ratio, int nwin, int num_table, int* p, int* q);
/* Run ONE encoder layer kind in isolation for benchmarking/roofline measurement:
 * kind 0 = depthwise (K, stride 1, dilation 1), 1 = pointwise GEMM (+BN+ReLU epilogue).
 * Buffers are caller provided [B][C][Tp] with Tp = vasr_padded_frames(T). */
VASR_API int vasr_bench_depthwise(const float* d_x, const float* d_w, const int32_t* d_lens, int batch, int channels,
                         int64_t frames, int kernel, float* d_y, vasr_stream stream);
/* One depthwise layer through the packed-FMA / generic kernels' own launcher (encoder_dw.hip launch_depthwise) with its full
 * argument list: any kernel / stride / dilation (not both > 1: VASR_ERR_INVALID, as the reference's get_same_padding refuses it),
 * pad = "same" padding of jasper.py:60-65.  x [B][C][vasr_padded_frames(frames_in)], y [B][C][vasr_padded_frames(t_out)] with
 * t_out = (frames_in + 2 pad - dilation (kernel - 1) - 1) / stride + 1; the caller supplies both length vectors (input mask,
 * output zeroed from d_lens_out[b] to the row pitch).  d_amax: NULL, or [batch][amax_stride] u32 receiving the per-wavefront
 * maxima of |y| (amax_stride >= channels * ceil(padded t_out / 256) * 4, else VASR_ERR_INVALID; unused slots are zeroed). */
VASR_API int vasr_bench_depthwise_layer(const float* d_x, const float* d_w, const int32_t* d_lens_in, const int32_t* d_lens_out,
                               int batch, int channels, int64_t frames_in, int kernel, int stride, int dilation, float* d_y,
                               uint32_t* d_amax, int amax_stride, vasr_stream stream);
/* Depthwise convolution on the matrix pipe (Toeplitz form, fp16-split arithmetic; stride 1, the (kernel, dilation) pairs
 * of the shipped models): vasr_depthwise_mfma_table_size = dwords per channel of the tap table (0 = shape not covered),
 * vasr_pack_depthwise_taps fills [channels][size] tables and [channels] inverse scales on the host; the bench call runs
 * one layer on [B][C][vasr_padded_frames(T)] buffers (dilation > 1: "same" padding as jasper.py:60-65).  d_amax as in
 * vasr_bench_pointwise_f16x2, amax_stride >= 256 and >= channels * ceil(padded frames / 256) * 4. */
VASR_API int vasr_depthwise_mfma_table_size(int kernel, int dilation);
VASR_API int vasr_pack_depthwise_taps(const float* h_w, int channels, int kernel, int dilation, uint32_t* h_table, float* h_inv);
VASR_API int vasr_bench_depthwise_mfma(const float* d_x, const uint32_t* d_taps, const float* d_tap_inv, const int32_t* d_lens,
                              int batch, int channels, int64_t frames, int kernel, int dilation, float* d_y,
                              uint32_t* d_amax, int amax_stride, vasr_stream stream);
/* Host helper: [cout][cin] row-major weights -> the MFMA fragment order the pointwise kernel streams
 * ([m_pad/32][cin/8][64 lanes][4], rows past cout zero); h_out holds m_pad*cin floats. */
VASR_API int vasr_pack_pointwise(const float* h_w, int cout, int cin, int m_pad, float* h_out);
/* Host helper: a non-separable conv's [cout][cin][kernel] weights -> the [cout][kernel * cin] matrix of its implicit GEMM
 * (reduction index k = tap * cin + c, input channel inner), which the vasr_pack_pointwise* packers then take with
 * cin' = kernel * cin -- the layout vasr_finalize packs K-tap convolutions in. */
VASR_API int vasr_conv_gemm_weights(const float* h_w, int cout, int cin, int kernel, float* h_out);
VASR_API int vasr_bench_pointwise(const float* d_x, const float* d_wt, const float* d_scale, const float* d_shift,
                         int batch, int cin, int cout, int64_t frames, float* d_y, vasr_stream stream);

/* Reference point for the GEMM roofline, like for like: launches `workgroups` x 8 wavefronts that issue nothing but the
 * MFMA stream of the pointwise kernel in arithmetic `gemm_mode` (vasr_set_gemm_mode numbering: 3 = f16x2 -- three
 * v_mfma_f32_32x32x16_f16 per tile pair and k-step on fp16 hi / lo planes, 24 per k-step; 1 = bf16x3 -- six
 * v_mfma_f32_32x32x16_bf16 on three planes, 48 per k-step), same 2 x 4 tile order, operands in registers with the bit
 * statistics of scaled weights and rectified activations; `steps` k-steps per wavefront; *flops = 16-bit flops issued.
 * Timed by the caller; what it sustains is the rate the chip holds under its power limit (box.measured_mfma_tflops). */
VASR_API int vasr_bench_mfma_sustained(int gemm_mode, int workgroups, int steps, float* d_sink, double* flops, vasr_stream stream);

/* 2 x fp16 scaled split variants (fragments: [m_pad/32][cin/16][2][64 lanes][8] fp16 bits; *inv_scale = 1 / the power
 * of two the weights were scaled by).  d_amax: [2][batch][amax_stride] u32 scratch (amax_stride >= 256 and >= cout *
 * frames / 1024) -- table 0 receives per-wavefront maxima of |x| per utterance (the call computes them), table 1 those of
 * |y|; unused slots are zeroed, so max over the last axis is the utterance's maximum. */
VASR_API int vasr_pack_pointwise_f16x2(const float* h_w, int cout, int cin, int m_pad, uint16_t* h_out, float* inv_scale);
VASR_API int vasr_bench_pointwise_f16x2(const float* d_x, const uint16_t* d_w16, float w_inv_scale, const float* d_scale,
                               const float* d_shift, int batch, int cin, int cout, int64_t frames, float* d_y,
                               uint32_t* d_amax, int amax_stride, vasr_stream stream);

/* 3 x bf16 split variants of the two helpers above (fragments: [m_pad/32][cin/16][3][64 lanes][8] bf16 bits). */
VASR_API int vasr_pack_pointwise_bf16x3(const float* h_w, int cout, int cin, int m_pad, uint16_t* h_out);
VASR_API int vasr_bench_pointwise_bf16x3(const float* d_x, const uint16_t* d_w3, const float* d_scale, const float* d_shift,
                                int batch, int cin, int cout, int64_t frames, float* d_y, vasr_stream stream);

/* GroupNorm's two device passes (encoder_norm.hip) in isolation: x, y [B][C][vasr_padded_frames(frames)], statistics over
 * t < d_lens[b] (and < frames), y = act(gamma (x - mean) rstd + beta), columns past the row's length stored as 0.
 * gamma / beta [C] on the host in PRE-shuffle order; shuffle = G_s > 1: the channels are stored after a GroupShuffle(G_s)
 * (stored channel j * G_s + g holds pre-shuffle channel g * (C / G_s) + j), 1: no shuffle.  Synchronous (allocates its own
 * tables).  VASR_ERR_INVALID when norm_groups does not divide C. */
VASR_API int vasr_bench_groupnorm(const float* d_x, const int32_t* d_lens, int batch, int channels, int64_t frames,
                                  int norm_groups, int shuffle, const float* h_gamma, const float* h_beta, int relu, float* d_y,
                                  vasr_stream stream);
/* The CTC head's epilogue alone (decode.hip launch_logsoftmax_argmax, as run_decoder calls it behind the head's GEMM):
 * d_logits [B][num_classes][vasr_padded_frames(frames)] class-major, columns >= frames are never read ->
 * d_logp [B][frames][num_classes] = log_softmax over the classes (or NULL) and d_pred [B][frames] int64 = the first index of
 * the row's maximum (or NULL).  The product's entry point vasr_decoder_logsoftmax_f32 passes no d_pred; this is the fused
 * arg-max without an engine around it.  VASR_ERR_INVALID, before any launch: num_classes outside 1..128 (the widest
 * instantiation), frames < 1, batch < 1, no logits, or both outputs NULL. */
VASR_API int vasr_bench_ctc_head(const float* d_logits, int batch, int64_t frames, int num_classes, float* d_logp,
                                 int64_t* d_pred, vasr_stream stream);
#ifdef __cplusplus
}
#endif
#endif /* VASR_DEVTOOLS_H_ */
