// The entry points of include/vasr.h that take no handle: decoding, scoring, CTC loss and alignment, audio intake, trim and
// split, the perturbations, the beam search and its LM tables.  Each is its refusals, then one launch.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "vasr_model.h"

using namespace vasr;

extern "C" {

int vasr_greedy_argmax(const float* d_logp, int batch, int64_t frames, int num_classes, int64_t* d_pred,
                       vasr_stream stream) {
  if (!d_logp || !d_pred || batch <= 0 || frames <= 0 || num_classes <= 0) return fail(VASR_ERR_INVALID, "bad argument");
  launch_argmax(d_logp, batch, frames, num_classes, d_pred, static_cast<hipStream_t>(stream));
  return check_launch("argmax");
}

int vasr_ctc_collapse(const int64_t* d_pred, int batch, int64_t frames, int blank_id, int32_t* d_ids,
                      int32_t* d_id_len, vasr_stream stream) {
  if (!d_pred || !d_ids || !d_id_len || batch <= 0 || frames < 0) return fail(VASR_ERR_INVALID, "bad argument");
  launch_ctc_collapse(d_pred, batch, frames, blank_id, d_ids, d_id_len, static_cast<hipStream_t>(stream));
  return check_launch("ctc_collapse");
}

// the word-separator ids of the three error-count calls, refused when there are too many or none are given
static int space_ids(const char* what, const int32_t* h_space_ids, int n_space, SpaceIds* sp) {
  if (n_space < 0 || n_space > kMetricsMaxSpace || (n_space > 0 && !h_space_ids))
    return fail(VASR_ERR_INVALID, "%s: n_space %d outside 0..%d (or no ids given)", what, n_space, kMetricsMaxSpace);
  sp->n = n_space;
  for (int k = 0; k < n_space; ++k) sp->id[k] = h_space_ids[k];
  return 0;
}

int vasr_error_counts_i32(const int32_t* d_hyp, int64_t hyp_width, const int32_t* d_hyp_len, const int32_t* d_ref,
                          int64_t ref_width, const int32_t* d_ref_len, int batch, const int32_t* h_space_ids, int n_space,
                          int32_t* d_counts, vasr_stream stream) {
  // every refusal comes before a device is touched
  if (!d_hyp || !d_hyp_len || !d_ref || !d_ref_len || !d_counts) return fail(VASR_ERR_INVALID, "error_counts: NULL pointer");
  if (batch <= 0 || hyp_width < 0 || ref_width < 0)
    return fail(VASR_ERR_INVALID, "error_counts: batch %d, widths %lld / %lld", batch, (long long)hyp_width, (long long)ref_width);
  SpaceIds sp{};
  if (int rc = space_ids("error_counts", h_space_ids, n_space, &sp)) return rc;
  if (reinterpret_cast<uintptr_t>(d_counts) & 15) return fail(VASR_ERR_INVALID, "error_counts: d_counts is not 16-byte aligned");
  if (hyp_width > kMetricsMaxWidth || ref_width > kMetricsMaxWidth)
    return fail(VASR_ERR_UNSUPPORTED, "error_counts: rows of %lld / %lld ids, at most %d per side", (long long)hyp_width,
                (long long)ref_width, kMetricsMaxWidth);
  const int rc = launch_error_counts(d_hyp, (int)hyp_width, d_hyp_len, d_ref, (int)ref_width, d_ref_len, batch, sp, d_counts,
                                     static_cast<hipStream_t>(stream));
  if (rc) return fail(VASR_ERR_HIP, "error_counts: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
  return check_launch("error_counts");
}

int vasr_error_ops_i32(const int32_t* d_hyp, int64_t hyp_width, const int32_t* d_hyp_len, const int32_t* d_ref,
                       int64_t ref_width, const int32_t* d_ref_len, int batch, const int32_t* h_space_ids, int n_space,
                       int32_t* d_ops_counts, int32_t* d_script, int32_t* d_script_len, vasr_stream stream) {
  // every refusal comes before a device is touched
  if (!d_hyp || !d_hyp_len || !d_ref || !d_ref_len || !d_ops_counts) return fail(VASR_ERR_INVALID, "error_ops: NULL pointer");
  if (!d_script != !d_script_len) return fail(VASR_ERR_INVALID, "error_ops: d_script and d_script_len go together (both or neither)");
  if (batch <= 0 || hyp_width < 0 || ref_width < 0)
    return fail(VASR_ERR_INVALID, "error_ops: batch %d, widths %lld / %lld", batch, (long long)hyp_width, (long long)ref_width);
  SpaceIds sp{};
  if (int rc = space_ids("error_ops", h_space_ids, n_space, &sp)) return rc;
  if (reinterpret_cast<uintptr_t>(d_ops_counts) & 15) return fail(VASR_ERR_INVALID, "error_ops: d_ops_counts is not 16-byte aligned");
  if (hyp_width > kMetricsMaxWidth || ref_width > kMetricsMaxWidth)
    return fail(VASR_ERR_UNSUPPORTED, "error_ops: rows of %lld / %lld ids, at most %d per side", (long long)hyp_width,
                (long long)ref_width, kMetricsMaxWidth);
  if (d_script && (hyp_width > kMetricsMaxScriptWidth || ref_width > kMetricsMaxScriptWidth))
    return fail(VASR_ERR_UNSUPPORTED, "error_ops: rows of %lld / %lld ids with a script, at most %d per side (counts alone: %d)",
                (long long)hyp_width, (long long)ref_width, kMetricsMaxScriptWidth, kMetricsMaxWidth);
  const int rc = launch_error_ops(d_hyp, (int)hyp_width, d_hyp_len, d_ref, (int)ref_width, d_ref_len, batch, sp, d_ops_counts,
                                  d_script, d_script_len, static_cast<hipStream_t>(stream));
  if (rc) return fail(VASR_ERR_HIP, "error_ops: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
  return check_launch("error_ops");
}

int vasr_nbest_error_counts_i32(const int32_t* d_ids, int64_t width, const int32_t* d_id_len, const int32_t* d_count, int nbest,
                                const int32_t* d_ref, int64_t ref_width, const int32_t* d_ref_len, int batch,
                                const int32_t* h_space_ids, int n_space, int32_t* d_slot_counts, int32_t* d_counts,
                                int32_t* d_slot, vasr_stream stream) {
  // every refusal comes before a device is touched
  if (!d_ids || !d_id_len || !d_count || !d_ref || !d_ref_len || !d_slot_counts)
    return fail(VASR_ERR_INVALID, "nbest_error_counts: NULL pointer");
  if (batch <= 0 || nbest < 1 || width < 0 || ref_width < 0)
    return fail(VASR_ERR_INVALID, "nbest_error_counts: batch %d, nbest %d, widths %lld / %lld", batch, nbest, (long long)width,
                (long long)ref_width);
  SpaceIds sp{};
  if (int rc = space_ids("nbest_error_counts", h_space_ids, n_space, &sp)) return rc;
  if ((reinterpret_cast<uintptr_t>(d_slot_counts) | reinterpret_cast<uintptr_t>(d_counts)) & 15)
    return fail(VASR_ERR_INVALID, "nbest_error_counts: d_slot_counts / d_counts is not 16-byte aligned");
  if (nbest > kMetricsMaxNbest)
    return fail(VASR_ERR_UNSUPPORTED, "nbest_error_counts: nbest %d, at most %d", nbest, kMetricsMaxNbest);
  if (width > kMetricsMaxWidth || ref_width > kMetricsMaxWidth)
    return fail(VASR_ERR_UNSUPPORTED, "nbest_error_counts: rows of %lld / %lld ids, at most %d per side", (long long)width,
                (long long)ref_width, kMetricsMaxWidth);
  const int rc = launch_nbest_error_counts(d_ids, (int)width, d_id_len, d_count, nbest, d_ref, (int)ref_width, d_ref_len, batch,
                                           sp, d_slot_counts, d_counts, d_slot, static_cast<hipStream_t>(stream));
  if (rc) return fail(VASR_ERR_HIP, "nbest_error_counts: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
  return check_launch("nbest_error_counts");
}

int vasr_class_scores_f32(const float* d_logits, int batch, int num_classes, const int64_t* d_targets, int k,
                          int32_t* d_topk_idx, float* d_topk_val, float* d_topk_prob, int32_t* d_rank, float* d_loss,
                          vasr_stream stream) {
  // every refusal comes before a device is touched
  if (!d_logits) return fail(VASR_ERR_INVALID, "class_scores: NULL logits");
  if (batch <= 0 || num_classes <= 0) return fail(VASR_ERR_INVALID, "class_scores: batch %d, num_classes %d", batch, num_classes);
  if (k < 0 || k > kClassScoresMaxK || k > num_classes)
    return fail(VASR_ERR_INVALID, "class_scores: k %d outside 0..%d or above num_classes %d", k, kClassScoresMaxK, num_classes);
  if ((d_rank || d_loss) && !d_targets) return fail(VASR_ERR_INVALID, "class_scores: d_rank / d_loss need d_targets");
  const bool topk = d_topk_idx || d_topk_val || d_topk_prob;
  if (k == 0 && !d_rank && !d_loss) return fail(VASR_ERR_INVALID, "class_scores: k == 0 and neither d_rank nor d_loss: nothing to do");
  if (k > 0 && !topk) return fail(VASR_ERR_INVALID, "class_scores: k %d without a top-k output", k);
  if (num_classes > kClassScoresMaxClasses)
    return fail(VASR_ERR_UNSUPPORTED, "class_scores: %d classes, at most %d", num_classes, kClassScoresMaxClasses);
  const int rc = launch_class_scores(d_logits, batch, num_classes, d_targets, k, d_topk_idx, d_topk_val, d_topk_prob, d_rank,
                                     d_loss, static_cast<hipStream_t>(stream));
  if (rc) return fail(VASR_ERR_HIP, "class_scores: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
  return check_launch("class_scores");
}

// what the two CTC calls refuse of their shape, in their order (have_workspace: the alignment's, refused before the width)
static int check_ctc_shape(const char* what, int batch, int64_t frames, int num_classes, int blank, int64_t tgt_width,
                           bool have_workspace = true) {
  if (batch <= 0 || frames < 0 || tgt_width < 0)
    return fail(VASR_ERR_INVALID, "%s: batch %d, frames %lld, tgt_width %lld", what, batch, (long long)frames, (long long)tgt_width);
  if (num_classes < 2 || blank < 0 || blank >= num_classes)
    return fail(VASR_ERR_INVALID, "%s: num_classes %d (at least 2), blank %d outside [0, num_classes)", what, num_classes, blank);
  if (!have_workspace) return fail(VASR_ERR_INVALID, "%s: NULL workspace", what);
  if (tgt_width > kCtcLossMaxWidth)
    return fail(VASR_ERR_UNSUPPORTED, "%s: targets of %lld ids, at most %d", what, (long long)tgt_width, kCtcLossMaxWidth);
  return 0;
}

int vasr_ctc_loss_f32(const float* d_logp, const int32_t* d_frames, int batch, int64_t frames, int num_classes, int blank,
                      const int32_t* d_tgt, int64_t tgt_width, const int32_t* d_tgt_len, float* d_loss, vasr_stream stream) {
  // every refusal comes before a device is touched
  if (!d_logp || !d_frames || !d_tgt || !d_tgt_len || !d_loss) return fail(VASR_ERR_INVALID, "ctc_loss: NULL pointer");
  if (int rc = check_ctc_shape("ctc_loss", batch, frames, num_classes, blank, tgt_width)) return rc;
  const int rc = launch_ctc_loss(d_logp, d_frames, batch, frames, num_classes, blank, d_tgt, (int)tgt_width, d_tgt_len, d_loss,
                                 static_cast<hipStream_t>(stream));
  if (rc) return fail(VASR_ERR_HIP, "ctc_loss: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
  return check_launch("ctc_loss");
}

size_t vasr_ctc_align_workspace_bytes(int batch, int64_t frames, int64_t tgt_width) {
  if (batch <= 0 || frames < 0 || tgt_width < 0 || tgt_width > kCtcLossMaxWidth) return 0;
  return ctc_align_workspace_bytes(batch, frames, (int)tgt_width);
}

int vasr_ctc_align_f32(const float* d_logp, const int32_t* d_frames, int batch, int64_t frames, int num_classes, int blank,
                       const int32_t* d_tgt, int64_t tgt_width, const int32_t* d_tgt_len, float* d_score, int32_t* d_start,
                       int32_t* d_end, float* d_tok_logp, int32_t* d_path, void* d_workspace, size_t workspace_bytes,
                       vasr_stream stream) {
  // every refusal comes before a device is touched
  if (!d_logp || !d_frames || !d_tgt || !d_tgt_len || !d_score || !d_start || !d_end)
    return fail(VASR_ERR_INVALID, "ctc_align: NULL pointer");
  if (int rc = check_ctc_shape("ctc_align", batch, frames, num_classes, blank, tgt_width, d_workspace != nullptr)) return rc;
  const size_t need = ctc_align_workspace_bytes(batch, frames, (int)tgt_width);
  if (workspace_bytes < need)
    return fail(VASR_ERR_INVALID, "ctc_align: workspace of %zu bytes, %zu needed (vasr_ctc_align_workspace_bytes)", workspace_bytes, need);
  const int rc = launch_ctc_align(d_logp, d_frames, batch, frames, num_classes, blank, d_tgt, (int)tgt_width, d_tgt_len, d_score,
                                  d_start, d_end, d_tok_logp, d_path, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  if (rc) return fail(VASR_ERR_HIP, "ctc_align: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
  return check_launch("ctc_align");
}

// crop or centre-pad of the classification path (classify.hip)
int vasr_crop_or_pad_f32(const float* d_in, int batch, int feat, int64_t frames, int64_t audio_length, const int64_t* d_offsets,
                         float* d_out, int64_t* d_out_len, vasr_stream stream) {
  if (!d_in || !d_out || batch <= 0 || feat <= 0 || frames <= 0 || audio_length <= 0 || frames > INT32_MAX ||
      audio_length > INT32_MAX)
    return fail(VASR_ERR_INVALID, "bad argument");
  if (frames > audio_length && !d_offsets)
    return fail(VASR_ERR_INVALID, "%lld frames are cropped to %lld: offsets needed", (long long)frames, (long long)audio_length);
  const int e = launch_crop_or_pad(d_in, frames, batch, feat, (int)frames, nullptr, 0, (int)audio_length, d_offsets, d_out,
                                   audio_length, (int)audio_length, d_out_len, static_cast<hipStream_t>(stream));
  if (e) return fail(VASR_ERR_HIP, "crop_or_pad: %s", hipGetErrorString((hipError_t)e));
  return 0;
}

// SpecAugment / SpecCutout rectangles (spec_augment.hip)
int vasr_spec_mask_f32(const float* d_in, int64_t ld_in, float* d_out, int64_t ld_out, int batch, int feat, int64_t frames,
                       const int32_t* d_rects, const int32_t* d_row_begin, vasr_stream stream) {
  // every refusal comes before a device is touched
  if (!d_in || !d_out || !d_rects || !d_row_begin) return fail(VASR_ERR_INVALID, "spec_mask: NULL pointer");
  if (batch <= 0 || feat <= 0 || frames <= 0 || ld_in < frames || ld_out < frames)
    return fail(VASR_ERR_INVALID, "spec_mask: batch %d, feat %d, frames %lld, ld_in %lld, ld_out %lld (all >= 1, ld >= frames)", batch,
                feat, (long long)frames, (long long)ld_in, (long long)ld_out);
  if ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 3)
    return fail(VASR_ERR_INVALID, "spec_mask: d_in and d_out must be 4-byte aligned");
  if (d_in != d_out || ld_in != ld_out) {
    // the bytes either tensor spans up to the last row's valid frames (in doubles: the products of refused sizes do not wrap)
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_in), b = reinterpret_cast<uintptr_t>(d_out);
    const double rows = (double)batch * feat - 1.0;
    const double ea = (double)a + 4.0 * (rows * (double)ld_in + (double)frames);
    const double eb = (double)b + 4.0 * (rows * (double)ld_out + (double)frames);
    if (d_in == d_out || ((double)a < eb && (double)b < ea))
      return fail(VASR_ERR_INVALID, "spec_mask: d_in and d_out overlap without being the same tensor (same pointer and pitch)");
  }
  if (!spec_mask_grid_fits(batch, feat, frames))
    return fail(VASR_ERR_UNSUPPORTED, "spec_mask: batch %d x feat %d x frames %lld needs more workgroups than one launch holds", batch,
                feat, (long long)frames);
  launch_spec_mask(d_in, ld_in, d_out, ld_out, batch, feat, (int)frames, d_rects, d_row_begin, static_cast<hipStream_t>(stream));
  return check_launch("spec_mask");
}

int vasr_pcm16_to_f32(const int16_t* d_pcm, int64_t n, float* d_out, vasr_stream stream) {
  if (!d_pcm || !d_out || n < 0) return fail(VASR_ERR_INVALID, "bad argument");
  if (n == 0) return 0;
  if ((reinterpret_cast<uintptr_t>(d_pcm) & 7) || (reinterpret_cast<uintptr_t>(d_out) & 15))
    return fail(VASR_ERR_INVALID, "pcm / float buffers must be 8 / 16-byte aligned");
  launch_pcm16_to_f32(d_pcm, n, d_out, static_cast<hipStream_t>(stream));
  return check_launch("pcm16_to_f32");
}

int vasr_resample_f32(const float* d_in, int64_t ld_in, const int64_t* d_len_in, int batch, const float* d_table,
                      int nwin, int num_table, double ratio, float* d_out, int64_t ld_out, int64_t* d_len_out,
                      vasr_stream stream) {
  if (!d_in || !d_len_in || !d_table || !d_out || !d_len_out || batch <= 0 || ld_in <= 0 || ld_out <= 0)
    return fail(VASR_ERR_INVALID, "bad argument");
  if (!(ratio > 0.0) || nwin < 2 || num_table < 1 || (int)((ratio < 1.0 ? ratio : 1.0) * num_table) < 1)
    return fail(VASR_ERR_INVALID, "invalid ratio / table for resampling");
  launch_resample(d_in, ld_in, d_len_in, batch, d_table, nwin, num_table, ratio, d_out, ld_out, d_len_out,
                  static_cast<hipStream_t>(stream));
  return check_launch("resample");
}

static bool trim_shape_supported(int frame_length, int hop_length) {
  return hop_length >= 1 && frame_length >= hop_length && frame_length <= kTrimMaxFrame && frame_length % hop_length == 0;
}

size_t vasr_trim_silence_workspace_bytes(int batch, int64_t ld_in, int frame_length, int hop_length) {
  if (batch <= 0 || ld_in < 0 || !trim_shape_supported(frame_length, hop_length)) return 0;
  return trim_workspace_bytes(batch, ld_in, frame_length, hop_length);
}

extern "C++" {
template <typename T>
static int trim_silence(const T* d_in, int64_t ld_in, const int64_t* d_len, int batch, float top_db, int frame_length,
                        int hop_length, T* d_out, int64_t ld_out, int64_t* d_len_out, int64_t* d_start, void* d_workspace,
                        size_t workspace_bytes, vasr_stream stream) {
  // every refusal comes before a device is touched
  if (!d_in || !d_len || !d_out || !d_len_out) return fail(VASR_ERR_INVALID, "trim_silence: NULL pointer");
  if (d_in == d_out) return fail(VASR_ERR_INVALID, "trim_silence: d_out must not alias d_in");
  if (batch <= 0 || ld_in < 0 || ld_out < 0 || ld_out < ld_in)
    return fail(VASR_ERR_INVALID, "trim_silence: batch %d, ld_in %lld, ld_out %lld (ld_out >= ld_in >= 0)", batch, (long long)ld_in,
                (long long)ld_out);
  if (!std::isfinite(top_db)) return fail(VASR_ERR_INVALID, "trim_silence: top_db is not finite");
  if (!d_workspace) return fail(VASR_ERR_INVALID, "trim_silence: NULL workspace");
  if (!trim_shape_supported(frame_length, hop_length))
    return fail(VASR_ERR_UNSUPPORTED, "trim_silence: frame_length %d, hop_length %d: hop_length >= 1 and frame_length a multiple of "
                "it, at most %d", frame_length, hop_length, kTrimMaxFrame);
  const size_t need = trim_workspace_bytes(batch, ld_in, frame_length, hop_length);
  if (workspace_bytes < need)
    return fail(VASR_ERR_INVALID, "trim_silence: workspace of %zu bytes, %zu needed (vasr_trim_silence_workspace_bytes)",
                workspace_bytes, need);
  const double factor = std::pow(10.0, -(double)top_db / 10.0);
  launch_trim_silence<T>(d_in, ld_in, d_len, batch, factor, frame_length, hop_length, d_out, ld_out, d_len_out, d_start, d_workspace,
                         static_cast<hipStream_t>(stream));
  return check_launch("trim_silence");
}
}  // extern "C++"

int vasr_trim_silence_f32(const float* d_in, int64_t ld_in, const int64_t* d_len, int batch, float top_db, int frame_length,
                          int hop_length, float* d_out, int64_t ld_out, int64_t* d_len_out, int64_t* d_start, void* d_workspace,
                          size_t workspace_bytes, vasr_stream stream) {
  return trim_silence<float>(d_in, ld_in, d_len, batch, top_db, frame_length, hop_length, d_out, ld_out, d_len_out, d_start,
                             d_workspace, workspace_bytes, stream);
}

int vasr_trim_silence_pcm16(const int16_t* d_in, int64_t ld_in, const int64_t* d_len, int batch, float top_db, int frame_length,
                            int hop_length, int16_t* d_out, int64_t ld_out, int64_t* d_len_out, int64_t* d_start,
                            void* d_workspace, size_t workspace_bytes, vasr_stream stream) {
  return trim_silence<short>(d_in, ld_in, d_len, batch, top_db, frame_length, hop_length, d_out, ld_out, d_len_out, d_start,
                             d_workspace, workspace_bytes, stream);
}

size_t vasr_split_silence_workspace_bytes(int batch, int64_t ld_in, int frame_length, int hop_length) {
  if (batch <= 0 || ld_in < 0 || !trim_shape_supported(frame_length, hop_length)) return 0;
  return split_workspace_bytes(batch, ld_in, frame_length, hop_length);
}

extern "C++" {
template <typename T>
static int split_silence(const T* d_in, int64_t ld_in, const int64_t* d_len, int batch, float top_db, int frame_length,
                         int hop_length, int min_silence_frames, int max_segment_frames, int64_t* d_bounds, int64_t max_segments,
                         int64_t* d_count, void* d_workspace, size_t workspace_bytes, vasr_stream stream) {
  // every refusal comes before a device is touched
  if (!d_in || !d_len || !d_bounds || !d_count) return fail(VASR_ERR_INVALID, "split_silence: NULL pointer");
  if (batch <= 0 || ld_in < 0 || max_segments < 0)
    return fail(VASR_ERR_INVALID, "split_silence: batch %d, ld_in %lld, max_segments %lld (batch >= 1, ld_in >= 0, max_segments >= 0)",
                batch, (long long)ld_in, (long long)max_segments);
  if (min_silence_frames < 1 || max_segment_frames < 0 || max_segment_frames == 1)
    return fail(VASR_ERR_INVALID, "split_silence: min_silence_frames %d (>= 1), max_segment_frames %d (0 = no limit, or >= 2)",
                min_silence_frames, max_segment_frames);
  if (!std::isfinite(top_db)) return fail(VASR_ERR_INVALID, "split_silence: top_db is not finite");
  if (!d_workspace) return fail(VASR_ERR_INVALID, "split_silence: NULL workspace");
  if (!trim_shape_supported(frame_length, hop_length))
    return fail(VASR_ERR_UNSUPPORTED, "split_silence: frame_length %d, hop_length %d: hop_length >= 1 and frame_length a multiple of "
                "it, at most %d", frame_length, hop_length, kTrimMaxFrame);
  const size_t need = split_workspace_bytes(batch, ld_in, frame_length, hop_length);
  if (workspace_bytes < need)
    return fail(VASR_ERR_INVALID, "split_silence: workspace of %zu bytes, %zu needed (vasr_split_silence_workspace_bytes)",
                workspace_bytes, need);
  const double factor = std::pow(10.0, -(double)top_db / 10.0);
  launch_split_silence<T>(d_in, ld_in, d_len, batch, factor, frame_length, hop_length, min_silence_frames, max_segment_frames,
                          d_bounds, max_segments, d_count, d_workspace, static_cast<hipStream_t>(stream));
  return check_launch("split_silence");
}

template <typename T>
static int gather_segments(const T* d_in, int64_t ld_in, int batch, const int32_t* d_row, const int64_t* d_start,
                           const int64_t* d_len, int64_t segments, T* d_out, int64_t ld_out, vasr_stream stream) {
  if (!d_in || !d_row || !d_start || !d_len || !d_out) return fail(VASR_ERR_INVALID, "gather_segments: NULL pointer");
  if (d_in == d_out) return fail(VASR_ERR_INVALID, "gather_segments: d_out must not alias d_in");
  if (batch <= 0 || ld_in < 0 || segments <= 0 || ld_out <= 0)
    return fail(VASR_ERR_INVALID, "gather_segments: batch %d, ld_in %lld, segments %lld, ld_out %lld (batch, segments, ld_out >= 1, "
                "ld_in >= 0)", batch, (long long)ld_in, (long long)segments, (long long)ld_out);
  launch_gather_segments<T>(d_in, ld_in, batch, d_row, d_start, d_len, segments, d_out, ld_out, static_cast<hipStream_t>(stream));
  return check_launch("gather_segments");
}
}  // extern "C++"

int vasr_split_silence_f32(const float* d_in, int64_t ld_in, const int64_t* d_len, int batch, float top_db, int frame_length,
                           int hop_length, int min_silence_frames, int max_segment_frames, int64_t* d_bounds, int64_t max_segments,
                           int64_t* d_count, void* d_workspace, size_t workspace_bytes, vasr_stream stream) {
  return split_silence<float>(d_in, ld_in, d_len, batch, top_db, frame_length, hop_length, min_silence_frames, max_segment_frames,
                              d_bounds, max_segments, d_count, d_workspace, workspace_bytes, stream);
}

int vasr_split_silence_pcm16(const int16_t* d_in, int64_t ld_in, const int64_t* d_len, int batch, float top_db, int frame_length,
                             int hop_length, int min_silence_frames, int max_segment_frames, int64_t* d_bounds, int64_t max_segments,
                             int64_t* d_count, void* d_workspace, size_t workspace_bytes, vasr_stream stream) {
  return split_silence<short>(d_in, ld_in, d_len, batch, top_db, frame_length, hop_length, min_silence_frames, max_segment_frames,
                              d_bounds, max_segments, d_count, d_workspace, workspace_bytes, stream);
}

int vasr_gather_segments_f32(const float* d_in, int64_t ld_in, int batch, const int32_t* d_row, const int64_t* d_start,
                             const int64_t* d_len, int64_t segments, float* d_out, int64_t ld_out, vasr_stream stream) {
  return gather_segments<float>(d_in, ld_in, batch, d_row, d_start, d_len, segments, d_out, ld_out, stream);
}

int vasr_gather_segments_pcm16(const int16_t* d_in, int64_t ld_in, int batch, const int32_t* d_row, const int64_t* d_start,
                               const int64_t* d_len, int64_t segments, int16_t* d_out, int64_t ld_out, vasr_stream stream) {
  return gather_segments<short>(d_in, ld_in, batch, d_row, d_start, d_len, segments, d_out, ld_out, stream);
}

size_t vasr_mean_square_workspace_bytes(int batch, int64_t ld_in) {
  if (batch <= 0 || ld_in < 0) return 0;
  return mean_square_workspace_bytes(batch, ld_in);
}

int vasr_mean_square_f32(const float* d_in, int64_t ld_in, const int64_t* d_len, int batch, double* d_ms, void* d_workspace,
                         size_t workspace_bytes, vasr_stream stream) {
  // every refusal comes before a device is touched
  if (!d_in || !d_len || !d_ms) return fail(VASR_ERR_INVALID, "mean_square: NULL pointer");
  if (batch <= 0 || ld_in < 0) return fail(VASR_ERR_INVALID, "mean_square: batch %d, ld_in %lld (batch >= 1, ld_in >= 0)", batch,
                                           (long long)ld_in);
  if (!d_workspace) return fail(VASR_ERR_INVALID, "mean_square: NULL workspace");
  const size_t need = mean_square_workspace_bytes(batch, ld_in);
  if (workspace_bytes < need)
    return fail(VASR_ERR_INVALID, "mean_square: workspace of %zu bytes, %zu needed (vasr_mean_square_workspace_bytes)",
                workspace_bytes, need);
  launch_mean_square(d_in, ld_in, d_len, batch, d_ms, d_workspace, static_cast<hipStream_t>(stream));
  return check_launch("mean_square");
}

int vasr_noise_plan_f64(const int64_t* d_len, const double* d_ms_x, const int32_t* d_row, const double* d_snr_db, const double* d_u,
                        int batch, const int64_t* d_noise_len, const double* d_ms_v, int noise_rows, double max_gain_db,
                        int sample_rate, float* d_scale, int64_t* d_start, vasr_stream stream) {
  if (!d_len || !d_ms_x || !d_row || !d_snr_db || !d_u || !d_noise_len || !d_ms_v || !d_scale || !d_start)
    return fail(VASR_ERR_INVALID, "noise_plan: NULL pointer");
  if (batch <= 0 || noise_rows <= 0 || sample_rate <= 0)
    return fail(VASR_ERR_INVALID, "noise_plan: batch %d, noise_rows %d, sample_rate %d (all >= 1)", batch, noise_rows, sample_rate);
  if (std::isnan(max_gain_db)) return fail(VASR_ERR_INVALID, "noise_plan: max_gain_db is not a number");
  double cap = std::pow(10.0, max_gain_db / 20.0);
  cap = cap > (double)FLT_MAX ? (double)FLT_MAX : cap;
  launch_noise_plan(d_len, d_ms_x, d_row, d_snr_db, d_u, batch, d_noise_len, d_ms_v, noise_rows, cap, sample_rate, d_scale, d_start,
                    static_cast<hipStream_t>(stream));
  return check_launch("noise_plan");
}

int vasr_mix_f32(const float* d_in, int64_t ld_in, const int64_t* d_len, int batch, const float* d_gain, const int64_t* d_shift,
                 const float* d_add, int64_t ld_add, int add_rows, const int64_t* d_add_len, const int32_t* d_add_row,
                 const float* d_scale, const int64_t* d_start, float* d_out, int64_t ld_out, vasr_stream stream) {
  if (!d_in || !d_len || !d_out) return fail(VASR_ERR_INVALID, "mix: NULL pointer");
  if (d_in == d_out) return fail(VASR_ERR_INVALID, "mix: d_out must not alias d_in");
  if (batch <= 0 || ld_in < 0 || ld_out < ld_in)
    return fail(VASR_ERR_INVALID, "mix: batch %d, ld_in %lld, ld_out %lld (ld_out >= ld_in >= 0)", batch, (long long)ld_in,
                (long long)ld_out);
  if (d_add && (!d_add_len || !d_add_row || !d_scale))
    return fail(VASR_ERR_INVALID, "mix: an addend needs d_add_len, d_add_row and d_scale");
  if (d_add && (ld_add < 0 || add_rows <= 0))
    return fail(VASR_ERR_INVALID, "mix: ld_add %lld, add_rows %d (ld_add >= 0, add_rows >= 1)", (long long)ld_add, add_rows);
  if (d_add == d_out) return fail(VASR_ERR_INVALID, "mix: d_out must not alias d_add");
  launch_mix(d_in, ld_in, d_len, batch, d_gain, d_shift, d_add, ld_add, add_rows, d_add_len, d_add_row, d_scale, d_start, d_out,
             ld_out, static_cast<hipStream_t>(stream));
  return check_launch("mix");
}

static const char* convolve_bank_error(int R, int64_t ld_ir) {
  if (R <= 0 || ld_ir < 1) return "R >= 1 and ld_ir >= 1";
  return nullptr;
}

size_t vasr_convolve_spectra_bytes(int R, int64_t ld_ir) {
  if (convolve_bank_error(R, ld_ir) || ld_ir > kConvMaxTaps || R > 65535) return 0;
  return convolve_spectra_bytes(R, ld_ir);
}

int vasr_convolve_prepare_f32(const float* d_ir, int64_t ld_ir, const int64_t* d_ir_len, int R, void* d_spectra,
                              size_t spectra_bytes, vasr_stream stream) {
  if (!d_ir || !d_ir_len || !d_spectra) return fail(VASR_ERR_INVALID, "convolve_prepare: NULL pointer");
  if (convolve_bank_error(R, ld_ir))
    return fail(VASR_ERR_INVALID, "convolve_prepare: R %d, ld_ir %lld (%s)", R, (long long)ld_ir, convolve_bank_error(R, ld_ir));
  if (reinterpret_cast<uintptr_t>(d_spectra) % 8) return fail(VASR_ERR_INVALID, "convolve_prepare: d_spectra must be 8-byte aligned");
  if (ld_ir > kConvMaxTaps || R > 65535)
    return fail(VASR_ERR_UNSUPPORTED, "convolve_prepare: ld_ir %lld, R %d: at most %lld taps and 65535 responses", (long long)ld_ir, R,
                (long long)kConvMaxTaps);
  const size_t need = convolve_spectra_bytes(R, ld_ir);
  if (spectra_bytes < need)
    return fail(VASR_ERR_INVALID, "convolve_prepare: spectra buffer of %zu bytes, %zu needed (vasr_convolve_spectra_bytes)",
                spectra_bytes, need);
  const int e = launch_convolve_prepare(d_ir, ld_ir, d_ir_len, R, d_spectra, static_cast<hipStream_t>(stream));
  if (e) return fail(VASR_ERR_HIP, "convolve_prepare: twiddle table copy: %s", hipGetErrorString((hipError_t)e));
  return check_launch("convolve_prepare");
}

int vasr_convolve_f32(const float* d_in, int64_t ld_in, const int64_t* d_len, int batch, const int32_t* d_ir_row,
                      const int64_t* d_ir_len, const void* d_spectra, int R, int64_t ld_ir, float* d_out, int64_t ld_out,
                      int64_t* d_len_out, vasr_stream stream) {
  if (!d_in || !d_len || !d_ir_row || !d_ir_len || !d_spectra || !d_out || !d_len_out)
    return fail(VASR_ERR_INVALID, "convolve: NULL pointer");
  if (d_in == d_out) return fail(VASR_ERR_INVALID, "convolve: d_out must not alias d_in");
  if (batch <= 0 || ld_in < 0) return fail(VASR_ERR_INVALID, "convolve: batch %d, ld_in %lld (batch >= 1, ld_in >= 0)", batch,
                                           (long long)ld_in);
  if (convolve_bank_error(R, ld_ir))
    return fail(VASR_ERR_INVALID, "convolve: R %d, ld_ir %lld (%s)", R, (long long)ld_ir, convolve_bank_error(R, ld_ir));
  if (ld_out < 1 || ld_out - ld_ir + 1 < ld_in)
    return fail(VASR_ERR_INVALID, "convolve: ld_out %lld (>= 1 and >= ld_in + ld_ir - 1 = %lld)", (long long)ld_out,
                (long long)(ld_in + ld_ir - 1));
  if (reinterpret_cast<uintptr_t>(d_spectra) % 8) return fail(VASR_ERR_INVALID, "convolve: d_spectra must be 8-byte aligned");
  if (ld_ir > kConvMaxTaps || R > 65535)
    return fail(VASR_ERR_UNSUPPORTED, "convolve: ld_ir %lld, R %d: at most %lld taps and 65535 responses", (long long)ld_ir, R,
                (long long)kConvMaxTaps);
  launch_convolve(d_in, ld_in, d_len, batch, d_ir_row, d_ir_len, d_spectra, R, ld_ir, d_out, ld_out, d_len_out,
                  static_cast<hipStream_t>(stream));
  return check_launch("convolve");
}

size_t vasr_beam_workspace_bytes(int batch, int64_t frames) {
  // back-pointer rows [B][T][128] u32, then the LM-cache key log [B][T * 128] u64 (beam_wave.hip: eoslog)
  return batch > 0 && frames > 0 ? (size_t)batch * frames * kBeamMax * (sizeof(unsigned int) + sizeof(uint64_t)) : 0;
}

int vasr_beam_workgroups(int batch) {
  if (batch <= 0) return 0;
  if (beam_group_width(batch) > 1) return batch;     // the latency form: a compute unit per utterance (beam_group.hip)
  const int upw = beam_wave_utts_per_workgroup(batch);
  return (batch + upw - 1) / upw;
}

// what both beam-search entry points refuse (pointers: all the caller's buffers are there; the one-best search: nbest 1)
static int check_beam_args(bool pointers, int batch, int64_t frames, int num_classes, int space_id, int beam_width, int nbest,
                           size_t ws_bytes) {
  if (!pointers || batch <= 0 || frames <= 0) return fail(VASR_ERR_INVALID, "bad argument");
  if (num_classes < 2 || num_classes > 128 || beam_width < 1 || beam_width > kBeamMax)
    return fail(VASR_ERR_UNSUPPORTED, "beam search supports 2..128 classes and beam_width 1..%d", kBeamMax);
  if (nbest < 1 || nbest > beam_width) return fail(VASR_ERR_INVALID, "nbest must be 1..beam_width (%d)", beam_width);
  if (space_id < -1 || space_id >= num_classes - 1) return fail(VASR_ERR_INVALID, "space_id out of range");
  const size_t need_bytes = vasr_beam_workspace_bytes(batch, frames);
  if (ws_bytes < need_bytes) return fail(VASR_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, need_bytes);
  return 0;
}

int vasr_beam_search_f32(const float* d_logp, int batch, int64_t frames, int num_classes, int space_id,
                         int beam_width, float token_min_logp, float beam_prune_logp, const vasr_lm* lm,
                         int32_t* d_ids, int32_t* d_id_len, float* d_score, void* d_ws, size_t ws_bytes,
                         vasr_stream stream) {
  return vasr_beam_search_rows_f32(d_logp, nullptr, batch, frames, num_classes, space_id, beam_width, token_min_logp,
                                   beam_prune_logp, lm, d_ids, d_id_len, d_score, d_ws, ws_bytes, stream);
}

int vasr_beam_search_rows_f32(const float* d_logp, const int32_t* d_row_frames, int batch, int64_t frames,
                              int num_classes, int space_id, int beam_width, float token_min_logp,
                              float beam_prune_logp, const vasr_lm* lm, int32_t* d_ids, int32_t* d_id_len,
                              float* d_score, void* d_ws, size_t ws_bytes, vasr_stream stream) {
  if (int rc = check_beam_args(d_logp && d_ids && d_id_len && d_score && d_ws, batch, frames, num_classes, space_id, beam_width, 1,
                               ws_bytes))
    return rc;
  // <= 64 utterances: an utterance on four wavefronts of a compute unit (beam_group.hip: the serving latency, and the shorter
  // stay in the way of an overlapped acoustic pass); beyond that
  // one wavefront per utterance, four utterances per compute unit (beam_wave.hip).  Same bits either way; VASR_BEAM_GROUP
  // (devtools build: 0 | 1 = never, 4 = always the four-wavefront form; anything else aborts) pins the form for A/B runs.
  const int e = launch_beam_search_group(
      d_logp, batch, (int)frames, num_classes, space_id < 0 ? 255 : space_id, beam_width, token_min_logp, beam_prune_logp,
      lm ? &lm->view : nullptr, static_cast<unsigned int*>(d_ws), d_ids, d_id_len, d_score, static_cast<hipStream_t>(stream),
      d_row_frames);
  if (e) return fail(VASR_ERR_HIP, "beam search: %s", hipGetErrorString((hipError_t)e));
  return check_launch("beam_search");
}

int vasr_beam_search_nbest_f32(const float* d_logp, const int32_t* d_row_frames, int batch, int64_t frames,
                               int num_classes, int space_id, int beam_width, int nbest, float token_min_logp,
                               float beam_prune_logp, const vasr_lm* lm, int32_t* d_ids, int32_t* d_id_len,
                               int32_t* d_count, double* d_logit_score, double* d_score, void* d_ws, size_t ws_bytes,
                               vasr_stream stream) {
  if (int rc = check_beam_args(d_logp && d_ids && d_id_len && d_count && d_logit_score && d_score && d_ws, batch, frames, num_classes,
                               space_id, beam_width, nbest, ws_bytes))
    return rc;
  // the same kernel forms as vasr_beam_search_rows_f32, with the n-best final pass
  const BeamNbest nb{nbest, d_count, d_logit_score, d_score};
  const int e = launch_beam_search_group(
      d_logp, batch, (int)frames, num_classes, space_id < 0 ? 255 : space_id, beam_width, token_min_logp, beam_prune_logp,
      lm ? &lm->view : nullptr, static_cast<unsigned int*>(d_ws), d_ids, d_id_len, nullptr, static_cast<hipStream_t>(stream),
      d_row_frames, &nb);
  if (e) return fail(VASR_ERR_HIP, "beam search: %s", hipGetErrorString((hipError_t)e));
  return check_launch("beam_search_nbest");
}

int vasr_lm_create(const void* h_vocab, int vcap, const void* h_ngram, int ncap, const void* h_trie, int trie_buckets,
                   int order, int bos_id, int eos_id, int unk_id, float alpha, float beta, float unk_offset, vasr_lm** out) {
  if (!h_vocab || !h_ngram || !out || vcap <= 0 || ncap <= 0) return fail(VASR_ERR_INVALID, "bad argument");
  if ((vcap & (vcap - 1)) || (ncap & (ncap - 1)) || vcap < 16 || ncap < 16)
    return fail(VASR_ERR_INVALID, "table capacities must be powers of two >= 16");
  if (h_trie && ((trie_buckets & (trie_buckets - 1)) || trie_buckets < 16))
    return fail(VASR_ERR_INVALID, "the trie's bucket count must be a power of two >= 16");
  if (order < 1 || order > 5) return fail(VASR_ERR_UNSUPPORTED, "n-gram order %d (supported: 1..5)", order);
  auto* lm = new vasr_lm();
  void *p0 = nullptr, *p1 = nullptr, *p2 = nullptr;
  hipError_t e = hipMalloc(&p0, (size_t)vcap * 16);
  if (e == hipSuccess) e = hipMalloc(&p1, (size_t)ncap * 16);
  if (e == hipSuccess && h_trie) e = hipMalloc(&p2, (size_t)trie_buckets * 16);
  if (e == hipSuccess) e = hipMemcpy(p0, h_vocab, (size_t)vcap * 16, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p1, h_ngram, (size_t)ncap * 16, hipMemcpyHostToDevice);
  if (e == hipSuccess && h_trie) e = hipMemcpy(p2, h_trie, (size_t)trie_buckets * 16, hipMemcpyHostToDevice);
  lm->allocs = {p0, p1, p2};
  if (e != hipSuccess) {
    vasr_lm_destroy(lm);
    return fail(VASR_ERR_HIP, "uploading the n-gram tables: %s", hipGetErrorString(e));
  }
  lm->view = BeamLm{p0, vcap, p1, ncap, p2, h_trie ? trie_buckets : 0, order, bos_id, eos_id, unk_id, alpha, beta, unk_offset};
  *out = lm;
  return 0;
}

void vasr_lm_destroy(vasr_lm* lm) {
  if (!lm) return;
  for (void* p : lm->allocs) if (p) (void)hipFree(p);
  delete lm;
}

uint64_t vasr_beam_hash_init(void) { return beam_hash_init(); }
uint64_t vasr_beam_hash_step(uint64_t h, uint64_t v) { return beam_hash_step(h, v); }

}  // extern "C"
