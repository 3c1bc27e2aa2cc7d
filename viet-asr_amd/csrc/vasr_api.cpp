// C ABI of libvasr_hip.so (see include/vasr.h): error state, the handle's life (create, weights, setters, finalize), the size
// queries, profiling, and the pipeline entry points.  The model's tables are built in model_build.cpp, the encoder pass runs
// in encoder_run.cpp, the entry points that take no handle are in api_stages.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "vasr_model.h"

using namespace vasr;

namespace {
thread_local std::string g_err;
}

namespace vasr {

thread_local LaunchProbe g_probe;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(VASR_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
  return 0;
}

// How many slices the batch is cut into; slice i runs on its own internal stream so that one slice's
// HBM-bound kernels (depthwise, epilogue stores) overlap another slice's MFMA-bound GEMM main loops.
int n_slices(const vasr_handle* h, int batch) {
  int n = h->slices;
  if (n < 1) n = 1;
  if (n > kMaxSlices) n = kMaxSlices;
  while (n > 1 && batch / n < 8) --n;   // tiny batches: one slice (the kernels would not fill the chip anyway)
  return n;
}

}  // namespace vasr

extern "C" {

const char* vasr_last_error(void) { return g_err.c_str(); }
const char* vasr_version(void) { return "vasr-hip 0.4 (gfx950)"; }
int vasr_abi_version(void) { return VASR_ABI_VERSION; }
int64_t vasr_padded_frames(int64_t frames) { return pad_frames(frames); }

int vasr_create(const vasr_model_desc* d, vasr_handle** out) {
  if (!d || !out) return fail(VASR_ERR_INVALID, "null argument");
  std::unique_ptr<vasr_handle> owner(new vasr_handle());   // freed on every refusal below
  vasr_handle* h = owner.get();
  if (d->frontend) {
    const vasr_frontend_desc& fe = *d->frontend;
    if (fe.n_fft != 512 || fe.n_mels != 64) {
      return fail(VASR_ERR_UNSUPPORTED, "front end supports n_fft=512, n_mels=64 (got %d, %d)", fe.n_fft, fe.n_mels);
    }
    if (fe.win_length <= 0 || fe.win_length > fe.n_fft || fe.hop_length <= 0 || fe.hop_length > 512 ||
        !fe.h_filterbank) {
      // FilterbankFeatures.__init__ raises ValueError for non-positive window sizes (features.py:137-149)
      return fail(VASR_ERR_INVALID, "invalid window/hop/filterbank in front-end description");
    }
    h->has_frontend = true;
    h->fe = fe;
    h->fe_window.resize(fe.win_length);
    for (int i = 0; i < fe.win_length; ++i)
      h->fe_window[i] = fe.h_window ? fe.h_window[i]
                                    : (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * i / (fe.win_length - 1)));
    h->fe_fb.assign(fe.h_filterbank, fe.h_filterbank + (size_t)fe.n_mels * (fe.n_fft / 2 + 1));
    h->fe.h_window = nullptr;
    h->fe.h_filterbank = nullptr;
  }
  if (d->n_blocks > 0) {
    if (!d->blocks || d->feat_in <= 0) return fail(VASR_ERR_INVALID, "encoder needs blocks and feat_in");
    h->has_encoder = true;
    h->feat_in = d->feat_in;
    for (int i = 0; i < d->n_blocks; ++i) {
      const vasr_block_desc& b = d->blocks[i];
      if (b.filters <= 0 || b.repeat <= 0 || b.kernel <= 0 || b.stride <= 0 || b.dilation <= 0) {
        return fail(VASR_ERR_INVALID, "block %d has a non-positive field", i);
      }
      Block B;
      B.d = b;
      h->blocks.push_back(B);
    }
    if (int rc = layout_dense_panes(h)) return rc;
  }
  if (d->num_classes > 0) {
    if (d->dec_feat_in <= 0 || d->num_classes > 128) {
      return fail(VASR_ERR_UNSUPPORTED, "decoder needs dec_feat_in > 0 and at most 128 classes incl. blank");
    }
    h->has_decoder = true;
    h->dec_feat_in = d->dec_feat_in;
    h->num_classes = d->num_classes;
  }
  *out = owner.release();
  return 0;
}

void vasr_destroy(vasr_handle* h) {
  if (!h) return;
  for (void* p : h->dev_allocs) (void)hipFree(p);
  for (auto& r : h->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
  if (h->slice_ready) {
    for (int i = 0; i < kMaxSlices; ++i) { (void)hipStreamDestroy(h->slice_stream[i]); (void)hipEventDestroy(h->slice_done[i]); }
    (void)hipEventDestroy(h->slice_fork);
  }
  delete h;
}

int vasr_load_weight(vasr_handle* h, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!h || !key || (!data && ndim > 0)) return fail(VASR_ERR_INVALID, "null argument");
  if (h->finalized) return fail(VASR_ERR_STATE, "handle already finalized");
  const size_t n = strlen(key);
  if (n >= 19 && strcmp(key + n - 19, "num_batches_tracked") == 0) return 0;
  size_t numel = 1;
  HostTensor t;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] < 0) return fail(VASR_ERR_INVALID, "negative dimension in '%s'", key);
    numel *= (size_t)shape[i];
    t.shape.push_back(shape[i]);
  }
  t.data.assign(data, data + numel);
  h->weights[key] = std::move(t);
  return 0;
}

// the per-block setters' common refusals
static int settable_block(vasr_handle* h, int block) {
  if (!h) return fail(VASR_ERR_INVALID, "null handle");
  if (h->finalized) return fail(VASR_ERR_STATE, "handle already finalized");
  if (block < 0 || block >= (int)h->blocks.size()) return fail(VASR_ERR_INVALID, "block %d of %zu", block, h->blocks.size());
  return 0;
}

int vasr_set_block_se(vasr_handle* h, int block, int reduction_ratio) {
  if (int rc = settable_block(h, block)) return rc;
  if (reduction_ratio < 0) return fail(VASR_ERR_INVALID, "se_reduction_ratio %d is negative", reduction_ratio);
  h->blocks[block].se_r = reduction_ratio;
  return 0;
}

int vasr_set_block_groups(vasr_handle* h, int block, int groups, int heads) {
  if (int rc = settable_block(h, block)) return rc;
  if (groups < 1) return fail(VASR_ERR_INVALID, "groups %d is not positive", groups);
  if (heads == 0 || heads < -1) return fail(VASR_ERR_INVALID, "heads %d: -1 (none) or a positive count", heads);
  h->blocks[block].groups = groups;
  h->blocks[block].heads = heads > 0 ? heads : 0;
  return 0;
}

int vasr_set_block_norm(vasr_handle* h, int block, int norm_groups) {
  if (int rc = settable_block(h, block)) return rc;
  if (norm_groups < 0) return fail(VASR_ERR_INVALID, "norm_groups %d is negative", norm_groups);
  h->blocks[block].norm_g = norm_groups;
  return 0;
}

int vasr_set_activation(vasr_handle* h, int activation, int residual_mode) {
  if (!h) return fail(VASR_ERR_INVALID, "null handle");
  if (h->finalized) return fail(VASR_ERR_STATE, "handle already finalized");
  if (activation < kActRelu || activation > kActSelu)
    return fail(VASR_ERR_INVALID, "activation %d (0 relu, 1 hardtanh, 2 selu)", activation);
  if (residual_mode < 0 || residual_mode > 1) return fail(VASR_ERR_INVALID, "residual_mode %d (0 add, 1 max)", residual_mode);
  h->act = activation;
  h->res_max = residual_mode == 1;
  return 0;
}

int vasr_set_classifier(vasr_handle* h, int feat_in, int num_classes, int pooling) {
  if (!h) return fail(VASR_ERR_INVALID, "null handle");
  if (h->finalized) return fail(VASR_ERR_STATE, "handle already finalized");
  if (h->has_decoder) return fail(VASR_ERR_INVALID, "the handle has a CTC head (dec_feat_in %d): one head per handle", h->dec_feat_in);
  if (pooling < 0 || pooling > 1) return fail(VASR_ERR_INVALID, "pooling %d (0 avg, 1 max)", pooling);
  if (feat_in <= 0 || num_classes <= 0)
    return fail(VASR_ERR_INVALID, "classifier needs feat_in > 0 and num_classes > 0 (got %d, %d)", feat_in, num_classes);
  if (feat_in > kClassifyMaxChannels)
    return fail(VASR_ERR_UNSUPPORTED, "classifier over %d channels (at most %d)", feat_in, kClassifyMaxChannels);
  h->has_classifier = true;
  h->cls_feat_in = feat_in;
  h->cls_classes = num_classes;
  h->cls_pool = pooling;
  return 0;
}

int vasr_finalize(vasr_handle* h) {
  if (!h) return fail(VASR_ERR_INVALID, "null handle");
  if (h->finalized) return 0;
  int rc;
  if (h->has_encoder && (rc = check_encoder(h))) return rc;
  if (h->has_classifier && (rc = check_classifier(h))) return rc;
  if (h->has_frontend && (rc = build_frontend(h))) return rc;
  if (h->has_encoder && (rc = build_encoder(h))) return rc;
  if (h->has_decoder && (rc = build_decoder(h))) return rc;
  if (h->has_classifier && (rc = build_classifier(h))) return rc;
  HIP_TRY(hipDeviceSynchronize());
  {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      h->n_cu = n;
  }
  h->weights.clear();
  h->finalized = true;
  return 0;
}

int64_t vasr_mel_frames(const vasr_handle* h, int64_t samples) {
  const int hop = (h && h->has_frontend) ? h->fe.hop_length : 160;
  return 1 + samples / hop;
}

int64_t vasr_encoded_frames(const vasr_handle* h, int64_t mel_frames) {
  if (!h || !h->has_encoder || !h->finalized) return mel_frames;
  return enc_frames(h, mel_frames);
}

static size_t sliced_workspace_bytes(const vasr_handle* h, int batch, int64_t T);

// what every entry point that runs the STFT refuses: torch.stft's reflect padding of a signal no longer than the pad
static int check_reflect(const vasr_handle* h, int64_t samples) {
  if (samples <= h->fe.n_fft / 2)
    return fail(VASR_ERR_INVALID, "reflect padding needs more than n_fft/2 = %d samples (got %lld)",
                h->fe.n_fft / 2, (long long)samples);
  return 0;
}

// The front end as launches of its own (the per-module entry point, the classification path): seq = ceil(len / hop), the
// STFT / log-mel tiles into mel [B][n_mels][ld], the normalisation.  (The transcribe path folds seq and the encoder's length
// chain into its normalisation launch: transcribe_part.)
static void run_frontend(vasr_handle* h, const float* d_wav, const int64_t* d_len, int batch, int64_t samples, float* mel,
                         int64_t ld, int T, int64_t* seq, hipStream_t st) {
  launch_seq_len(d_len, batch, h->fe.hop_length, seq, st);
  launch_stft_logmel(h->ft, d_wav, false, batch, samples, h->row_independent ? d_len : nullptr, h->fe.hop_length,
                     h->fe.preemph, h->fe.log_guard, mel, ld, T, st);
  launch_normalize(mel, ld, seq, batch, h->fe.n_mels, T, h->fe.normalize == 1, st);
  if (h->fe.normalize == 2) launch_normalize_all(mel, ld, seq, batch, h->fe.n_mels, T, st);
}

size_t vasr_workspace_bytes(const vasr_handle* h, int batch, int64_t samples, int64_t mel_frames) {
  if (!h || !h->finalized || batch <= 0) return 0;
  const int64_t T = samples > 0 ? vasr_mel_frames(h, samples) : mel_frames;
  const size_t whole = plan_ws(h, batch, T).total;
  if (samples > 0 && h->has_frontend && h->has_encoder && h->has_decoder)
    return std::max(whole, sliced_workspace_bytes(h, batch, T));
  return whole;
}

int vasr_melspec_f32(vasr_handle* h, const float* d_wav, const int64_t* d_len, int batch, int64_t samples,
                     float* d_mel, int64_t* d_seq, vasr_stream stream) {
  if (!h || !h->has_frontend || !h->finalized) return fail(VASR_ERR_STATE, "no finalized front end in this handle");
  if (batch <= 0 || !d_wav || !d_len || !d_mel || !d_seq) return fail(VASR_ERR_INVALID, "bad argument");
  if (int rc = check_reflect(h, samples)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int T = (int)vasr_mel_frames(h, samples);
  run_frontend(h, d_wav, d_len, batch, samples, d_mel, T, T, d_seq, st);
  return check_launch("melspec");
}

int vasr_encoder_f32(vasr_handle* h, const float* d_mel, const int64_t* d_seq, int batch, int64_t mel_frames,
                     float* d_enc, float* d_enc_len, void* d_ws, size_t ws_bytes, vasr_stream stream) {
  if (!h || !h->has_encoder || !h->finalized) return fail(VASR_ERR_STATE, "no finalized encoder in this handle");
  if (batch <= 0 || mel_frames <= 0 || !d_mel || !d_seq || !d_enc || !d_ws) return fail(VASR_ERR_INVALID, "bad argument");
  const WsPlan p = plan_ws(h, batch, mel_frames);
  if (ws_bytes < p.total) return fail(VASR_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, p.total);
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(d_ws);
  if (port_input_in_place(h))
    return run_encoder(h, d_mel, mel_frames, mel_frames, d_seq, batch, d_enc, p.T1, d_enc_len, ws, p, st);
  float* melp = reinterpret_cast<float*>(ws + p.melp);
  launch_repad(d_mel, mel_frames, batch * h->feat_in, (int)mel_frames, melp, p.Tp0, st);
  return run_encoder(h, melp, p.Tp0, mel_frames, d_seq, batch, d_enc, p.T1, d_enc_len, ws, p, st);
}

int vasr_decoder_logsoftmax_f32(vasr_handle* h, const float* d_enc, int batch, int64_t enc_frames_, float* d_logp,
                                void* d_ws, size_t ws_bytes, vasr_stream stream) {
  if (!h || !h->has_decoder || !h->finalized) return fail(VASR_ERR_STATE, "no finalized decoder in this handle");
  if (batch <= 0 || enc_frames_ <= 0 || !d_enc || !d_logp || !d_ws) return fail(VASR_ERR_INVALID, "bad argument");
  const int64_t ld = pad_frames(enc_frames_);
  const size_t enc_bytes = align_up((size_t)batch * h->dec_feat_in * ld * 4, 256);
  const size_t need_bytes = enc_bytes + (size_t)batch * h->num_classes * ld * 4;
  if (ws_bytes < need_bytes) return fail(VASR_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, need_bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* encp = static_cast<float*>(d_ws);
  float* logits = reinterpret_cast<float*>(static_cast<char*>(d_ws) + enc_bytes);
  launch_repad(d_enc, enc_frames_, batch * h->dec_feat_in, (int)enc_frames_, encp, ld, st);
  // The fused path's head runs in the fp16-split arithmetic on the maxima the last encoder GEMM published; a port tensor carries
  // none, and rounds 2-5 ran this entry point as 3 x bf16 instead -- same tolerance, other bits: of 181 272 signals 38 came out of
  // the reference-style module-by-module path one character different from the fused row-independent path that promises "what the
  // signal alone gives" (round 6, tests/devtools/fuzz_dag.py).  Now the maxima are taken here, over the same frames, when the
  // caller's workspace has the 1 KB per utterance for them (vasr.h): the two paths give the same bits.
  AmaxTab ax{};
  const size_t amax_off = align_up(need_bytes, 256), amax_bytes = (size_t)batch * 256 * 4;
  if (h->gemm_mode == 3 && ws_bytes >= amax_off + amax_bytes) {
    ax = AmaxTab{reinterpret_cast<unsigned int*>(static_cast<char*>(d_ws) + amax_off), 256, 0};
    launch_amax(encp, ld, h->dec_feat_in, (int)enc_frames_, nullptr, batch, &ax, st);
  }
  return run_decoder(h, encp, ld, enc_frames_, batch, logits, d_logp, nullptr, st, ax);
}

// One contiguous slice of the batch through the whole path on one stream.
// row0: the slice's first row in the whole batch (the feature masks' row_begin is indexed by it).
static int transcribe_part(vasr_handle* h, const void* d_wav, bool pcm16, const int64_t* d_len, int batch, int64_t samples,
                           int64_t* d_pred, int32_t* d_ids, int32_t* d_id_len, float* d_logp, float* d_enc_len,
                           char* ws, hipStream_t st, int row0 = 0) {
  const int64_t T = vasr_mel_frames(h, samples);
  const WsPlan p = plan_ws(h, batch, T);
  int64_t* seq = reinterpret_cast<int64_t*>(ws + p.seq);
  float* melp = reinterpret_cast<float*>(ws + p.melp);
  float* encp = reinterpret_cast<float*>(ws + p.encp);
  float* logits = reinterpret_cast<float*>(ws + p.logits);
  int64_t* pred = d_pred ? d_pred : reinterpret_cast<int64_t*>(ws + p.pred);
  {
    // two launches: the STFT / log-mel tiles, then the per-feature normalisation whose launch also carries (as extra
    // workgroups) seq = ceil(len / hop) and the encoder's length chain -- three launches fewer on the critical path of a
    // batch-1 call than seq_len + stft + normalize + len_chain
    ProfScope ps(h, kProfFrontend, st);
    launch_stft_logmel(h->ft, d_wav, pcm16, batch, samples, h->row_independent ? d_len : nullptr, h->fe.hop_length,
                       h->fe.preemph, h->fe.log_guard, melp, p.Tp0, (int)T, st);
    launch_normalize_chain(melp, p.Tp0, d_len, h->fe.hop_length, batch, h->fe.n_mels, (int)T, h->fe.normalize == 1, seq,
                           h->d_steps, (int)h->steps.size(), reinterpret_cast<int32_t*>(ws + p.lens_tab), d_enc_len,
                           h->row_independent ? d_len : nullptr, (int)p.T1, st);
    if (h->fe.normalize == 2) launch_normalize_all(melp, p.Tp0, seq, batch, h->fe.n_mels, (int)T, st);
  }
  if (h->mask_rects) {
    // vasr_set_feature_masks: one launch that only stores zeros over this slice's rectangles, behind the normalisation (the
    // reference masks the preprocessor's output) and in front of run_encoder, which takes the first layer's operand maxima from
    // the tensor as it then is (launch_amax inside the pass; no kernel in front of it publishes any)
    ProfScope ps(h, kProfFrontend, st);
    launch_spec_mask(melp, p.Tp0, melp, p.Tp0, batch, h->fe.n_mels, (int)T, h->mask_rects, h->mask_row_begin + row0, st);
  }
  AmaxTab enc_amax{};
  const int32_t* own_frames = nullptr;
  int rc = run_encoder(h, melp, p.Tp0, T, seq, batch, encp, p.Tp1, d_enc_len, ws, p, st, &enc_amax, d_len, &own_frames, true);
  if (rc) return rc;
  if ((rc = run_decoder(h, encp, p.Tp1, p.T1, batch, logits, d_logp, pred, st, enc_amax, own_frames))) return rc;
  if (d_ids && d_id_len) {
    ProfScope ps(h, kProfHead, st);
    if (h->row_independent)
      launch_ctc_collapse(pred, batch, p.T1, h->num_classes - 1, d_ids, d_id_len, st, d_len, h->fe.hop_length,
                          h->d_steps, (int)h->steps.size());
    else
      launch_ctc_collapse(pred, batch, p.T1, h->num_classes - 1, d_ids, d_id_len, st);
  }
  return 0;
}

static size_t sliced_workspace_bytes(const vasr_handle* h, int batch, int64_t T) {
  const int n = n_slices(h, batch);
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    const int lo = slice_bounds(batch, i, n), hi = slice_bounds(batch, i + 1, n);
    total += align_up(plan_ws(h, hi - lo, T).total, 256);
  }
  return total;
}

static int transcribe_any(vasr_handle* h, const void* d_wav, bool pcm16, const int64_t* d_len, int batch, int64_t samples,
                          int64_t* d_pred, int32_t* d_ids, int32_t* d_id_len, float* d_logp, float* d_enc_len,
                          void* d_ws, size_t ws_bytes, vasr_stream stream) {
  if (!h || !h->finalized || !h->has_frontend || !h->has_encoder || !h->has_decoder)
    return fail(VASR_ERR_STATE, "handle needs a finalized front end, encoder and decoder");
  if (batch <= 0 || !d_wav || !d_len || !d_ws) return fail(VASR_ERR_INVALID, "bad argument");
  if (int rc = check_reflect(h, samples)) return rc;
  const int64_t T = vasr_mel_frames(h, samples);
  const size_t need_bytes = sliced_workspace_bytes(h, batch, T);
  if (ws_bytes < need_bytes) return fail(VASR_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, need_bytes);
  if (h->mask_rects && !spec_mask_grid_fits(batch, h->fe.n_mels, T))
    return fail(VASR_ERR_UNSUPPORTED, "feature masks: batch %d x %lld frames needs more workgroups than one launch holds", batch,
                (long long)T);
  hipStream_t user = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(d_ws);
  const int n = n_slices(h, batch);
  const int64_t T1 = vasr_encoded_frames(h, T);
  if (n == 1) {
    int rc = transcribe_part(h, d_wav, pcm16, d_len, batch, samples, d_pred, d_ids, d_id_len, d_logp, d_enc_len, ws, user);
    return rc ? rc : check_launch("transcribe");
  }
  if (!h->slice_ready) {
    for (int i = 0; i < kMaxSlices; ++i) {
      HIP_TRY(hipStreamCreateWithFlags(&h->slice_stream[i], hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&h->slice_done[i], hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&h->slice_fork, hipEventDisableTiming));
    h->slice_ready = true;
  }
  HIP_TRY(hipEventRecord(h->slice_fork, user));
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    const int lo = slice_bounds(batch, i, n), hi = slice_bounds(batch, i + 1, n);
    hipStream_t st = h->slice_stream[i];
    HIP_TRY(hipStreamWaitEvent(st, h->slice_fork, 0));
    int rc = transcribe_part(h, static_cast<const char*>(d_wav) + (int64_t)lo * samples * (pcm16 ? 2 : 4), pcm16, d_len + lo, hi - lo, samples,
                             d_pred ? d_pred + (int64_t)lo * T1 : nullptr, d_ids ? d_ids + (int64_t)lo * T1 : nullptr,
                             d_id_len ? d_id_len + lo : nullptr,
                             d_logp ? d_logp + (int64_t)lo * T1 * h->num_classes : nullptr,
                             d_enc_len ? d_enc_len + lo : nullptr, ws + off, st, lo);
    if (rc) return rc;
    off += align_up(plan_ws(h, hi - lo, T).total, 256);
    HIP_TRY(hipEventRecord(h->slice_done[i], st));
    HIP_TRY(hipStreamWaitEvent(user, h->slice_done[i], 0));
  }
  return check_launch("transcribe");
}

int vasr_transcribe_greedy_f32(vasr_handle* h, const float* d_wav, const int64_t* d_len, int batch, int64_t samples,
                               int64_t* d_pred, int32_t* d_ids, int32_t* d_id_len, float* d_logp, float* d_enc_len,
                               void* d_ws, size_t ws_bytes, vasr_stream stream) {
  return transcribe_any(h, d_wav, false, d_len, batch, samples, d_pred, d_ids, d_id_len, d_logp, d_enc_len, d_ws, ws_bytes, stream);
}

int vasr_transcribe_greedy_pcm16(vasr_handle* h, const int16_t* d_pcm, const int64_t* d_len, int batch, int64_t samples,
                                 int64_t* d_pred, int32_t* d_ids, int32_t* d_id_len, float* d_logp, float* d_enc_len,
                                 void* d_ws, size_t ws_bytes, vasr_stream stream) {
  return transcribe_any(h, d_pcm, true, d_len, batch, samples, d_pred, d_ids, d_id_len, d_logp, d_enc_len, d_ws, ws_bytes, stream);
}

// ---- classification path (classify.hip) ----
// pool + linear (+ softmax) over x [B][cls_feat_in][ld]; pooled: [B][cls_feat_in] scratch
static int run_classifier(vasr_handle* h, const float* x, int64_t ld, int64_t frames, int batch, int softmax, float* pooled,
                          float* d_out, hipStream_t st) {
  ProfScope ps(h, kProfHead, st);
  const ClassifyLaunch a{x, ld, batch, h->cls_feat_in, (int)frames, h->cls_classes, h->cls_pool, softmax ? 1 : 0,
                         h->d_cls_w, h->d_cls_b, pooled, d_out};
  const int e = launch_classifier(a, st);
  if (e) return fail(VASR_ERR_HIP, "classifier: %s", hipGetErrorString((hipError_t)e));
  return 0;
}

int vasr_classifier_f32(vasr_handle* h, const float* d_enc, int batch, int64_t enc_frames_, int softmax, float* d_out,
                        void* d_ws, size_t ws_bytes, vasr_stream stream) {
  if (!h || !h->has_classifier || !h->finalized) return fail(VASR_ERR_STATE, "no finalized classifier in this handle");
  if (batch <= 0 || enc_frames_ <= 0 || enc_frames_ > INT32_MAX || !d_enc || !d_out || !d_ws)
    return fail(VASR_ERR_INVALID, "bad argument");
  const size_t need_bytes = (size_t)batch * h->cls_feat_in * 4;
  if (ws_bytes < need_bytes) return fail(VASR_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, need_bytes);
  return run_classifier(h, d_enc, enc_frames_, enc_frames_, batch, softmax, static_cast<float*>(d_ws), d_out,
                        static_cast<hipStream_t>(stream));
}

// vasr_classify_f32's workspace: the encoder's plan over audio_length frames, then the uncropped mel [B][n_mels][pad(T)], its
// lengths [B] i64, the encoder's float lengths [B] and the pooled vectors [B][feat_in]
namespace {
struct ClsPlan { WsPlan enc; size_t mel_raw, seq_raw, enc_len, pooled, total; int64_t T, Tp; };
ClsPlan plan_classify(const vasr_handle* h, int batch, int64_t samples, int64_t audio_length) {
  ClsPlan c{};
  c.enc = plan_ws(h, batch, audio_length);
  c.T = vasr_mel_frames(h, samples);
  c.Tp = pad_frames(c.T);
  size_t o = align_up(c.enc.total, 256);
  auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
  c.mel_raw = take((size_t)batch * h->fe.n_mels * c.Tp * 4);
  c.seq_raw = take((size_t)batch * 8);
  c.enc_len = take((size_t)batch * 4);
  c.pooled = take((size_t)batch * h->cls_feat_in * 4);
  c.total = o;
  return c;
}
}  // namespace

size_t vasr_classify_workspace_bytes(const vasr_handle* h, int batch, int64_t samples, int64_t audio_length) {
  if (!h || !h->finalized || !h->has_frontend || !h->has_encoder || !h->has_classifier || batch <= 0 || samples <= 0 ||
      audio_length <= 0)
    return 0;
  return plan_classify(h, batch, samples, audio_length).total;
}

int vasr_classify_f32(vasr_handle* h, const float* d_wav, const int64_t* d_len, int batch, int64_t samples, int64_t audio_length,
                      const int64_t* d_offsets, int softmax, float* d_out, float* d_mel, void* d_ws, size_t ws_bytes,
                      vasr_stream stream) {
  if (!h || !h->finalized || !h->has_frontend || !h->has_encoder || !h->has_classifier)
    return fail(VASR_ERR_STATE, "handle needs a finalized front end, encoder and classifier");
  if (batch <= 0 || !d_wav || !d_len || !d_out || !d_ws || audio_length <= 0 || audio_length > INT32_MAX)
    return fail(VASR_ERR_INVALID, "bad argument");
  if (int rc = check_reflect(h, samples)) return rc;
  if (h->feat_in != h->fe.n_mels) return fail(VASR_ERR_INVALID, "encoder feat_in %d, front end n_mels %d", h->feat_in, h->fe.n_mels);
  const ClsPlan c = plan_classify(h, batch, samples, audio_length);
  if (c.T > audio_length && !d_offsets)
    return fail(VASR_ERR_INVALID, "%lld mel frames are cropped to %lld: offsets needed", (long long)c.T, (long long)audio_length);
  if (ws_bytes < c.total) return fail(VASR_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, c.total);
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(d_ws);
  const WsPlan& p = c.enc;
  float* mel_raw = reinterpret_cast<float*>(ws + c.mel_raw);
  int64_t* seq_raw = reinterpret_cast<int64_t*>(ws + c.seq_raw);
  int64_t* seq = reinterpret_cast<int64_t*>(ws + p.seq);
  float* melp = reinterpret_cast<float*>(ws + p.melp);
  float* encp = reinterpret_cast<float*>(ws + p.encp);
  {
    ProfScope ps(h, kProfFrontend, st);
    run_frontend(h, d_wav, d_len, batch, samples, mel_raw, c.Tp, (int)c.T, seq_raw, st);
    // cut or centred straight into the encoder's padded-pitch input; every row is audio_length frames long from here on
    const int e = launch_crop_or_pad(mel_raw, c.Tp, batch, h->fe.n_mels, (int)c.T, h->row_independent ? d_len : nullptr,
                                     h->fe.hop_length, (int)audio_length, d_offsets, melp, p.Tp0, (int)p.Tp0, seq, st);
    if (e) return fail(VASR_ERR_HIP, "crop_or_pad: %s", hipGetErrorString((hipError_t)e));
    if (d_mel) launch_repad(melp, p.Tp0, batch * h->fe.n_mels, (int)audio_length, d_mel, audio_length, st);
  }
  int rc = run_encoder(h, melp, p.Tp0, audio_length, seq, batch, encp, p.Tp1, reinterpret_cast<float*>(ws + c.enc_len), ws, p, st);
  if (rc) return rc;
  if ((rc = run_classifier(h, encp, p.Tp1, p.T1, batch, softmax, reinterpret_cast<float*>(ws + c.pooled), d_out, st))) return rc;
  return check_launch("classify");
}

int vasr_set_gemm_mode(vasr_handle* h, int mode) {
  if (!h || mode < 0 || mode > 3)
    return fail(VASR_ERR_INVALID, "gemm mode must be 0 (fp32 MFMA), 1 (3 x bf16 split), 2 (2 x bf16 split, reduced) or "
                                  "3 (2 x fp16 scaled split)");
  h->gemm_mode = mode;
  return 0;
}

int vasr_get_gemm_mode(const vasr_handle* h) { return h ? h->gemm_mode : -1; }

int vasr_set_busy_cus(vasr_handle* h, int cus) {
  if (!h || cus < 0) return fail(VASR_ERR_INVALID, "busy compute units must be >= 0");
  h->busy_cus = cus;
  return 0;
}

int vasr_set_row_independent(vasr_handle* h, int on) {
  if (!h) return fail(VASR_ERR_INVALID, "null handle");
  h->row_independent = on != 0;
  return 0;
}

int vasr_set_feature_masks(vasr_handle* h, const int32_t* d_rects, const int32_t* d_row_begin) {
  if (!h) return fail(VASR_ERR_INVALID, "null handle");
  if ((d_rects == nullptr) != (d_row_begin == nullptr))
    return fail(VASR_ERR_INVALID, "feature masks: d_rects and d_row_begin are set together, or both NULL to clear");
  h->mask_rects = d_rects;
  h->mask_row_begin = d_row_begin;
  return 0;
}

int vasr_set_slices(vasr_handle* h, int slices) {
  if (!h || slices < 1 || slices > kMaxSlices) return fail(VASR_ERR_INVALID, "slices must be 1..%d", kMaxSlices);
  h->slices = slices;
  return 0;
}

int vasr_profile_begin(vasr_handle* h) {
  if (!h) return fail(VASR_ERR_INVALID, "null handle");
  for (auto& r : h->prof) { h->ev_pool.push_back(r.a); h->ev_pool.push_back(r.b); }
  h->prof.clear();
  h->profiling = true;
  return 0;
}

int vasr_profile_end(vasr_handle* h, double ms[5], int64_t launches[5], double flops[5], double bytes[5]) {
  if (!h || !ms || !launches) return fail(VASR_ERR_INVALID, "bad argument");
  h->profiling = false;
  for (int i = 0; i < 5; ++i) { ms[i] = 0.0; launches[i] = 0; if (flops) flops[i] = 0.0; if (bytes) bytes[i] = 0.0; }
  for (auto& r : h->prof) {
    HIP_TRY(hipEventSynchronize(r.b));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
    ms[r.cls] += t;
    launches[r.cls] += 1;
    if (flops) flops[r.cls] += r.flops;
    if (bytes) bytes[r.cls] += r.bytes;
    h->ev_pool.push_back(r.a);
    h->ev_pool.push_back(r.b);
  }
  h->prof.clear();
  return 0;
}

int vasr_algorithmic_work(const vasr_handle* h, int batch, int64_t samples, double out[5]) {
  if (!h || !h->finalized || !out) return fail(VASR_ERR_INVALID, "bad argument");
  for (int i = 0; i < 5; ++i) out[i] = 0.0;
  int64_t T = vasr_mel_frames(h, samples);
  if (h->has_frontend) {
    const double per_frame = 2.5 * 512 * 9 + 2.0 * 257 + 2.0 * 64 * 23;
    out[4] = per_frame * (double)T * batch;
  }
  int64_t t = T;
  for (const Block& B : h->blocks) {
    const int64_t t_in = t;
    for (const SubBlock& S : B.subs) {
      if (S.separable) {
        const int64_t to = conv_out_frames(t, S.dw);
        out[1] += 2.0 * S.dw.kernel * S.dw.cin * (double)to * batch;
        out[2] += 4.0 * ((double)S.dw.cin * t + (double)S.dw.cin * to) * batch + 4.0 * S.dw.cin * S.dw.kernel;
        t = to;
      } else {
        t = conv_out_frames(t, S.pw);
      }
      out[0] += 2.0 * S.pw.cin * S.pw.cout * (double)t * batch;
    }
    // (a folded residual's GEMM counts as its own; the per-pane GEMMs of a dense residual have never been counted)
    if (B.res.size() == 1) out[0] += 2.0 * B.res[0].w.cin * B.res[0].w.cout * (double)t_in * batch;
  }
  if (h->has_decoder) out[3] = 2.0 * h->dec_feat_in * h->num_classes * (double)t * batch;
  return 0;
}

}  // extern "C"
