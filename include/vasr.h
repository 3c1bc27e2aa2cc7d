/*
 * vasr.h -- C ABI of libvasr_hip.so: the MI355X (gfx950) implementation of the
 * viet-asr infer.py hot path.
 *
 * Nothing like this exists in the reference (it is Python on ATen ops only); each entry
 * point below names the reference interface whose arithmetic it replaces, paths under
 * /root/reference.  The boundary carries plain pointers, sizes and a hipStream_t: no torch
 * types.  The library never allocates or frees caller-visible result buffers; weights are
 * copied into a library-owned handle at vasr_load_weight()/vasr_finalize().
 *
 * All pointers named d_* are DEVICE pointers (HBM); h_* are HOST pointers.
 * All functions return 0 on success or a negative vasr_status; vasr_last_error() gives a
 * thread-local human readable message for the last failure.
 * Re-entrancy: calls on distinct handles, or on one handle with distinct workspaces and
 * streams, may run concurrently; there is no global mutable state besides the error string.
 * Round 6 made that true ON THE DEVICE as well: next to 16-bit matrix kernels of another stream -- a second handle of this
 * library, or anybody else's GEMM -- packed-FP32 and FP64 vector arithmetic of a small kernel returned wrong values on MI355X
 * (profiles/r06_concurrency.txt); the front end no longer contains the first and runs the second alone on its compute unit.
 * tests/devtools/stress_attack.py and stress_threads.py are the harnesses: every entry point next to torch's fp16 bmm, and
 * N host threads on N streams, each result against the idle-device one bit for bit.
 */
#ifndef VASR_H_
#define VASR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions marked VASR_API are its ONLY dynamic symbols. */
#if defined(__GNUC__) || defined(__clang__)
#define VASR_API __attribute__((visibility("default")))
#else
#define VASR_API
#endif

/* Binary interface number of this header; vasr_abi_version() returns the one the library was built from.  Bumped whenever
 * a signature or struct layout changes (4: vasr_profile_end reports five kernel classes with flops / bytes per class --
 * a caller built against the four-class form would be written past its arrays; 5: vasr_lm_create takes 16-byte table
 * entries with power-of-two capacities; 6: vasr_lm_create takes the character trie of pyctcdecode's unigram set, the
 * vocabulary entries carry a set-membership flag, vasr_resample_f32 emits ceil(len * ratio) samples,
 * vasr_frontend_desc ends in log_guard_clamp and knows normalize = 2; 7: + vasr_transcribe_greedy_pcm16; 8: vasr_block_desc
 * ends in residual_dense, and non-separable blocks take any kernel / stride / dilation). */
#define VASR_ABI_VERSION 8

typedef struct vasr_handle vasr_handle;
typedef void* vasr_stream; /* hipStream_t */

typedef enum {
  VASR_OK = 0,
  VASR_ERR_INVALID = -1,     /* bad argument (Python side raises ValueError) */
  VASR_ERR_STATE = -2,       /* call order: weight missing, not finalized ... */
  VASR_ERR_HIP = -3,         /* HIP runtime failure */
  VASR_ERR_WORKSPACE = -4,   /* workspace too small */
  VASR_ERR_UNSUPPORTED = -5  /* configuration the kernels do not cover */
} vasr_status;

/* One JasperBlock (nemo/collections/asr/parts/jasper.py:175-288), as the YAML spells it
 * (configs/quartznet12x1_vi.yaml:25-165).  A non-separable block of kernel > 1 (Jasper) runs as an implicit GEMM over
 * (tap, input channel) and needs an input channel count that is a multiple of 64. */
typedef struct {
  int32_t filters;
  int32_t repeat;
  int32_t kernel;
  int32_t stride;
  int32_t dilation;
  int32_t residual;  /* 0/1 */
  int32_t separable; /* 0/1 */
  int32_t residual_dense; /* 0/1: JasperEncoder's residual_dense (jasper.py:152-161, parts/jasper.py:264-288, :428-448): the
                             residual sums a 1x1 conv + BN of every pane -- the block input and the outputs of the earlier
                             blocks of the contiguous dense run (the encoder input when the run starts at block 0); weights
                             encoder.{i}.res.{p}.{0.conv.weight,1.*}.  vasr_create refuses the layouts the reference cannot
                             run: a dense block after a non-dense one that followed a dense run, a dense block without
                             residual followed by a dense block, a strided dense block with residual.  (ABI 8: appended) */
} vasr_block_desc;

/* Front end = FilterbankFeatures.__init__ (parts/features.py:113-236) with the knobs the
 * path uses: dither 0, pad_to 0 (infer.py:89-90), stft_conv false, mag_power 2, frame_splicing 1; log guard "add" or
 * "clamp" (:269-274), normalisation per_feature, all_features or none (:17-46). */
typedef struct {
  int32_t sample_rate;  /* 16000 */
  int32_t n_fft;        /* 512 (only 512 is implemented) */
  int32_t win_length;   /* 320 */
  int32_t hop_length;   /* 160 */
  int32_t n_mels;       /* 64 (only 64 is implemented) */
  float preemph;        /* 0.97; <0 disables */
  float log_guard;      /* 2^-24 */
  int32_t normalize;    /* 1 = per_feature (per utterance and mel bin), 2 = all_features (one mean / std per utterance over
                           every bin and frame, features.py:31-39), 0 = none */
  const float* h_window;     /* [win_length] or NULL -> symmetric hann */
  const float* h_filterbank; /* [n_mels][n_fft/2+1] row-major, REQUIRED */
  int32_t log_guard_clamp;   /* 0 = log(x + log_guard) (log_zero_guard_type "add", the shipped configs), 1 = log(max(x,
                                log_guard)) ("clamp", features.py:272-273).  (ABI 6: appended) */
} vasr_frontend_desc;

typedef struct {
  const vasr_frontend_desc* frontend; /* NULL -> handle has no front end */
  int32_t feat_in;                    /* encoder input channels (64) */
  int32_t n_blocks;                   /* 0 -> handle has no encoder */
  const vasr_block_desc* blocks;
  int32_t dec_feat_in;                /* 1024; 0 -> handle has no CTC head */
  int32_t num_classes;                /* V+1, blank = V is the last class */
} vasr_model_desc;

/* ---- life cycle ------------------------------------------------------------------- */
VASR_API int vasr_create(const vasr_model_desc* desc, vasr_handle** out);
VASR_API void vasr_destroy(vasr_handle* h);

/* Replaces TrainableNM.restore_from -> load_state_dict (nemo/backends/pytorch/nm.py:97-103):
 * feed every float tensor of the module state_dict under its reference key, e.g.
 * "encoder.3.mconv.1.conv.weight", "encoder.3.mconv.2.running_var",
 * "encoder.3.res.0.0.conv.weight", "decoder_layers.0.bias".
 * Keys ending in "num_batches_tracked" are accepted and ignored. */
VASR_API int vasr_load_weight(vasr_handle* h, const char* key, const float* h_data, const int64_t* shape, int ndim);

/* JasperBlock's se / se_reduction_ratio (parts/jasper.py:152-168, :223-253) for block `block`: reduction_ratio 0 = no SE (the
 * default), else SqueezeExcite(filters, reduction_ratio) -- y = x * sigmoid(W2 relu(W1 mean_t(x))), W1 [filters / r][filters],
 * W2 [filters][filters / r], no bias -- where the reference puts it: with residual, on every residual pane's branch after its
 * BN (weights encoder.{i}.res.{p}.2.fc.{0,2}.weight); without, after every sub-layer (after its activation, except the last
 * one's: after its BN, before the block's output activation), weights encoder.{i}.mconv.{j}.fc.{0,2}.weight with the mconv
 * indices of the reference's ModuleList (each SE entry shifts the ones behind it).  Between vasr_create and vasr_finalize.
 * vasr_finalize refuses filters / r == 0 (VASR_ERR_INVALID), filters > 1024 (VASR_ERR_UNSUPPORTED) and missing SE weights
 * (VASR_ERR_STATE).  The one deliberate difference: the time mean is taken over each row's OWN frames at that layer (sum over
 * t < len_b, divided by len_b), not over the padded tensor width as nn.AdaptiveAvgPool1d does -- equal whenever the row is as
 * long as the tensor (every batch-1 call with pad_to = 0, the longest row of a batch), and what keeps a row's result
 * independent of its batch.  (ABI 8: a function, no layout change.) */
VASR_API int vasr_set_block_se(vasr_handle* h, int block, int reduction_ratio);

/* JasperBlock's groups / heads (parts/jasper.py:70-150, :329-400) for block `block`; groups 1 and heads -1 are the defaults.
 * groups = G > 1: every main-branch conv of the block -- the 1x1 after each depthwise conv of a separable block, the K-tap (or
 * 1x1) conv of a non-separable one -- is grouped, weight [filters][C_in / G][K], and followed (after its BN) by the
 * reference's GroupShuffle: output channel j * G + g holds pre-shuffle channel g * (filters / G) + j.  The shuffle is its own
 * ModuleList entry, so every later mconv index (and SE entry) moves by one per sub-layer.  Residual branches, dense panes
 * included, are never grouped; they are added after the shuffle.  heads = H > 0: the depthwise weight of a separable block is
 * [H][1][K] and channel c uses row c % H; on a block that is not separable heads is ignored, as the reference ignores it
 * there (it never hands heads to a non-separable conv).  Between vasr_create and vasr_finalize.  vasr_finalize refuses,
 * before it touches a device, groups that do not divide a sub-layer's in- and out-channels and C % heads != 0
 * (VASR_ERR_INVALID), a grouped block whose filters are not a multiple of 128 (VASR_ERR_UNSUPPORTED, the rule for every
 * block), and a grouped or shared conv weight that is missing (VASR_ERR_STATE) or not of the exact shape above
 * (VASR_ERR_INVALID).  What runs where: in the split arithmetics (f16x2, bf16x3, bf16x2) a grouped layer whose per-group
 * widths filters / G and C_in / G are multiples of 64 runs the grouped split GEMM (encoder_pw_split.hip: one workgroup per
 * tile of one group, K = taps * C_in / G, the shuffle applied in its store).  Narrower groups -- e.g. a first block reading the 64 mel
 * features at G >= 2 -- and every grouped layer in the fp32 mode run the dense kernels on the block-diagonal form of the
 * weight (rows and BN permuted by the shuffle).  Grouped blocks never take the fused depthwise + pointwise kernel or the folded
 * dual-source residual GEMM.  (ABI 8: a function, no layout change.) */
VASR_API int vasr_set_block_groups(vasr_handle* h, int block, int groups, int heads);

/* JasperEncoder's normalization_mode / norm_groups (jasper.py:136-186, parts/jasper.py:385-391) for block `block`:
 * norm_groups 0 = eval-mode BatchNorm1d(eps=1e-3) (the default, folded into the GEMM epilogues), G > 0 = nn.GroupNorm(G,
 * filters) after every conv of the block -- "group" with norm_groups (-1: filters), "instance" = G filters, "layer" = G 1.
 * GroupNorm: y = gamma[c] * (x - mean) / sqrt(var + 1e-5) + beta[c], mean and the BIASED variance per utterance and norm
 * group (filters / G consecutive channels, counted before a grouped block's GroupShuffle), weights <prefix>.weight /
 * <prefix>.bias [filters] at the BatchNorm's keys (no running statistics).  Order as in the reference: conv -> norm ->
 * GroupShuffle -> activation (not on the last sub-layer) -> SE; each residual pane conv -> norm (-> SE), its own pass; the
 * block output act(main + sum of the panes).  Between vasr_create and vasr_finalize.  vasr_finalize refuses, before it
 * touches a device, a G that does not divide filters and a gamma / beta that is missing or not of shape [filters]
 * (VASR_ERR_INVALID).  The one deliberate difference: the statistics are taken over each row's OWN frames at that layer
 * (t < len_b), not over the padded tensor width as nn.GroupNorm does -- equal whenever the row is as long as the tensor
 * (every batch-1 call with pad_to = 0 whose length is not a multiple of the hop), and what keeps a row's result independent
 * of its batch.  Normalized blocks store their convs' raw outputs and take two device passes per norm (statistics, apply;
 * encoder_norm.hip); they never take the fused depthwise + pointwise kernel or a folded residual.  (ABI 8: a function, no
 * layout change.) */
VASR_API int vasr_set_block_norm(vasr_handle* h, int block, int norm_groups);

/* JasperEncoder's activation and residual_mode (jasper.py:136-190, parts/jasper.py:21-25, :428-448), one setting for the
 * whole encoder as in the reference, which builds ONE activation module and hands it to every block.  activation: 0 = ReLU
 * (the default), 1 = nn.Hardtanh() with its defaults, clamp(x, -1, 1), 2 = nn.SELU(): lambda * x for x > 0, else
 * lambda * alpha * expm1(x), lambda = 1.0507009873554804934193349852946, alpha = 1.6732632423543772848170429916717.  It
 * takes the place of ReLU everywhere the block applies one: after every sub-layer but the last (conv -> norm -> [shuffle]
 * -> act -> [SE]) and on the block output act(combine(main, residual panes)).  SqueezeExcite's inner ReLU stays a ReLU
 * whatever the activation (parts/jasper.py:152-168).  residual_mode: 0 = "add" (the default), out + res_p for each pane
 * in turn; 1 = max, out = max(out, res_p) -- the reference treats every residual_mode other than "add" so, and the Python
 * layer maps them here.  Max is taken with fmaxf: a NaN operand yields the other one (torch.max propagates NaN); the two
 * agree wherever no NaN is present.  Between vasr_create and vasr_finalize.  Codes out of range: VASR_ERR_INVALID.
 * vasr_finalize refuses residual_mode max together with any GroupNorm block (vasr_set_block_norm) with
 * VASR_ERR_UNSUPPORTED, before it touches a device.  What runs where: a max residual is never folded into the main GEMM
 * (its residual GEMM stores R and the main GEMM's epilogue takes the maximum), and a dense residual runs one GEMM per pane,
 * each combined into R by max.  Non-ReLU activations and max residuals take epilogue variants of the same kernels; ReLU / add
 * models run exactly the kernels they ran before.  (ABI 8: a function, no layout change.) */
VASR_API int vasr_set_activation(vasr_handle* h, int activation, int residual_mode);

/* JasperDecoderForClassification (jasper.py:257-319) as the handle's head, in place of a CTC head: the handle is created with
 * dec_feat_in = 0 and num_classes = 0.  pooling 0 = 'avg' (nn.AdaptiveAvgPool1d(1)), 1 = 'max' (nn.AdaptiveMaxPool1d(1)); the
 * weights arrive through vasr_load_weight under the reference's keys, decoder_layers.0.weight [num_classes][feat_in] (2-D: an
 * nn.Linear) and decoder_layers.0.bias [num_classes].  Between vasr_create and vasr_finalize.  Refused here: a CTC head on the
 * same handle, a pooling code out of range, feat_in or num_classes <= 0 (VASR_ERR_INVALID), feat_in > 1024
 * (VASR_ERR_UNSUPPORTED).  vasr_finalize refuses, before it touches a device, a feat_in that is not the encoder's output width
 * and a weight of any other shape (VASR_ERR_INVALID) and a missing weight (VASR_ERR_STATE).
 * The pool is taken over the WIDTH OF THE TENSOR AS HANDED IN -- all T' frames of every row, as the reference's forward does,
 * which takes no lengths; after CropOrPadSpectrogramAugmentation every row is audio_length frames long anyway.  This differs
 * from vasr_set_block_se, whose time mean is over each row's own frames.  Never over the columns between T' and the
 * 128-frame pitch of an internal buffer (vasr_padded_frames).  The maximum is taken with fmaxf: a NaN frame is skipped
 * (nn.AdaptiveMaxPool1d propagates it); the two agree wherever no NaN is present.  Every sum has one fixed order that depends
 * on (feat_in, T') alone and there are no atomics: a row's output bits are the same whatever else is in the batch.
 * (ABI 8: a function, no layout change.) */
VASR_API int vasr_set_classifier(vasr_handle* h, int feat_in, int num_classes, int pooling);

/* Checks that every tensor arrived, folds eval-mode BatchNorm1d(eps=1e-3)
 * (parts/jasper.py:392) into per-channel (scale, shift), packs the 1x1-conv weights
 * K-major for the MFMA kernels and uploads everything.  Needed before any compute call. */
VASR_API int vasr_finalize(vasr_handle* h);

/* ---- shapes ------------------------------------------------------------------------ */
/* T = 1 + L / hop (torch.stft center=True, parts/features.py:181-188). */
VASR_API int64_t vasr_mel_frames(const vasr_handle* h, int64_t samples);
/* T' after every strided block: floor((T + 2p - d(K-1) - 1)/s) + 1 (parts/jasper.py:108-111). */
VASR_API int64_t vasr_encoded_frames(const vasr_handle* h, int64_t mel_frames);
/* Scratch needed by vasr_encoder_f32 / vasr_decoder_* / vasr_transcribe_greedy_f32 for a
 * batch of B utterances padded to `samples` (or, if samples == 0, to mel_frames). */
VASR_API size_t vasr_workspace_bytes(const vasr_handle* h, int batch, int64_t samples, int64_t mel_frames);

/* ---- the path, stage by stage (each = one NeuralModule forward) ---------------------- */

/* AudioToMelSpectrogramPreprocessor.forward == FilterbankFeatures.forward
 * (audio_preprocessing.py:78-87, parts/features.py:245-301).
 *   d_wav [B][L] f32 (rows zero padded), d_len [B] i64
 *   -> d_mel [B][n_mels][T] f32 contiguous, d_seq [B] i64 = ceil(len/hop) */
VASR_API int vasr_melspec_f32(vasr_handle* h, const float* d_wav, const int64_t* d_len, int batch, int64_t samples,
                     float* d_mel, int64_t* d_seq, vasr_stream stream);

/* JasperEncoder.forward (jasper.py:198-204; JasperBlock.forward parts/jasper.py:408-448;
 * MaskedConv1d.forward parts/jasper.py:113-132).
 *   d_mel [B][feat_in][T] f32 contiguous, d_seq [B] i64
 *   -> d_enc [B][C_last][T'] f32 contiguous, d_enc_len [B] f32 (quirk Q3: float lengths) */
VASR_API int vasr_encoder_f32(vasr_handle* h, const float* d_mel, const int64_t* d_seq, int batch, int64_t mel_frames,
                     float* d_enc, float* d_enc_len, void* d_workspace, size_t workspace_bytes,
                     vasr_stream stream);

/* JasperDecoderForCTC.forward (jasper.py:253-254): conv1x1+bias -> transpose -> log_softmax.
 *   d_enc [B][dec_feat_in][T'] f32 contiguous -> d_logp [B][T'][V+1] f32
 * Workspace: align256(B * dec_feat_in * ld * 4) + B * (V+1) * ld * 4 bytes with ld = vasr_padded_frames(T'); with
 * align256(that) + B * 1024 bytes the maxima of the port tensor are taken first and the head GEMM runs in the handle's GEMM mode
 * like the fused path's (the same bits as vasr_transcribe_greedy_f32 on the same encoder output); with less, mode 3 falls back
 * to the 3 x bf16 form (same tolerance). */
VASR_API int vasr_decoder_logsoftmax_f32(vasr_handle* h, const float* d_enc, int batch, int64_t enc_frames,
                                float* d_logp, void* d_workspace, size_t workspace_bytes, vasr_stream stream);

/* GreedyCTCDecoder.forward (greedy_ctc_decoder.py:33-36): argmax(-1), first max wins.
 *   d_logp [B][T'][V+1] f32 -> d_pred [B][T'] i64 */
VASR_API int vasr_greedy_argmax(const float* d_logp, int batch, int64_t frames, int num_classes, int64_t* d_pred,
                       vasr_stream stream);

/* __ctc_decoder_predictions_tensor inner loop (helpers.py:20-31): drop repeats and blanks over
 * ALL frames (quirk Q4).  d_pred [B][T'] i64 -> d_ids [B][T'] i32 (compacted), d_id_len [B] i32 */
VASR_API int vasr_ctc_collapse(const int64_t* d_pred, int batch, int64_t frames, int blank_id, int32_t* d_ids,
                      int32_t* d_id_len, vasr_stream stream);

/* word_error_rate (nemo/collections/asr/metrics.py:30-63), both use_cer settings, per row, on device ids.
 *   d_hyp [B][hyp_width] i32, d_hyp_len [B] i32 (d_ids / d_id_len of the calls below and of the beam search),
 *   d_ref [B][ref_width] i32, d_ref_len [B] i32 (the data layer's transcripts / transcript_length)
 *   -> d_counts [B][4] i32 = {word_edits, ref_words, char_edits, ref_chars}, 16-byte aligned (one vector store per row).
 * Characters: the Levenshtein distance (unit costs, metrics.py:7-27) between the two id rows over their own lengths,
 * whitespace ids included -- list(h) against list(r); ref_chars = the reference's length.  Words: the same distance between the
 * rows' words -- h.split() against r.split(): a word is a maximal run of ids that are not among h_space_ids (host, n_space ids,
 * 0..8: every label for which str.isspace() holds), so leading, trailing and repeated whitespace make no empty words, a row
 * of whitespace has none, and with n_space = 0 a non-empty row is one word.  Two words are equal iff their id runs are equal:
 * a 64-bit fold (vasr_beam_hash_step) only prefilters, equal folds are confirmed id by id.  Integer arithmetic throughout.
 * A row's counts depend on that row alone -- not on the batch, the other rows or the ids behind its lengths, which are never
 * read.  Lengths are clamped into [0, width]; a NEGATIVE length on either side (the beam search's id_len = -1 overflow
 * report) gives {-1, -1, -1, -1} for that row, never a plausible number.  A width of 0 is legal (the distance to an empty side
 * is the other side's length); widths above 4096 return VASR_ERR_UNSUPPORTED before anything is launched; NULL pointers,
 * batch <= 0, a width < 0, n_space outside 0..8 and a misaligned d_counts return VASR_ERR_INVALID before a device is touched.
 * No handle, no workspace: one workgroup per row, everything in LDS (133 KB at 4096 x 4096, where ONE row takes about
 * 10.0 ms -- the rows of a batch run side by side; DESIGN section 7c has the measured times).  (ABI 8) */
VASR_API int vasr_error_counts_i32(const int32_t* d_hyp, int64_t hyp_width, const int32_t* d_hyp_len,
                                   const int32_t* d_ref, int64_t ref_width, const int32_t* d_ref_len, int batch,
                                   const int32_t* h_space_ids, int n_space,   /* host, 0..8 ids */
                                   int32_t* d_counts /* [B][4] */, vasr_stream stream);

/* The alignment rule.  vasr_error_ops_i32 splits the distance above into substitutions, deletions and insertions; the sum is
 * unique, the split is not (other tools break ties differently), so the rule is part of the interface.  For a hypothesis
 * h[0..n) and a reference r[0..m), unit costs:
 *   borders:   D[i][0] = i (every hypothesis element there is an insertion), D[0][j] = j (every reference element a deletion);
 *   interior:  diag = D[i-1][j-1] + (h[i-1] != r[j-1]),
 *              dele = D[i][j-1] + 1   (reference element j has no partner),
 *              ins  = D[i-1][j] + 1   (hypothesis element i has no partner);
 *   tie-break: the cell's predecessor is diag if diag <= min(dele, ins), otherwise dele if dele <= ins, otherwise ins;
 *   the alignment is the one path from (n, m) back to (0, 0) along those predecessors; a diagonal step is a hit if the two
 *   elements are equal and a substitution if not.
 * A cell's predecessor depends on its three neighbours' costs alone, so the path is the same in whatever order the cells are
 * computed (the kernel walks anti-diagonals).  hits + sub + del = m, hits + sub + ins = n, sub + del + ins = D[n][m].
 *
 * vasr_error_ops_i32: inputs, word and character semantics, clamping and refusals of vasr_error_counts_i32
 *   -> d_ops_counts [B][8] i32 = {word_sub, word_del, word_ins, word_hits, char_sub, char_del, char_ins, char_hits}, 16-byte
 *      aligned (two vector stores per row); eight -1 for a row with a negative length on either side;
 *   -> optionally the WORD-level edit script: d_script [B][L] i32 and d_script_len [B] i32, both or neither, with
 *      L = (hyp_width + 1) / 2 + (ref_width + 1) / 2 (a word needs a separator: no alignment of the rows' words is longer).
 *      d_script[b][0 .. len) is the alignment from the first word to the last as op codes 0 = hit, 1 = substitution,
 *      2 = deletion, 3 = insertion; word indices are implied: a hit or a substitution consumes one word of each side, a deletion
 *      one reference word, an insertion one hypothesis word.  Entries at or beyond len are not written; a -1 row gets
 *      d_script_len = -1.  The script's op counts equal the row's four word counts.
 * Counts alone take widths up to 4096 in the LDS vasr_error_counts_i32 takes (a cell carries its cost and its path's
 * substitutions in one word; deletions - insertions = j - i on every path into (i, j)).  A script keeps the predecessor of
 * every word cell, 2 bits each, in LDS: both widths must then be <= 1024 (512 words per side, about 66 KB of bits, 98 KB in
 * all); wider requests return VASR_ERR_UNSUPPORTED with the limit in vasr_last_error().  One script pointer without the other
 * returns VASR_ERR_INVALID.  All refusals come before a device is touched.  No handle, no workspace, no atomics, integers only:
 * one workgroup per row, and a row's outputs do not depend on the batch it sits in.  (ABI 8) */
VASR_API int vasr_error_ops_i32(const int32_t* d_hyp, int64_t hyp_width, const int32_t* d_hyp_len,
                                const int32_t* d_ref, int64_t ref_width, const int32_t* d_ref_len, int batch,
                                const int32_t* h_space_ids, int n_space,   /* host, 0..8 ids */
                                int32_t* d_ops_counts /* [B][8] */, int32_t* d_script /* [B][L] or NULL */,
                                int32_t* d_script_len /* [B] or NULL */, vasr_stream stream);

/* vasr_error_counts_i32 of every hypothesis of an n-best list against the row's ONE reference, and the oracle: the best slot
 * per row.  Inputs as vasr_beam_search_nbest_f32 writes them:
 *   d_ids [B][nbest][width] i32, d_id_len [B][nbest] i32, d_count [B] i32 (slots filled; clamped to nbest),
 *   d_ref [B][ref_width] i32, d_ref_len [B] i32 -- row b serves all its slots, it is not replicated in memory
 *   -> d_slot_counts [B][nbest][4] i32 (required, 16-byte aligned): vasr_error_counts_i32's four numbers of every filled slot,
 *      four -1 in slots at or beyond d_count[b];
 *   -> d_counts [B][4] i32 (may be NULL; 16-byte aligned) = {min word_edits, ref_words, min char_edits, ref_chars}: the two
 *      minima are taken independently over the FILLED slots only (an unfilled slot has length 0 and never wins, even where
 *      the empty string would beat every hypothesis); the layout is vasr_error_counts_i32's and accumulates the same way;
 *   -> d_slot [B][2] i32 (may be NULL): the slot of the word minimum and of the character minimum, the lower slot among equals.
 * A row with a negative d_id_len in a filled slot (the search's overflow report), a negative d_ref_len or d_count < 1 gives
 * -1 in every output of that row.  Refusals as vasr_error_counts_i32, plus nbest < 1 (VASR_ERR_INVALID) and nbest > 65535
 * (VASR_ERR_UNSUPPORTED; the beam search returns at most 128).  B x nbest
 * workgroups, then one wavefront per row for the minima in a fixed order: no atomics, no workspace.  (ABI 8) */
VASR_API int vasr_nbest_error_counts_i32(const int32_t* d_ids, int64_t width, const int32_t* d_id_len,
                                         const int32_t* d_count, int nbest, const int32_t* d_ref, int64_t ref_width,
                                         const int32_t* d_ref_len, int batch, const int32_t* h_space_ids, int n_space,
                                         int32_t* d_slot_counts /* [B][nbest][4] */, int32_t* d_counts /* [B][4] or NULL */,
                                         int32_t* d_slot /* [B][2] or NULL */, vasr_stream stream);

/* Scores of classification logits, per row: metrics.classification_accuracy (nemo/collections/asr/metrics.py:66-99) for
 * every k at once, nn.CrossEntropyLoss(reduction='none') as CrossEntropyLossNM calls it, and the top-k classes.
 *   d_logits [B][num_classes] f32 contiguous; d_targets [B] i64 or NULL; k: 0, or 1..16 with k <= num_classes
 *   -> d_topk_idx [B][k] i32, d_topk_val [B][k] f32, d_topk_prob [B][k] f32; d_rank [B] i32, d_loss [B] f32 (both need
 *      d_targets).  Every output may be NULL.
 * ONE total order on a row's classes: the larger value first; a NaN ranks above every number (as torch.topk orders it);
 * -0 equals +0; among equal values, and among NaNs, the LOWER class index comes first.  torch.topk leaves the order of
 * equal values unspecified ([1,3,3,2,3].topk(3) returns the indices 2,4,1 on the CPU): the tie rule is this library's own,
 * and on a row with ties among its first k values or at its target the reference's own answer is not defined.
 *   d_topk_idx / d_topk_val: the first k classes of that order and their logits (copies, bit-equal to the input);
 *   d_topk_prob: expf(x - logsumexp(row)), the softmax probability of each of them;
 *   d_rank[b]: the 0-based position of d_targets[b] in the order = the number of classes that come before it, so the row is
 *     top-k correct iff 0 <= rank < k, for every k;
 *   d_loss[b]: logsumexp(row) - row[target] in float32, the maximum subtracted first, expf / logf (no fast intrinsics).
 * A target outside [0, num_classes) gives rank -1 and loss +0.0f for that row (the convention of vasr_error_counts_i32's -1
 * rows); nothing is read outside the row.  Every reduction has one fixed order that depends on num_classes alone and there
 * are no atomics: a row's outputs are bit-identical whatever batch it sits in.  NULL logits, batch <= 0, num_classes <= 0, k
 * outside 0..16 or above num_classes, d_rank / d_loss without d_targets, k == 0 with neither of them, and k > 0 with all
 * three top-k pointers NULL return VASR_ERR_INVALID; num_classes > 65536 returns VASR_ERR_UNSUPPORTED (the limit is in
 * vasr_last_error()) -- all before a device is touched.  No handle, no workspace: one wavefront per row.  (ABI 8) */
VASR_API int vasr_class_scores_f32(const float* d_logits, int batch, int num_classes, const int64_t* d_targets, int k,
                                   int32_t* d_topk_idx, float* d_topk_val, float* d_topk_prob, int32_t* d_rank,
                                   float* d_loss, vasr_stream stream);

/* The CTC forward score, per row: nn.CTCLoss(blank, reduction='none', zero_infinity=False) as CTCLossNM builds it
 * (nemo/collections/asr/losses.py) -- the reference's Evaluation_Loss for the ASR path, and minus log P(transcript | audio) of
 * any transcript.  Forward only: no alignment, no gradient.
 *   d_logp [B][frames][num_classes] f32 contiguous (d_logp of the calls below), d_frames [B] i32: the row's own frames,
 *   d_tgt [B][tgt_width] i32, d_tgt_len [B] i32 (the data layer's transcripts / transcript_length)
 *   -> d_loss [B] f32 = -log sum_paths prod_t p(t, path_t) over row b's own T = d_frames[b] frames and L = d_tgt_len[b] ids.
 * The formula, in float32 log space with expf / logf (no fast intrinsics).  The extended sequence e has S = 2 L + 1 states
 * (blank, y1, blank, ..., yL, blank).
 *   alpha(0, 0) = logp[0][blank], alpha(0, 1) = logp[0][y1], alpha(0, s) = -inf for s >= 2;
 *   for t >= 1:  x0 = alpha(t-1, s), x1 = alpha(t-1, s-1), and x2 = alpha(t-1, s-2) only where e_s is not blank and
 *                e_s != e_(s-2); a term that does not exist (s-1 < 0, no x2) counts as -inf;
 *                lse(x0, x1, x2) = m + logf((expf(x0 - m) + expf(x1 - m)) + expf(x2 - m)) with m the largest of them -- the
 *                terms in the fixed order s, s-1, s-2 -- and -inf where m = -inf;
 *                alpha(t, s) = lse(x0, x1, x2) + logp[t][e_s];
 *   d_loss[b] = -lse(alpha(T-1, S-1), alpha(T-1, S-2), -inf)   (of the only state when L = 0).
 * expf(-inf) adds an exact zero, so a sum of two terms and a sum of three with one -inf have the same bits.  A -inf
 * log-prob is legal input and never produces a NaN.  What torch defines comes out as torch gives it: a row without a path
 * (T < L + the number of adjacent equal label pairs; T == 0 with L > 0) has loss +inf; L == 0 gives minus the sum of the
 * blank's log-probs over the row's frames, taken frame by frame; T == 0 and L == 0 give 0.
 * This library's own conventions, where torch raises or does not check: lengths are clamped into [0, frames] and
 * [0, tgt_width]; a NEGATIVE length on either side gives a quiet NaN for that row; a target id INSIDE the row's length that
 * is < 0, >= num_classes or == blank gives a quiet NaN for that row -- NaN means "never a plausible number", the float
 * counterpart of vasr_error_counts_i32's -1 rows.  Nothing behind a row's lengths is ever read: neither frames >= d_frames[b]
 * nor ids >= d_tgt_len[b].  A state's value depends on its three predecessors alone and the order above is fixed, so a row's
 * loss is bit-identical whatever batch, `frames` or `tgt_width` it is launched with.  No atomics, no workspace, no handle.
 * NULL pointers, batch <= 0, frames < 0, tgt_width < 0, num_classes < 2 and blank outside [0, num_classes) return
 * VASR_ERR_INVALID; tgt_width > 4096 (the limit of vasr_error_counts_i32) returns VASR_ERR_UNSUPPORTED with the limit in
 * vasr_last_error() -- all before a device is touched.  frames == 0 and tgt_width == 0 are legal.  One workgroup per row, the
 * alpha vector double-buffered in LDS (64 KB at tgt_width 4096); DESIGN section 7d has the measured times.  (ABI 8) */
VASR_API int vasr_ctc_loss_f32(const float* d_logp, const int32_t* d_frames, int batch, int64_t frames, int num_classes,
                               int blank, const int32_t* d_tgt, int64_t tgt_width, const int32_t* d_tgt_len,
                               float* d_loss /* [B] */, vasr_stream stream);

/* Forced (Viterbi) CTC alignment, per row: the best SINGLE path of a transcript through the row's log-probs -- the trellis of
 * vasr_ctc_loss_f32 with max in place of log-sum-exp -- and from it the frames each token occupies: character time offsets.
 * The transcript may be a reference, a beam hypothesis, or the row's own greedy transcript (d_ids / d_id_len of the calls
 * below: the best path of the greedy collapse is the per-frame argmax path).
 *   d_logp, d_frames, d_tgt, d_tgt_len, blank: the meaning, the clamping -- T = clamp(d_frames[b], 0, frames), L =
 *   clamp(d_tgt_len[b], 0, tgt_width) -- and the conventions of vasr_ctc_loss_f32.
 * The formula.  The extended sequence e has S = 2 L + 1 states (blank, y1, blank, ..., yL, blank).
 *   delta(0, 0) = logp[0][blank], delta(0, 1) = logp[0][y1], delta(0, s) = -inf for s >= 2;
 *   for t >= 1:  x0 = delta(t-1, s), x1 = delta(t-1, s-1), and x2 = delta(t-1, s-2) only where e_s is not blank and
 *                e_s != e_(s-2); a term that does not exist counts as -inf;
 *                best = x0, bp = 0;  if x1 > best: best = x1, bp = 1;  if x2 > best: best = x2, bp = 2;
 *                delta(t, s) = best + logp[t][e_s];
 *   a later candidate wins only STRICTLY (the order s, s-1, s-2 of the loss).  The final state is S-1, unless
 *   delta(T-1, S-2) > delta(T-1, S-1) strictly; d_score[b] = that delta; the path follows bp back from there to frame 0.
 * Only comparisons and float32 additions: no transcendental function, no multiply, nothing a compiler can contract -- the
 * same recursion in IEEE float32 gives the same bits, in score, path and spans.
 * Rows: a row whose score is -inf has NO PATH (T < L + the number of adjacent equal label pairs; T == 0 with L > 0; -inf
 * log-probs that block every path).  A negative length on either side, or an id inside the row's length that is < 0, >=
 * num_classes or == blank, gives a quiet NaN score.  T == 0 and L == 0 give score 0.  A -inf log-prob is legal and never
 * makes a NaN.
 * Outputs:
 *   d_score [B] f32
 *   d_start, d_end [B][tgt_width] i32: token j holds the frames [start, end) whose state is 2 j + 1; blank frames belong to no
 *                  token; on a path every token has end > start
 *   d_tok_logp [B][tgt_width] f32 (may be NULL): the sum over t = start .. end-1, ascending, of logp[t][y_j], starting from
 *                  the first term
 *   d_path [B][frames] i32 (may be NULL): the state index s(t) for t < T
 * Unfilled entries -- j >= L, t >= T, every entry of a row with no path or a NaN score -- are -1 in the three i32 arrays and
 * +0.0f in d_tok_logp.  EVERY element of every non-NULL output is written; nothing behind a row's lengths is ever read.
 * No atomics; a row's outputs are bit-identical whatever batch, `frames` or `tgt_width` it is launched with.
 * The back-pointers (2 bits per frame and state) go through d_workspace: vasr_ctc_align_workspace_bytes(batch, frames,
 * tgt_width) bytes of device memory at any address, contents undefined before and after; the function is host only, touches
 * no device, and returns 0 for arguments the call below refuses (batch <= 0, frames < 0, tgt_width outside 0..4096).  At
 * most 2 bits per frame and state slot (256 lanes x 4 slots while 2 * tgt_width + 1 <= 1024, x 33 slots above) + 256 bytes.
 * NULL d_logp / d_frames / d_tgt / d_tgt_len / d_score / d_start / d_end, batch <= 0, frames < 0, tgt_width < 0, num_classes < 2,
 * blank outside [0, num_classes) and a workspace that is NULL or smaller than required return VASR_ERR_INVALID; tgt_width >
 * 4096 returns VASR_ERR_UNSUPPORTED with the limit in vasr_last_error() -- all before a device is touched.  frames == 0 and
 * tgt_width == 0 are legal.  No handle; one workgroup per row; DESIGN section 7e has the measured times.  (ABI 8) */
VASR_API size_t vasr_ctc_align_workspace_bytes(int batch, int64_t frames, int64_t tgt_width);
VASR_API int vasr_ctc_align_f32(const float* d_logp, const int32_t* d_frames, int batch, int64_t frames, int num_classes,
                                int blank, const int32_t* d_tgt, int64_t tgt_width, const int32_t* d_tgt_len,
                                float* d_score /* [B] */, int32_t* d_start, int32_t* d_end, float* d_tok_logp, int32_t* d_path,
                                void* d_workspace, size_t workspace_bytes, vasr_stream stream);

/* ---- the whole path in one call (the fast path bench.py times) ------------------------ */
/* wav -> mel -> encoder -> CTC head -> log-softmax/argmax -> collapse, all intermediates in
 * the workspace (padded time stride, no port tensors materialised).
 *   d_pred   [B][T'] i64  (may be NULL)          d_ids [B][T'] i32, d_id_len [B] i32
 *   d_logp   [B][T'][V+1] f32 (may be NULL: greedy only needs the argmax)
 *   d_enc_len [B] f32 (may be NULL) */
VASR_API int vasr_transcribe_greedy_f32(vasr_handle* h, const float* d_wav, const int64_t* d_len, int batch,
                               int64_t samples, int64_t* d_pred, int32_t* d_ids, int32_t* d_id_len,
                               float* d_logp, float* d_enc_len, void* d_workspace, size_t workspace_bytes,
                               vasr_stream stream);

/* The same call on int16 PCM as it sits in a wav file (AudioSegment._convert_samples_to_float32, parts/segment.py:61-74:
 * samples.astype('float32') * 2^-15): the front end's staging load converts and scales each sample as it reads it (SURVEY
 * section 8 f1) -- an exact conversion times an exact power of two, so every output equals, bit for bit, what
 * vasr_pcm16_to_f32 followed by vasr_transcribe_greedy_f32 returns; half the bytes over PCIe and into the first kernel, one
 * launch and one [B][L] float buffer fewer.  d_pcm [B][L] int16 (rows zero padded).  (ABI 7) */
VASR_API int vasr_transcribe_greedy_pcm16(vasr_handle* h, const int16_t* d_pcm, const int64_t* d_len, int batch,
                                 int64_t samples, int64_t* d_pred, int32_t* d_ids, int32_t* d_id_len,
                                 float* d_logp, float* d_enc_len, void* d_workspace, size_t workspace_bytes,
                                 vasr_stream stream);

/* ---- the classification path (speech commands, keywords) ----------------------------------- */
/* CropOrPadSpectrogramAugmentation.forward (audio_preprocessing.py:666-738) on contiguous port tensors.
 *   d_in [B][feat][frames] f32 -> d_out [B][feat][audio_length] f32, d_out_len [B] i64 = audio_length (may be NULL)
 * frames > audio_length: row b is d_in[b, :, off : off + audio_length] with off = d_offsets[b] (device i64 [B], required;
 * the reference draws torch.randint(0, frames - audio_length + 1, [B])), clamped into [0, frames - audio_length] so that no
 * read leaves the row.  Otherwise (frames == audio_length included, with zero pads) the row sits between
 * left = (audio_length - frames) / 2 zero frames and audio_length - frames - left on the right: the odd frame goes right.
 * A copy: every value is bit-equal to the one it was cut from.  d_offsets may be NULL when frames <= audio_length. */
VASR_API int vasr_crop_or_pad_f32(const float* d_in, int batch, int feat, int64_t frames, int64_t audio_length,
                                  const int64_t* d_offsets, float* d_out, int64_t* d_out_len, vasr_stream stream);

/* JasperDecoderForClassification.forward (jasper.py:310-319): pool over time, Linear, optional softmax (vasr_set_classifier).
 *   d_enc [B][feat_in][T'] f32 contiguous -> d_out [B][num_classes] f32: logits, or (softmax != 0) F.softmax(logits, -1)
 * Workspace: B * feat_in * 4 bytes (the pooled vectors). */
VASR_API int vasr_classifier_f32(vasr_handle* h, const float* d_enc, int batch, int64_t enc_frames, int softmax, float* d_out,
                                 void* d_workspace, size_t workspace_bytes, vasr_stream stream);

/* The whole classification path in one call, as vasr_transcribe_greedy_f32 is for CTC: wav -> mel -> crop / pad to
 * audio_length -> encoder -> pool + Linear (+ softmax), all intermediates in the workspace; the crop / pad writes straight
 * into the encoder's padded-pitch input buffer.  The handle needs a front end, an encoder and vasr_set_classifier.
 *   d_wav [B][samples] f32 (rows zero padded), d_len [B] i64; d_offsets [B] i64 device, may be NULL when
 *   1 + samples / hop <= audio_length (no crop can occur); d_out [B][num_classes] f32;
 *   d_mel (may be NULL) [B][n_mels][audio_length] f32: the encoder's input, CropOrPadSpectrogramAugmentation's output port.
 * The reference's batched semantics by default: the crop acts on the batch tensor's width, every row of which is
 * 1 + samples / hop frames.  With vasr_set_row_independent row b is as wide as a call on it alone makes it, 1 + d_len[b] / hop
 * frames, reflected at its own end, and is cut (d_offsets[b], clamped into the row) or centred on that width: its output
 * is what a batch-1 call on the row alone returns, bit for bit.
 * Workspace: vasr_classify_workspace_bytes(h, batch, samples, audio_length). */
VASR_API size_t vasr_classify_workspace_bytes(const vasr_handle* h, int batch, int64_t samples, int64_t audio_length);
VASR_API int vasr_classify_f32(vasr_handle* h, const float* d_wav, const int64_t* d_len, int batch, int64_t samples,
                               int64_t audio_length, const int64_t* d_offsets, int softmax, float* d_out, float* d_mel,
                               void* d_workspace, size_t workspace_bytes, vasr_stream stream);

/* GEMM arithmetic of the 1x1 convolutions of the encoder:
 *   0            v_mfma_f32_32x32x2_f32: bit-for-bit an fp32 fmaf chain;
 *   1            every fp32 operand split exactly into three bf16 terms, six cross products per multiply on
 *                v_mfma_f32_32x32x16_bf16 with fp32 accumulation (product error < one fp32 rounding, measured
 *                error against fp64 not larger than mode 0's; 2.67x less matrix time);
 *   2 (opt-in)   REDUCED precision: only the two upper bf16 terms of each operand (16 significant bits) and the
 *                three largest cross products -- half the MFMA work of mode 1 (QuartzNet15x5, B = 64: 5.5 instead of
 *                7.4 ms per batch), log-prob error against the reference goldens 5-10x mode 1's (still inside the
 *                2e-3 tolerance there, identical predictions), more accurate than the TF32 convolutions PyTorch
 *                runs by default on the GPUs the reference targets.  Never the default, never the headline number.
 *   3 (default)  every fp32 operand scaled by a power of two (exact) and split into TWO fp16 terms (22 significant
 *                bits; the scale comes from the maximum |x| of the utterance, which the kernel that produced the tensor
 *                publishes, so a row's result does not depend on the rest of its batch), the three largest cross
 *                products on v_mfma_f32_32x32x16_f16 with fp32 accumulation: half the matrix work of mode 1.  Its
 *                per-product error is larger than mode 1's (<= 3 * 2^-22) but it rounds the accumulator half as often;
 *                measured against fp64 it is not less accurate than modes 0 and 1 (tests/test_gpu_parity.py::
 *                test_split_gemms_are_as_accurate_as_fp32_mfma) and all reference fixtures hold with the same
 *                tolerances.  A GEMM whose input has no published maxima (port tensors of the per-module entry points,
 *                the CTC head) runs as mode 1.  In this mode the 256-channel separable sub-blocks (depthwise K = 33 / 39 +
 *                1x1 conv + BN + residual + ReLU) run as ONE fused kernel when the batch's 128-frame tiles fill the chip
 *                (encoder_fused.hip; its operand scale comes from a bound -- max |x| times the layer's largest tap sum --
 *                instead of the measured maximum, same tolerances).  Whether a sub-block is fused depends on the batch
 *                shape, and the two forms round differently: bit-identical rows across batch compositions are promised by
 *                vasr_set_row_independent (which never fuses), not by the default mode.
 * Layers whose shape the split kernel does not cover keep mode 0.
 * The environment variable VASR_GEMM=fp32 / bf16x3 / bf16x2 / f16x2 sets the initial mode of new handles. */
VASR_API int vasr_set_gemm_mode(vasr_handle* h, int mode);
VASR_API int vasr_get_gemm_mode(const vasr_handle* h);

/* ---- audio ingest (callers of the path: infer.py:200 librosa.load(sr=16000); parts/segment.py:19-32,61-74) ---- */
/* int16 PCM -> float32 scaled by 2^-15 (AudioSegment._convert_samples_to_float32). n = total samples. */
VASR_API int vasr_pcm16_to_f32(const int16_t* d_pcm, int64_t n, float* d_out, vasr_stream stream);
/* Band-limited sample-rate conversion of a padded batch (interpolated windowed-sinc, the scheme of resampy's
 * kaiser_best that librosa.load uses by default; third-party => parity unpinned).  d_table = [nwin][2] floats
 * (window value, delta to the next entry) with num_table entries per zero crossing, built on the host
 * (viet-asr_amd/audio.py::sinc_table); ratio = sr_out / sr_in.  Lengths as librosa.load -> librosa.resample(fix=True)
 * produces them: resampy computes int(d_len_in[b] * ratio) samples, librosa pads (with zeros) to
 * d_len_out[b] = ceil(d_len_in[b] * ratio), both products in double (11 025 -> 16 000 Hz: 5 000 samples give 7 256
 * computed samples and a length of 7 257; the reference's 8 -> 16 kHz: 2 n either way).  Rows of d_out are
 * zero from int(d_len_in[b] * ratio) on, up to ld_out.  ld_out >= ceil(ld_in * ratio).  A row's length is clamped to
 * [0, ld_in] (a negative one gives an all-zero row of length 0); samples at or beyond it are never read: the caller's padding
 * may hold anything, NaN included.  (ABI 6; ABI 5 reported int(len * ratio).) */
VASR_API int vasr_resample_f32(const float* d_in, int64_t ld_in, const int64_t* d_len_in, int batch, const float* d_table,
                      int nwin, int num_table, double ratio, float* d_out, int64_t ld_out, int64_t* d_len_out,
                      vasr_stream stream);

/* Leading / trailing silence trim of a padded batch: AudioSegment(trim=True) (parts/segment.py:19-32) ->
 * librosa.effects.trim(samples, top_db) of librosa < 0.10, which the shipped QuartzNet15x5 config turns on
 * (AudioToTextDataLayer.trim_silence: true).  Third-party arithmetic restated from its published form, parity unpinned
 * (librosa is not available to the tests; tests/trim_reference.py is the float64 restatement they use).
 * Per row of n = clamp(d_len[b], 0, ld_in) samples x, with frame_length (librosa: 2048), hop_length (512), top_db (60):
 *   y      = x padded by frame_length / 2 on both sides in numpy's `reflect` mode: periodic mirroring with period 2 (n - 1),
 *            the edge sample not repeated; for n == 1 every padded sample is that sample;
 *   F      = 1 + n / hop_length frames; frame f covers y[f hop : f hop + frame_length]; mse[f] = the mean of its squares;
 *   ref    = max_f mse[f], amin = 1e-10; frame f is NON-SILENT iff
 *            10 log10(max(amin, mse[f])) - 10 log10(max(amin, ref)) > -top_db,
 *            decided here in the product form max(amin, mse[f]) > max(amin, ref) * 10^(-top_db / 10), in float64, the factor
 *            computed on the host (squares and sums are float64 too: a float32 square is exact there);
 *   start  = first * hop, end = min(n, (last + 1) * hop) over the first and last non-silent frame; start = end = 0 if none;
 *   d_out[b] = x[start : end] bit for bit, then zeros up to ld_out; d_len_out[b] = end - start; d_start[b] = start.
 * Consequences, as in librosa:
 *   - a row whose loudest frame has mse < 1e-10 is NOT trimmed: every frame sits at the amin floor, 0 dB below ref (all-zero
 *     rows, rows at the 1e-6 level);
 *   - for top_db > 0 the loudest frame is always non-silent; with frame_length >= 2 hop_length and top_db > 3.02 so is the
 *     frame in front of the last one whenever the last one is (it holds every sample the last one mirrors: at least half its
 *     energy), hence d_len_out[b] >= min(n, hop_length).  (With frame_length == hop_length a row whose only loud frame is
 *     the last one, which starts at n when hop_length divides n, comes out empty.);
 *   - n == 0 gives start = d_len_out = 0; an inner gap is kept.
 * int16 rows (the _pcm16 form): energies are of value * 2^-15, as AudioSegment scales -- the scale matters only through
 * amin --; the copy stays int16.
 * Samples at or beyond a row's length are never read as data (the mirror indexes inside [0, n)): the caller's padding may
 * hold anything.  A row's outputs do not depend on the other rows, on the batch size, on ld_in or on the row's alignment.
 * Three launches, no atomics, no host synchronisation, no handle.  EVERY element of every non-NULL output is written.
 * d_out must not alias d_in; ld_out >= ld_in; ld_in == 0 is legal; d_start may be NULL.
 * The chunk sums go through d_workspace: vasr_trim_silence_workspace_bytes(batch, ld_in, frame_length, hop_length) bytes of
 * device memory at any address, contents undefined before and after (8 bytes per hop_length samples + 8 per row + 512); the
 * function is host only and returns 0 for arguments the calls refuse.
 * NULL d_in / d_len / d_out / d_len_out / d_workspace, d_out == d_in, batch <= 0, a negative ld, ld_out < ld_in, a non-finite
 * top_db and a workspace smaller than required (the byte count is in vasr_last_error()) return VASR_ERR_INVALID; hop_length < 1,
 * frame_length not a multiple of hop_length or frame_length > 8192 return VASR_ERR_UNSUPPORTED with the limit in
 * vasr_last_error(); an argument error wins over the limit -- all before a device is touched.  DESIGN section 7f has the
 * measured times.  (ABI 8) */
VASR_API size_t vasr_trim_silence_workspace_bytes(int batch, int64_t ld_in, int frame_length, int hop_length);
VASR_API int vasr_trim_silence_f32(const float* d_in, int64_t ld_in, const int64_t* d_len, int batch, float top_db,
                                   int frame_length, int hop_length, float* d_out, int64_t ld_out, int64_t* d_len_out,
                                   int64_t* d_start, void* d_workspace, size_t workspace_bytes, vasr_stream stream);
VASR_API int vasr_trim_silence_pcm16(const int16_t* d_in, int64_t ld_in, const int64_t* d_len, int batch, float top_db,
                                     int frame_length, int hop_length, int16_t* d_out, int64_t ld_out, int64_t* d_len_out,
                                     int64_t* d_start, void* d_workspace, size_t workspace_bytes, vasr_stream stream);

/* Split at silences: the non-silent intervals of every row of a padded batch, for cutting a long recording at its pauses.
 * With min_silence_frames = 1 and max_segment_frames = 0 this is librosa.effects.split(y, top_db, ref=np.max, frame_length,
 * hop_length) of librosa < 0.10 -- the trim above with EVERY run of non-silent frames reported, not only the outer bounds.
 * Third-party arithmetic restated from its published form, parity unpinned (librosa is not available to the tests;
 * tests/split_reference.py is the float64 restatement they use).  Two rules of an ASR front end sit on top of it: short
 * pauses are bridged, over-long runs are cut at their quietest frame.
 * Per row of n = clamp(d_len[b], 0, ld_in) samples, with frame_length, hop_length, top_db as for the trim,
 * m = min_silence_frames >= 1 and M = max_segment_frames (0: no limit, otherwise >= 2):
 *   A. flags: exactly the trim's.  F = 1 + n / hop_length frames of the reflect-padded row; frame f is NON-SILENT iff
 *      max(amin, mse[f]) > max(amin, ref) * 10^(-top_db / 10), ref the loudest frame's mse, amin = 1e-10, all in float64.  A row
 *      with n == 0 has no segment; a row whose loudest frame is below amin has every frame non-silent (for top_db > 0);
 *   B. runs: a run is a maximal stretch of frames that starts and ends on a non-silent frame and contains no m or more
 *      consecutive silent frames: a silent gap of fewer than m frames between two non-silent frames is bridged; leading and
 *      trailing silence never is.  With m = 1 the runs are librosa.effects.split's;
 *   C. cuts (M > 0 only): a run [s, e) with e - s > M is cut at c, the frame with the smallest energy among s + ceil(M / 2) ..
 *      s + M inclusive, the lowest index among equal energies -- the energy is the float64 frame sum the threshold uses --;
 *      [s, c) is a segment and the rule is applied again to [c, e).  Every segment is then at most M frames long and the pieces
 *      of a run are contiguous: no sample of a run is lost;
 *   D. bounds: the segment of frames [f0, f1) is the samples [min(n, f0 hop), min(n, f1 hop)) (librosa's frames_to_samples and
 *      np.minimum).  As in librosa, a run that starts on the last frame of a row whose n is a multiple of hop_length gives the
 *      empty interval [n, n); it is reported, not filtered;
 *   E. output: d_bounds[b][k] = (start, end), int64 pairs in ascending order for k < min(count, max_segments), the row pitch
 *      is 2 max_segments; d_count[b] = the row's total number of segments, ALSO where it exceeds max_segments (the caller sees
 *      the overflow).  Entries at and behind min(count, max_segments) are not written.  A row has at most F segments.
 * int16 rows (the _pcm16 form): energies of value * 2^-15, as for the trim.  Samples at or beyond a row's length are never
 * read as data.  A row's outputs do not depend on the other rows, on the batch size, on ld_in or on the row's alignment.
 * Two launches, no atomics, no host synchronisation, no handle.
 * The chunk sums and the runs go through d_workspace: vasr_split_silence_workspace_bytes(batch, ld_in, frame_length,
 * hop_length) bytes of device memory at any address, contents undefined before and after (16 bytes per hop_length samples +
 * 512); the function is host only and returns 0 for arguments the calls refuse.
 * NULL d_in / d_len / d_bounds / d_count / d_workspace, batch <= 0, ld_in < 0, max_segments < 0, min_silence_frames < 1,
 * max_segment_frames < 0 or == 1, a non-finite top_db and a workspace smaller than required return VASR_ERR_INVALID; the frame
 * forms the trim refuses return VASR_ERR_UNSUPPORTED; an argument error wins over the limit -- all before a device is touched.
 * DESIGN section 7g has the kernels.  (added within ABI 8) */
VASR_API size_t vasr_split_silence_workspace_bytes(int batch, int64_t ld_in, int frame_length, int hop_length);
VASR_API int vasr_split_silence_f32(const float* d_in, int64_t ld_in, const int64_t* d_len, int batch, float top_db,
                                    int frame_length, int hop_length, int min_silence_frames, int max_segment_frames,
                                    int64_t* d_bounds, int64_t max_segments, int64_t* d_count, void* d_workspace,
                                    size_t workspace_bytes, vasr_stream stream);
VASR_API int vasr_split_silence_pcm16(const int16_t* d_in, int64_t ld_in, const int64_t* d_len, int batch, float top_db,
                                      int frame_length, int hop_length, int min_silence_frames, int max_segment_frames,
                                      int64_t* d_bounds, int64_t max_segments, int64_t* d_count, void* d_workspace,
                                      size_t workspace_bytes, vasr_stream stream);

/* Gather segments of a padded batch into a padded batch: d_out[s][t] = d_in[d_row[s]][d_start[s] + t] for t < d_len[s], bit
 * for bit, and zero up to ld_out, for s < segments.  EVERY element of every output row is written.  A segment whose row is
 * outside [0, batch), whose start or length is negative, with start + len > ld_in, or with len > ld_out gives a row of zeros;
 * nothing is read or written out of bounds.  One launch, no atomics, no host synchronisation, no handle; d_out must not alias
 * d_in.  NULL pointers, batch <= 0, ld_in < 0, segments <= 0 and ld_out <= 0 return VASR_ERR_INVALID before a device is
 * touched.  (added within ABI 8) */
VASR_API int vasr_gather_segments_f32(const float* d_in, int64_t ld_in, int batch, const int32_t* d_row, const int64_t* d_start,
                                      const int64_t* d_len, int64_t segments, float* d_out, int64_t ld_out, vasr_stream stream);
VASR_API int vasr_gather_segments_pcm16(const int16_t* d_in, int64_t ld_in, int batch, const int32_t* d_row,
                                        const int64_t* d_start, const int64_t* d_len, int64_t segments, int16_t* d_out,
                                        int64_t ld_out, vasr_stream stream);

/* ---- audio perturbation: the arithmetic of AudioAugmentor (parts/perturb.py) on a padded float32 batch -------------------
 * Gain, shift, noise at an SNR, white noise and convolution with a room impulse response, for robustness sweeps without a
 * round trip through the host.  The host draws the random parameters (viet-asr_amd/perturb.py consumes the generators as the
 * reference's per-utterance calls do) and uploads them as small per-row arrays; these entry points are the arithmetic.  An
 * int16 batch goes through vasr_pcm16_to_f32 first.  Common to all of them: no handle, no atomics, no host synchronisation;
 * a row's length is n = clamp(d_len[b], 0, ld_in); samples at or behind it are never read as data (the caller's padding may
 * hold NaN); EVERY element of every non-NULL output is written, zeros behind a row's length up to ld_out; a row's bits do
 * not depend on the other rows, on the batch size, on ld_in or on the row's alignment; every argument is checked before a
 * device is touched, VASR_ERR_INVALID wins over VASR_ERR_UNSUPPORTED, limits are reported in vasr_last_error().  tests/
 * perturb_reference.py is the float64 restatement; DESIGN section 7h has the kernels.  (added within ABI 8)
 *
 * vasr_mean_square_f32: d_ms[b] = mean(x^2) of row b in float64, the argument of AudioSegment.rms_db (parts/segment.py:
 * 136-139; the reference takes the mean in float32).  A float32 square is exact in float64; the sums run over chunks of 4096
 * samples counted from the row's first one (thread t of 256 adds positions 4 t + 1024 i + {0 .. 3} in ascending order, the
 * threads are added in a binary tree), the chunk sums are added in the same fixed order, the total is divided by n: within
 * n 2^-53 of the exact sum.  n == 0 gives 0.0.  Two launches.  The chunk sums go through d_workspace:
 * vasr_mean_square_workspace_bytes(batch, ld_in) bytes at any address (8 per 4096 samples + 256), contents undefined before
 * and after; the function is host only and returns 0 for arguments the call refuses.  NULL d_in / d_len / d_ms /
 * d_workspace, batch <= 0, ld_in < 0 and a workspace smaller than required return VASR_ERR_INVALID. */
VASR_API size_t vasr_mean_square_workspace_bytes(int batch, int64_t ld_in);
VASR_API int vasr_mean_square_f32(const float* d_in, int64_t ld_in, const int64_t* d_len, int batch, double* d_ms,
                                  void* d_workspace, size_t workspace_bytes, vasr_stream stream);

/* vasr_noise_plan_f64: NoisePerturbation.perturb (parts/perturb.py:94-107) restated in float64 and product form, one launch.
 * Per row b: n = max(d_len[b], 0), ms_x = d_ms_x[b], the noise row r = d_row[b] with N = max(d_noise_len[r], 0) samples and
 * mean square ms_v = d_ms_v[r], snr_db = d_snr_db[b], u = d_u[b] in [0, 1) (the one random() that uniform(0.0, .) consumes):
 *   d_scale[b] = (float) min(sqrt(ms_x / ms_v) * 10^(-snr_db / 20), 10^(max_gain_db / 20)), which is 10^(gain / 20) of the
 *                reference's noise_gain_db = min(rms_db(x) - rms_db(v) - snr_db, max_gain_db); the cap is at most FLT_MAX.
 *                ms_x == 0 gives 0 (the reference: 0 or NaN); ms_v == 0 with ms_x > 0 gives the cap;
 *   d_start[b]:  for N > n, rint(((N / sr - n / sr) * u) * sr) in doubles, each operation rounded once, half to even -- the
 *                reference's start_time = uniform(0.0, noise.duration - data.duration) and int(round(start_time * sr)) --
 *                clamped to [0, N - n]; for N <= n it is 0 and vasr_mix_f32 wraps the noise modulo N (a stated deviation:
 *                the reference raises there).
 * r < 0 or r >= noise_rows gives scale 0 and start 0: nothing is added.  NULL pointers, batch / noise_rows / sample_rate <= 0
 * and a NaN max_gain_db return VASR_ERR_INVALID. */
VASR_API int vasr_noise_plan_f64(const int64_t* d_len, const double* d_ms_x, const int32_t* d_row, const double* d_snr_db,
                                 const double* d_u, int batch, const int64_t* d_noise_len, const double* d_ms_v, int noise_rows,
                                 double max_gain_db, int sample_rate, float* d_scale, int64_t* d_start, vasr_stream stream);

/* vasr_mix_f32: gain, shift and an additive signal in one memory-bound pass; the length does not change.  Per row, with
 * g = d_gain[b], s = d_shift[b] (samples), c = d_scale[b], r = d_add_row[b], v = row r of d_add [add_rows][ld_add] with
 * N = clamp(d_add_len[r], 0, ld_add) samples, st = d_start[b] mod N:
 *   d_out[b][t] = g * x[t + s] + c * v[(st + t) mod N]     for t < n, zero from n up to ld_out,
 * in float32 as fmaf(c, v, fl(g * x)).  The x term is 0 where t + s falls outside [0, n): ShiftPerturbation's copy in place
 * with zero fill, for both signs (perturb.py:69-81; s = int(shift_ms * sr // 1000)); a shift with |s| > n is ignored, the
 * reference's duration rule in samples.  g is GainPerturbation's 10^(gain_db / 20).  d_gain, d_shift and d_add may each be
 * NULL (1, 0, nothing added); d_start may be NULL (0).  With c == 0, r outside [0, add_rows) or N == 0 the addend is NOT
 * read: a NaN there changes nothing.  With g == 1, s == 0 and nothing added the row is a bit-for-bit copy.  White noise is
 * an addend the caller draws on the device (one row per utterance, r = b).  One launch, 16-byte loads and stores where the
 * addresses allow (the same arithmetic either way).  d_out must not alias d_in or d_add; ld_out >= ld_in >= 0.
 * NULL d_in / d_len / d_out, an addend without d_add_len / d_add_row / d_scale, ld_add < 0 or add_rows <= 0 with an addend,
 * batch <= 0, a negative ld and ld_out < ld_in return VASR_ERR_INVALID. */
VASR_API int vasr_mix_f32(const float* d_in, int64_t ld_in, const int64_t* d_len, int batch, const float* d_gain,
                          const int64_t* d_shift, const float* d_add, int64_t ld_add, int add_rows, const int64_t* d_add_len,
                          const int32_t* d_add_row, const float* d_scale, const int64_t* d_start, float* d_out, int64_t ld_out,
                          vasr_stream stream);

/* Convolution with a bank of impulse responses: ImpulsePerturbation (perturb.py:56-60), scipy.signal.fftconvolve(x, h,
 * "full"), length n + m - 1.  d_ir [R][ld_ir] holds the responses, m = clamp(d_ir_len[r], 1, ld_ir) taps each.
 * vasr_convolve_prepare_f32 runs once per bank: it writes the spectra of the zero-padded partitions of every response into
 * d_spectra (vasr_convolve_spectra_bytes(R, ld_ir) bytes, 8-byte aligned: 16 KiB per 2048 taps and response + 8 KiB; host only,
 * 0 for arguments the calls refuse), behind the transform's twiddle factors, which it builds on the host (float64 rounded to
 * float32) and copies there with one hipMemcpyAsync from host memory -- the one call of this group that is not launches only.  The buffer is opaque and belongs to this version of the library.
 * vasr_convolve_f32 runs per batch: with r = d_ir_row[b],
 *   d_out[b][t] = sum_k h_r[k] x[t - k]   for t < n + m - 1, zero up to ld_out; d_len_out[b] = n + m - 1;
 *   r < 0 (or r >= R) copies the row bit for bit, d_len_out[b] = n;   n == 0 gives d_len_out[b] = 0.
 * Uniformly partitioned overlap-save in ONE kernel, transform length 2048, partitions of 1024 taps, one workgroup per row and
 * block of 1024 outputs: it stages the input segments it needs and transforms them in LDS, multiplies by the partition spectra
 * and accumulates in registers across partitions, runs one inverse transform and stores; no spectrum of x goes through
 * memory.  Two partitions share one complex transform (the spectrum stored for a pair is that of h_even - i h_odd).  The error is normwise: |error| <= c 2^-24 |h|_2
 * |x|_2 per row (tests/perturb_reference.py has c).  d_ir_len passed here must be the array the spectra were prepared from.
 * d_out must not alias d_in.  NULL pointers, batch <= 0, R <= 0, ld_in < 0, ld_ir < 1, ld_out < 1, ld_out < ld_in + ld_ir
 * - 1, a misaligned or too small spectra buffer return VASR_ERR_INVALID; ld_ir > 32768 or R > 65535 return
 * VASR_ERR_UNSUPPORTED with the limit in vasr_last_error(); an argument error wins over the limit. */
VASR_API size_t vasr_convolve_spectra_bytes(int R, int64_t ld_ir);
VASR_API int vasr_convolve_prepare_f32(const float* d_ir, int64_t ld_ir, const int64_t* d_ir_len, int R, void* d_spectra,
                                       size_t spectra_bytes, vasr_stream stream);
VASR_API int vasr_convolve_f32(const float* d_in, int64_t ld_in, const int64_t* d_len, int batch, const int32_t* d_ir_row,
                               const int64_t* d_ir_len, const void* d_spectra, int R, int64_t ld_ir, float* d_out,
                               int64_t ld_out, int64_t* d_len_out, vasr_stream stream);

/* ---- feature masks: SpecAugment / SpecCutout (parts/spectr_augment.py) on a [batch][feat][ld] float32 feature tensor --------
 * `x.masked_fill(mask, 0)` for a mask that is a union of rectangles.  The host draws them (viet-asr_amd/asr.py consumes Python's
 * generator as the reference's forward does, for exact parity) and uploads them RESOLVED: d_rects [n][4] int32 = f0, f1, t0, t1,
 * the half-open ranges [f0, f1) of feature rows and [t0, t1) of frames; d_row_begin [batch + 1] int32: batch row b owns the
 * rectangles d_row_begin[b] .. d_row_begin[b + 1] - 1 (a CSR list; n is never given to the call -- the entries of d_row_begin
 * must index d_rects).  No handle, no atomics, no host synchronisation, ONE launch in either form:
 *   in place (d_out == d_in and ld_out == ld_in): the kernel only STORES +0.0f over the rectangles; it does not read the tensor,
 *     its work is proportional to the masked area, a row without rectangles costs two dword loads per workgroup;
 *   out of place: one pass copies d_in to d_out with the masked cells written as +0.0f (16-byte loads and stores where both
 *     addresses allow; a pitch or a base that is no multiple of 4 cells takes dwords for the rows it misaligns).
 * A masked cell is exactly +0.0f whatever it held (NaN, +-inf, -0.0); every other cell of [0, feat) x [0, frames) keeps its bit
 * pattern; columns frames .. ld are never written in either form.  The kernel clips every rectangle to [0, feat) x [0, frames)
 * and treats lo >= hi, a non-increasing d_row_begin pair and a negative d_row_begin[b] as empty: no store leaves the tensor
 * whatever the device arrays hold.  Rectangles may overlap (all writers store the same value).  Every refusal comes before a
 * device is touched: NULL pointers, batch / feat / frames <= 0, ld_in or ld_out < frames, a pointer that is not 4-byte aligned,
 * and d_in / d_out ranges that overlap without being the same tensor (same pointer and pitch) return VASR_ERR_INVALID; a tensor
 * of more than 2^31 - 1 workgroups (8 feature rows x 1024 frames each) or frames > 2^31 - 2049 returns VASR_ERR_UNSUPPORTED.
 * tests/specaug_reference.py is the rasteriser the kernel is held to; DESIGN section 7i has the kernels.  (added within ABI 8) */
VASR_API int vasr_spec_mask_f32(const float* d_in, int64_t ld_in, float* d_out, int64_t ld_out, int batch, int feat, int64_t frames,
                                const int32_t* d_rects, const int32_t* d_row_begin, vasr_stream stream);

/* While set, vasr_transcribe_greedy_f32 / _pcm16 run the in-place form above on the normalised log-mel features (pitch and
 * valid frames as the call has them, feat = n_mels), behind the normalisation launch(es) and in front of the encoder: one more
 * launch, no more memory; the first layer's operand maxima are taken from the masked tensor.  d_row_begin has batch + 1 entries
 * for the batch of the call; with vasr_set_slices every slice applies the rows it owns.  The pointers are BORROWED until they
 * are cleared (NULL, NULL) and must stay valid for every call enqueued in between.  With nothing set the call is what it is
 * without this entry point: same launches, same bits.  vasr_classify_f32 is not hooked.  A NULL handle and one pointer without
 * the other return VASR_ERR_INVALID.  (added within ABI 8) */
VASR_API int vasr_set_feature_masks(vasr_handle* h, const int32_t* d_rects, const int32_t* d_row_begin);

/* The fused call can cut the batch into `slices` contiguous parts (1..4; default 1 = off, because on MI355X it
 * measured slower: 11.7 -> 13.5 ms at 2 slices) and run each on its own
 * internal HIP stream, forked from / joined to `stream` with events: one part's HBM-bound kernels (depthwise,
 * GEMM epilogue stores) then overlap another part's MFMA-bound GEMM main loops.  In row-independent mode results do not depend
 * on it; in the default mode every slice is a batch of its own for the shape-dependent choice between the fused and the
 * two-kernel form of a 256-channel sub-block (same tolerance, different rounding: vasr_set_gemm_mode, mode 3). */
VASR_API int vasr_set_slices(vasr_handle* h, int slices);

/* Row-independent batching (net-new; default off = the reference's batched semantics).  The reference's results
 * depend on the padded batch a signal sits in: torch.stft reflects at the end of the PADDED row (parts/features.py:
 * 181-188) and the greedy decoder collapses the padded frames too (helpers.py:7-33, quirk Q4), which is
 * why it serves one utterance per call (app.py:66-67).  With on != 0, vasr_melspec_f32 and vasr_transcribe_greedy_f32
 * treat row b as if it were alone: reflect padding at length[b], ids / id_len collapsed over the 1 + length[b] / hop mel
 * frames (taken through the conv chain) an unbatched call would have produced.  Everything in between is already
 * row-local (masks at the row's length, eval-mode BN), so ids / id_len equal those of batch-1 calls bit for bit
 * whatever the other rows are -- also in ragged batches in the fp16-split arithmetic: the encoder output's maxima (the
 * CTC head's operand scale) are taken over the row's own frames and the head reads zeros behind them.  Every length[b]
 * must exceed n_fft / 2 (an unbatched torch.stft refuses shorter input); pred / logp keep their [B, T'] shapes, frames
 * past a row's own count are unspecified. */
VASR_API int vasr_set_row_independent(vasr_handle* h, int on);
/* Compute units that another kernel of the caller's keeps busy while this handle's kernels run -- e.g. the beam search of
 * the previous batch on a side stream, one workgroup per utterance (engine.forward_beam).  The GEMM tile choice then
 * fills whole rounds of the REMAINING units: with 64 of 256 taken, 512 x 128 workgroups (one per CU) would need two
 * rounds, the second a third full; 256 x 64 ones quantise four times finer.  0 (default) = the whole device.
 * RESULTS DO NOT DEPEND ON THE HINT: it selects only between forms that give the same bits (GEMM tile shapes, the fused kernel's
 * tile width); whether a sub-block runs fused follows the batch shape alone (round 6: the hint follows a concurrent kernel's
 * progress, and with it in that decision the log-probs of a batch depended on timing). */
VASR_API int vasr_set_busy_cus(vasr_handle* h, int cus);

/* ---- beam search (+ n-gram LM) ------------------------------------------------------------ */
/* BeamSearchDecoderWithLM.forward (beam_search_decoder.py:95-102 -> pyctcdecode, third-party: parity unpinned,
 * algorithm restated in oracle/beam_oracle.py).  Unlike the reference any batch size is accepted.
 *   d_logp [B][T'][V+1] f32 log-probabilities, blank = V (last class); space_id = index of ' ' in the labels
 *   -> d_ids [B][T'] i32 label ids of the best hypothesis (words separated by space_id), d_id_len [B] i32 (-1: the
 *      four-wavefront kernel's merge cells overflowed -- a prefix is reached by at most four pairs, so this cannot happen; it is
 *      reported instead of a wrong answer),
 *      d_score [B] f32 combined (acoustic + LM) natural-log score of that hypothesis.
 * beam_width <= 128, V+1 <= 128.  token_min_logp / beam_prune_logp: pyctcdecode defaults are -5 / -10. */
typedef struct vasr_lm vasr_lm;
VASR_API size_t vasr_beam_workspace_bytes(int batch, int64_t frames);
/* Compute units a search of `batch` utterances occupies while it runs: what a caller that overlaps the search with the next
 * acoustic pass hands to vasr_set_busy_cus().  Up to 64 utterances an utterance is searched by four wavefronts of a compute
 * unit of its own (`batch` units, for the shortest time); beyond that by one wavefront, four utterances per workgroup = per
 * compute unit (ceil(batch / 4) units).  Both forms give the same bits. */
VASR_API int vasr_beam_workgroups(int batch);
VASR_API int vasr_beam_search_f32(const float* d_logp, int batch, int64_t frames, int num_classes, int space_id,
                         int beam_width, float token_min_logp, float beam_prune_logp, const vasr_lm* lm,
                         int32_t* d_ids, int32_t* d_id_len, float* d_score, void* d_workspace,
                         size_t workspace_bytes, vasr_stream stream);
/* Same with a frame count per row: d_row_frames [B] i32 (device), row b is searched over its first
 * min(d_row_frames[b], frames) frames -- for batches of utterances of different lengths whose rows must come out as
 * batch-1 calls would (vasr_set_row_independent); NULL = all frames for every row (the call above). */
VASR_API int vasr_beam_search_rows_f32(const float* d_logp, const int32_t* d_row_frames, int batch, int64_t frames,
                              int num_classes, int space_id, int beam_width, float token_min_logp,
                              float beam_prune_logp, const vasr_lm* lm, int32_t* d_ids, int32_t* d_id_len,
                              float* d_score, void* d_workspace, size_t workspace_bytes, vasr_stream stream);
/* The n-best list, pyctcdecode's decode_beams (oracle/beam_oracle.py decode_beams): per row b the text groups of the final
 * beams whose combined score is >= best + beam_prune_logp, best first (exact ties: a fixed order that depends on the texts and
 * scores only), at most `nbest` of them, 1 <= nbest <= beam_width.  Slot s of row b:
 *   d_ids [B][nbest][frames] i32: ids row b * nbest + s, d_id_len [B][nbest] i32 (-1 in every slot of a row: the overflow of
 *   vasr_beam_search_rows_f32), d_logit_score / d_score [B][nbest] f64 the merged logit (acoustic) score and the combined
 *   (acoustic + LM) score; d_count [B] i32 the number of slots filled (>= 1).  Slots at or beyond the count get length 0 and
 *   scores -INFINITY; their ids are not written.  Slot 0 is vasr_beam_search_rows_f32's hypothesis: the same ids and length,
 *   and (float)d_score[b][0] is its score.  Workspace: vasr_beam_workspace_bytes; d_row_frames as above (NULL = all). */
VASR_API int vasr_beam_search_nbest_f32(const float* d_logp, const int32_t* d_row_frames, int batch, int64_t frames,
                               int num_classes, int space_id, int beam_width, int nbest, float token_min_logp,
                               float beam_prune_logp, const vasr_lm* lm, int32_t* d_ids, int32_t* d_id_len,
                               int32_t* d_count, double* d_logit_score, double* d_score, void* d_workspace,
                               size_t workspace_bytes, vasr_stream stream);
/* Back-off n-gram model as two open-addressing hash tables of 16-BYTE entries (one load returns key and value), both with
 * power-of-two capacity 2^lg >= 16, linear probing from the home slot ((uint32)(key ^ key >> 32) * 0x9E3779B1) >> (32 - lg),
 * key 0 = empty slot, stored keys have bit 0 set:
 *   h_vocab [vcap] {uint64 key, int32 word id, uint32 flags}: key = the word's label ids folded with vasr_beam_hash_step from
 *           vasr_beam_hash_init(), first character first; flags bit 0 = the word is in pyctcdecode's unigram set (below);
 *   h_ngram [ncap] {uint64 key, float log10 p, float log10 back-off}: the key of (w_1 .. w_n) folds the word ids from the
 *           LAST word backwards, hash_step(... hash_step(hash_step(init, w_n), w_{n-1}) ..., w_1) -- the keys of every suffix
 *           of a history then come out of one chain, and the kernel requests the whole back-off walk in one trip to memory.
 *   h_trie  [trie_buckets] buckets of TWO uint64 keys (16 bytes), trie_buckets a power of two >= 16, or NULL.
 *           pyctcdecode's build_ctcdecoder(labels, kenlm_model_path, alpha, beta) -- the reference's call,
 *           beam_search_decoder.py:82-87 -- behaves in one of two ways depending on the path's SUFFIX: for "*.arpa" it reads
 *           the file's unigrams (1-gram lines with a back-off field), keeps those the model knows (unigram_set) and builds a
 *           character trie of them: a partial word that is a prefix of a set member carries NO out-of-vocabulary penalty,
 *           and a committed word outside the set gets the unk offset even if the model knows it.  For any other suffix (the
 *           reference's own `3-gram-lm.binary`) there is no set: every partial word is penalised.
 *           h_trie = the trie's nodes: key = (label ids of a non-empty PREFIX of a set member folded like a word's) | 1, in its
 *           home bucket ((uint32)(key ^ key >> 32) * 0x9E3779B1) >> (32 - lg buckets) or the next one with a free cell (0);
 *           NULL = the no-unigram behaviour (also what an EMPTY unigram set amounts to).
 * Host arrays are copied to the device.  alpha/beta/unk_offset as in pyctcdecode's LanguageModel.  (ABI 6; ABI 5 had no
 * trie; ABI 4 took four parallel arrays with odd capacities and `key % cap`.) */
VASR_API int vasr_lm_create(const void* h_vocab, int vcap, const void* h_ngram, int ncap, const void* h_trie, int trie_buckets,
                   int order, int bos_id, int eos_id, int unk_id, float alpha, float beta, float unk_offset, vasr_lm** out);
VASR_API void vasr_lm_destroy(vasr_lm* lm);
VASR_API uint64_t vasr_beam_hash_init(void);
VASR_API uint64_t vasr_beam_hash_step(uint64_t h, uint64_t v);

/* ---- introspection -------------------------------------------------------------------- */
VASR_API const char* vasr_last_error(void);
VASR_API const char* vasr_version(void);
VASR_API int vasr_abi_version(void);
/* Algorithmic work of one call at (batch, samples): flops of the 1x1-conv GEMMs, flops and
 * minimum HBM bytes (read input + write output + weights, fp32) of the depthwise layers.
 * out[0]=pointwise_flops out[1]=depthwise_flops out[2]=depthwise_bytes out[3]=decoder_flops
 * out[4]=frontend_flops (2.5 N log2 N per frame + mel) */
VASR_API int vasr_algorithmic_work(const vasr_handle* h, int batch, int64_t samples, double out[5]);
/* Per-kernel-class timing with HIP events recorded on the launch stream (used by bench.py for the
 * roofline figures).  Between begin and end every launch of vasr_transcribe_greedy_f32 /
 * vasr_encoder_f32 / vasr_decoder_* is bracketed by an event pair; end() synchronises on the events
 * and returns the summed milliseconds and launch counts per class:
 *   [0] front end (seq_len + STFT/mel + CMVN)  [1] depthwise convs  [2] pointwise GEMMs
 *   [3] CTC head (decoder GEMM + log-softmax/argmax + collapse)  [4] fused depthwise + pointwise sub-blocks
 * flops / bytes (optional, may be NULL): the algorithmic work of the launches of each class that actually ran --
 * 2 M N K of every GEMM (class 2 and 4), HBM bytes read + written by every depthwise (1) and fused (4) layer, bytes STORED by
 * every plain GEMM (2: its store-only epilogue is the part of its time the matrix pipe does not bound). */
VASR_API int vasr_profile_begin(vasr_handle* h);
VASR_API int vasr_profile_end(vasr_handle* h, double ms[5], int64_t launches[5], double flops[5], double bytes[5]);
/* Row pitch of the library's padded activation buffers: frames rounded up to the 128-frame tile. */
VASR_API int64_t vasr_padded_frames(int64_t frames);

#ifdef __cplusplus
}
#endif
/* Measurement / development entry points (isolated layers, weight packers, bracket overhead) live in vasr_devtools.h and
 * are exported only by libvasr_hip_dev.so (-DVASR_DEVTOOLS); the product library has none of them and reads no
 * VASR_* tuning variable from the environment except VASR_GEMM and VASR_SLICES (the documented modes above). */
#endif /* VASR_H_ */
