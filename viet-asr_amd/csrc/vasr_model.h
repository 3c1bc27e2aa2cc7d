// The model behind a handle, shared by the host sources (vasr_api.cpp, model_build.cpp, encoder_run.cpp, vasr_devtools.cpp):
// layers, blocks, vasr_handle, the workspace plan, and the few functions that cross those files.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "vasr.h"
#include "vasr_host.h"
#include "vasr_internal.h"

namespace vasr {

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
};

struct ConvLayer {
  int cin = 0, cout = 0, kernel = 1, stride = 1, dilation = 1, pad = 0;
  int m_pad = 0;             // pointwise: rows of the packed weight (multiple of 128)
  float* d_w = nullptr;      // depthwise [C][K]; pointwise: MFMA A-fragment order (fp32)
  unsigned short* d_w3 = nullptr;  // pointwise: 3 x bf16 split fragments (encoder_pw_split.hip), when the shape allows
  unsigned short* d_w16 = nullptr; // pointwise: 2 x fp16 scaled split fragments, same condition
  float w16_inv = 1.f;             // 1 / (power-of-two scale of the fp16 pack)
  unsigned int* d_taps = nullptr;  // depthwise, Toeplitz / MFMA form: [C][tap_tsz] (hi | lo << 16) fp16 tap tables
  float* d_tap_inv = nullptr;      // [C] 1 / (power-of-two scale of the channel's taps)
  int tap_tsz = 0;
  float* d_ftaps = nullptr;        // depthwise, fused dw -> pw kernel (encoder_fused.hip): [C / 2][taps per pair][2]
  float f_l1 = 0.f;                // max_c sum_k |w[c][k]|: bound of the depthwise output per unit of input
  float* d_scale = nullptr;  // [m_pad]
  float* d_shift = nullptr;  // [m_pad]
  int step = -1;             // index in the MaskedConv1d length chain
  int conv_cin = 0;          // non-separable K-tap conv (implicit GEMM over k = tap * conv_cin + c; cin = kernel * conv_cin)
  int groups = 1;            // > 1: grouped conv + channel shuffle on the grouped split GEMM (PwArgs::groups); cin, conv_cin
                             // per group, split packs only (no fp32 pack: the fp32 mode runs SubBlock::pw_bd)
};

// squeeze-and-excitation (parts/jasper.py:152-168): fc.0 [hidden][c], fc.2 [c][hidden] (encoder_se.hip)
struct SeLayer {
  float* d_w1 = nullptr;
  float* d_w2 = nullptr;
  int c = 0, hidden = 0;
};

// GroupNorm (parts/jasper.py:385-391; encoder_norm.hip) after a convolution whose GEMM stores its raw output: gamma / beta
// and the group of every STORED channel (a grouped block stores them shuffled), members = the stored channels of each group
// in pre-shuffle order (d_gamma == nullptr: none -- BatchNorm, folded into the GEMM's epilogue)
struct NormLayer {
  float* d_gamma = nullptr;
  float* d_beta = nullptr;
  int32_t* d_group_of = nullptr;
  int32_t* d_members = nullptr;
  int c = 0, groups = 0;
};

struct SubBlock {
  bool separable = true;
  ConvLayer dw, pw;
  // pw grouped (pw.groups > 1): the same layer as a dense block-diagonal GEMM whose rows and BN are permuted by the channel
  // shuffle -- what the fp32 mode runs (encoder_pw.hip has no grouped form)
  ConvLayer pw_bd;
  SeLayer se;               // se and not residual: after this sub-layer (d_w1 == nullptr: none)
  NormLayer norm;           // GroupNorm of the conv's output (the GEMM then stores it raw)
};

// One 1x1 GEMM of a block's residual branch: the conv (+ its folded BatchNorm) of one source, then its GroupNorm and its
// SqueezeExcite where the block has them (parts/jasper.py:264-288, :428-441)
struct ResGemm {
  ConvLayer w;
  int pane_off = -1;        // the source: channels [pane_off, pane_off + w.cin) of the pane buffer; -1: the block input
  NormLayer norm;           // d_gamma == nullptr: none
  SeLayer se;               // d_w1 == nullptr: none
};

struct Block {
  vasr_block_desc d;
  std::vector<SubBlock> subs;
  bool has_res = false;
  // The residual GEMMs, summed (residual_mode max: combined by max) into the block's residual (build_encoder fills it, run_encoder
  // runs it in order).  One entry: a plain residual reads the block input, a res_pane0 one pane 0, a dense one (dense_panes
  // >= 2) channels [0, w.cin) of the pane buffer with w = [a_0 W_0 | a_1 W_1 | ...], scale 1, shift sum b_p.  With SE, GroupNorm
  // or max a dense residual cannot be summed before those: dense_panes entries, one per pane.
  std::vector<ResGemm> res;
  bool fused_res = false;   // the (single) residual GEMM folded into the last sub-block's GEMM (dual-source K): res is not run
  ConvLayer fused;          // weights [s1*W1 | s2*W2], scale 1, shift h1 + h2; cin = K1 + K2
  int fused_k1 = 0;
  int first_step = 0;
  // dense residual (residual_dense): the block's input is pane `pane` of its run's pane buffer [B][pane_c][ld] (-1: not
  // kept); dense_panes: the panes this block's residual reads (0: not a dense residual)
  int pane = -1, pane_off = 0, pane_c = 0, dense_panes = 0;
  bool keep_input = false;   // a later block of the run (or this one) reads this block's input as a pane
  // a residual block that is NOT dense right after a dense run receives the run's pane list and takes its (single) residual
  // from pane 0, the run's input, not from its own input (parts/jasper.py:428-436: res_out = xs[0])
  bool res_pane0 = false;
  // se (vasr_set_block_se): 0 = none, else the reduction ratio.  With residual, one SE per residual pane (res[p].se); the
  // residual then always takes the separate-GEMM form
  int se_r = 0;
  // groups / heads (vasr_set_block_groups): every main-branch conv grouped (groups > 1) and followed by a GroupShuffle; the
  // depthwise weights of a separable block shared by channel c % heads (heads > 0)
  int groups = 1, heads = 0;
  // norm_g (vasr_set_block_norm): 0 = BatchNorm (folded into the epilogues), else GroupNorm(norm_g, filters) after every conv
  // of the block: its GEMMs store raw output, each residual pane is its own GEMM normalized on its own (res[p].norm), and
  // the last sub-layer's normalization adds the residual sum and applies the output activation
  int norm_g = 0;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// Default 3 (2 x fp16 scaled split): against fp64 its error is not larger than mode 0's or mode 1's (K = 256 ... 1024,
// Gaussian / ReLU'd / 30-octave inputs), every reference fixture holds with the same tolerance, results stay independent
// of batch composition, at half the matrix work of mode 1 (QuartzNet15x5, 64 x 10 s: GEMMs 5.4 -> 3.7 ms per batch).
constexpr int kDefaultGemmMode = 3;
inline int parse_gemm_mode(const char* s) {
  if (!s) return kDefaultGemmMode;
  if (!strcmp(s, "fp32")) return 0;
  if (!strcmp(s, "bf16x3")) return 1;
  if (!strcmp(s, "bf16x2")) return 2;
  if (!strcmp(s, "f16x2")) return 3;
  return kDefaultGemmMode;
}
constexpr int kMaxSlices = 4;
constexpr int kAmaxTabs = 4;

inline int64_t conv_out_frames(int64_t t, const ConvLayer& c) {
  return (t + 2 * c.pad - (int64_t)c.dilation * (c.kernel - 1) - 1) / c.stride + 1;
}

// ---------------- workspace plan ----------------
struct WsPlan {
  size_t lens_tab, amax, se, norm, seq, melp, bufP, bufQ, bufD, bufR, bufS, pane, encp, logits, pred, total;
  int64_t T, Tp0, T1, Tp1;
  int amax_stride;   // slots per utterance of one maxima table (kAmaxTabs tables: [tab][B][amax_stride] u32)
};

// what a dry pass of run_encoder records: (kind, dst, src, src2, res) per launch, in buffer numbers (vasr_host.h)
struct PlanRec { std::vector<int32_t> v; };

}  // namespace vasr

struct vasr_handle {
  bool has_frontend = false, has_encoder = false, has_decoder = false, finalized = false;
  vasr_frontend_desc fe{};
  std::vector<float> fe_window, fe_fb;
  int feat_in = 0, dec_feat_in = 0, num_classes = 0;
  std::vector<vasr::Block> blocks;
  int pane_c_max = 0;   // channels of the dense-residual pane buffer (0: no dense residual GEMM)
  int se_c_max = 0;     // widest squeeze-and-excitation (0: the model has none)
  int norm_c_max = 0, norm_g_max = 0;   // widest GroupNorm, most groups (0: the model has none)
  // vasr_set_activation: the encoder's activation (kAct*) and residual_mode max (false: add)
  int act = vasr::kActRelu;
  bool res_max = false;
  // vasr_set_classifier: JasperDecoderForClassification in place of a CTC head (classify.hip)
  bool has_classifier = false;
  int cls_feat_in = 0, cls_classes = 0, cls_pool = 0;
  float* d_cls_w = nullptr;   // [cls_classes][cls_feat_in]
  float* d_cls_b = nullptr;   // [cls_classes]
  std::vector<vasr::LenStep> steps;
  std::map<std::string, vasr::HostTensor> weights;
  std::vector<void*> dev_allocs;
  // device tables
  vasr::FrontendTables ft{};
  vasr::LenStep* d_steps = nullptr;
  vasr::ConvLayer dec;
  int c_mid_max = 0, c_last = 0;
  // batch slicing across internal streams (vasr_set_slices)
  // measured on MI355X (QuartzNet15x5, B=64, 512x128 GEMM tiles pinned): 1 slice 7.35 ms, 2 slices 7.41 ms, 2 slices
  // phase-shifted by 40 / 100 / 300 us 7.39 / 7.34 / 7.68 ms -- the kernels of the two streams do not overlap in any
  // useful way (one workgroup per CU each), so slicing is OFF by default
  int slices = getenv("VASR_SLICES") ? atoi(getenv("VASR_SLICES")) : 1;
  bool slice_ready = false;
  bool plan_only = false;         // vasr_plan_buffers' host-side shadow of an unfinalized handle: upload() allocates nothing
  bool row_independent = false;   // vasr_set_row_independent
  int busy_cus = 0;               // vasr_set_busy_cus
  // vasr_set_feature_masks: borrowed device arrays, rectangles of the normalised features zeroed in front of the encoder
  // (spec_augment.hip); nullptr: the fused call is what it is without them
  const int32_t* mask_rects = nullptr;
  const int32_t* mask_row_begin = nullptr;
  vasr::DevSwitches sw = vasr::dev_switches();   // kernel-selection switches of the devtools build (vasr_internal.h); defaults in the product
  int n_cu = 256;                 // compute units of the device the handle was finalized on (tile-fill decisions)
  hipStream_t slice_stream[vasr::kMaxSlices] = {};
  hipEvent_t slice_done[vasr::kMaxSlices] = {}, slice_fork{};
  // 0 = v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chain), 1 = 3 x bf16 split operands on v_mfma_f32_32x32x16_bf16 (measured
  // max error against fp64 slightly LOWER than mode 0's: 3.6e-6 vs 4.7e-6 at K = 512), 2 = reduced 2 x bf16 (opt-in),
  // 3 = 2 x fp16 scaled split operands on v_mfma_f32_32x32x16_f16 (half the matrix work of mode 1, see vasr.h)
  int gemm_mode = vasr::parse_gemm_mode(getenv("VASR_GEMM"));
  // optional per-kernel-class HIP-event timing (vasr_profile_begin/end)
  bool profiling = false;
  struct ProfRec { hipEvent_t a, b; int cls; double flops, bytes; };
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> ev_pool;
};

struct vasr_lm {
  vasr::BeamLm view{};
  std::vector<void*> allocs;
};

namespace vasr {

// ---- model_build.cpp: vasr_create's pane layout, vasr_finalize's checks and table builders ----
int layout_dense_panes(vasr_handle* h);
int check_encoder(vasr_handle* h);
int check_classifier(const vasr_handle* h);
int build_frontend(vasr_handle* h);
int build_encoder(vasr_handle* h);
int build_decoder(vasr_handle* h);
int build_classifier(vasr_handle* h);

// ---- encoder_run.cpp: the workspace plan and the encoder / CTC-head passes ----
int64_t enc_frames(const vasr_handle* h, int64_t t);
WsPlan plan_ws(const vasr_handle* h, int batch, int64_t T);

// Brackets one launch (or a short launch group) with HIP events on the launch stream.
struct ProfScope {
  vasr_handle* h; hipStream_t st; hipEvent_t a{}, b{}; int cls; double flops, bytes;
  static hipEvent_t get(vasr_handle* h);
  ProfScope(vasr_handle* h_, int cls_, hipStream_t st_, double flops_ = 0.0, double bytes_ = 0.0);
  ~ProfScope();
};
enum { kProfFrontend = 0, kProfDepthwise = 1, kProfPointwise = 2, kProfHead = 3, kProfFused = 4 };

int run_encoder(vasr_handle* h, const float* x, int64_t x_ld, int64_t T, const int64_t* seq, int batch,
                float* out, int64_t out_ld, float* enc_len, char* ws, const WsPlan& p, hipStream_t st,
                AmaxTab* enc_amax = nullptr, const int64_t* wav_len = nullptr, const int32_t** own_frames = nullptr,
                bool chain_done = false, PlanRec* rec = nullptr);
int run_decoder(vasr_handle* h, const float* encp, int64_t ld, int64_t T1, int batch, float* logits, float* logp,
                int64_t* pred, hipStream_t st, AmaxTab enc_amax = AmaxTab{}, const int32_t* own_frames = nullptr);

// ---- vasr_api.cpp ----
int n_slices(const vasr_handle* h, int batch);
// rows [lo, hi) of slice i of n: lo = slice_bounds(batch, i, n), hi = slice_bounds(batch, i + 1, n)
inline int slice_bounds(int batch, int i, int n) { return (int)((int64_t)batch * i / n); }
// vasr_encoder_f32: block 0 reads the port tensor in place (the generic depthwise kernel copes with the unpadded pitch)
inline bool port_input_in_place(const vasr_handle* h) {
  const Block& b0 = h->blocks[0];
  return b0.subs[0].separable && !b0.has_res;
}

}  // namespace vasr
