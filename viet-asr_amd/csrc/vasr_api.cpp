// C ABI of libvasr_hip.so (see include/vasr.h): handle, weight intake, BN folding / packing,
// workspace planning and the launch sequences for each stage of the path.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <algorithm>
#include <vector>

#include "vasr.h"
#ifdef VASR_DEVTOOLS
#include "vasr_devtools.h"   // vasr_plan_buffers: the one devtools entry point that needs the handle's insides
#endif
#include "vasr_host.h"
#include "vasr_internal.h"

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

NormTables norm_tables(const float* gamma, const float* beta, int c, int G, int shuffle) {
  NormTables t{std::vector<float>(c), std::vector<float>(c), std::vector<int32_t>(c), std::vector<int32_t>(c)};
  const int cpg = c / G, mg = c / shuffle;
  for (int p = 0; p < c; ++p) {
    const int o = (p % mg) * shuffle + p / mg;
    t.gamma[o] = gamma[p];
    t.beta[o] = beta[p];
    t.group_of[o] = p / cpg;
    t.members[p] = o;
  }
  return t;
}

}  // namespace vasr

namespace {

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

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// Default 3 (2 x fp16 scaled split): against fp64 its error is not larger than mode 0's or mode 1's (K = 256 ... 1024,
// Gaussian / ReLU'd / 30-octave inputs), every reference fixture holds with the same tolerance, results stay independent
// of batch composition, at half the matrix work of mode 1 (QuartzNet15x5, 64 x 10 s: GEMMs 5.4 -> 3.7 ms per batch).
constexpr int kDefaultGemmMode = 3;
int parse_gemm_mode(const char* s) {
  if (!s) return kDefaultGemmMode;
  if (!strcmp(s, "fp32")) return 0;
  if (!strcmp(s, "bf16x3")) return 1;
  if (!strcmp(s, "bf16x2")) return 2;
  if (!strcmp(s, "f16x2")) return 3;
  return kDefaultGemmMode;
}
constexpr int kMaxSlices = 4;
constexpr int kAmaxTabs = 4;

}  // namespace

struct vasr_handle {
  bool has_frontend = false, has_encoder = false, has_decoder = false, finalized = false;
  vasr_frontend_desc fe{};
  std::vector<float> fe_window, fe_fb;
  int feat_in = 0, dec_feat_in = 0, num_classes = 0;
  std::vector<Block> blocks;
  int pane_c_max = 0;   // channels of the dense-residual pane buffer (0: no dense residual GEMM)
  int se_c_max = 0;     // widest squeeze-and-excitation (0: the model has none)
  int norm_c_max = 0, norm_g_max = 0;   // widest GroupNorm, most groups (0: the model has none)
  // vasr_set_activation: the encoder's activation (kAct*) and residual_mode max (false: add)
  int act = kActRelu;
  bool res_max = false;
  // vasr_set_classifier: JasperDecoderForClassification in place of a CTC head (classify.hip)
  bool has_classifier = false;
  int cls_feat_in = 0, cls_classes = 0, cls_pool = 0;
  float* d_cls_w = nullptr;   // [cls_classes][cls_feat_in]
  float* d_cls_b = nullptr;   // [cls_classes]
  std::vector<LenStep> steps;
  std::map<std::string, HostTensor> weights;
  std::vector<void*> dev_allocs;
  // device tables
  FrontendTables ft{};
  LenStep* d_steps = nullptr;
  ConvLayer dec;
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
  DevSwitches sw = dev_switches();   // kernel-selection switches of the devtools build (vasr_internal.h); defaults in the product
  int n_cu = 256;                 // compute units of the device the handle was finalized on (tile-fill decisions)
  hipStream_t slice_stream[kMaxSlices] = {};
  hipEvent_t slice_done[kMaxSlices] = {}, slice_fork{};
  // 0 = v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chain), 1 = 3 x bf16 split operands on v_mfma_f32_32x32x16_bf16 (measured
  // max error against fp64 slightly LOWER than mode 0's: 3.6e-6 vs 4.7e-6 at K = 512), 2 = reduced 2 x bf16 (opt-in),
  // 3 = 2 x fp16 scaled split operands on v_mfma_f32_32x32x16_f16 (half the matrix work of mode 1, see vasr.h)
  int gemm_mode = parse_gemm_mode(getenv("VASR_GEMM"));
  // optional per-kernel-class HIP-event timing (vasr_profile_begin/end)
  bool profiling = false;
  struct ProfRec { hipEvent_t a, b; int cls; double flops, bytes; };
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> ev_pool;
};

struct vasr_lm {
  BeamLm view{};
  std::vector<void*> allocs;
};

namespace {

template <class T>
int upload(vasr_handle* h, const std::vector<T>& v, T** out) {
  if (h->plan_only) {   // a host-side shadow: the pointer only says "this table exists", nothing ever reads through it
    alignas(16) static char no_table[16];
    *out = reinterpret_cast<T*>(no_table);
    return 0;
  }
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, std::max<size_t>(v.size() * sizeof(T), 16)));
  h->dev_allocs.push_back(p);
  HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = static_cast<T*>(p);
  return 0;
}

int same_pad(int k, int stride, int dil, int* pad) {
  // get_same_padding (parts/jasper.py:60-65)
  if (stride > 1 && dil > 1) return fail(VASR_ERR_INVALID, "Only stride OR dilation may be greater than 1");
  *pad = dil > 1 ? (dil * k) / 2 - 1 : k / 2;
  return 0;
}

int64_t conv_out_frames(int64_t t, const ConvLayer& c) {
  return (t + 2 * c.pad - (int64_t)c.dilation * (c.kernel - 1) - 1) / c.stride + 1;
}

const HostTensor* find(const vasr_handle* h, const std::string& key) {
  auto it = h->weights.find(key);
  return it == h->weights.end() ? nullptr : &it->second;
}

int need(const vasr_handle* h, const std::string& key, size_t numel, const HostTensor** out) {
  const HostTensor* t = find(h, key);
  if (!t) return fail(VASR_ERR_STATE, "missing weight '%s'", key.c_str());
  if (t->data.size() != numel)
    return fail(VASR_ERR_INVALID, "weight '%s' has %zu elements, expected %zu", key.c_str(), t->data.size(), numel);
  *out = t;
  return 0;
}

// eval-mode BatchNorm1d(eps=1e-3) -> y = x * alpha + beta  (parts/jasper.py:392)
int bn_affine(vasr_handle* h, const std::string& prefix, int c, std::vector<float>* alpha, std::vector<float>* beta) {
  const HostTensor *g, *b, *m, *v;
  int rc;
  if ((rc = need(h, prefix + ".weight", c, &g)) || (rc = need(h, prefix + ".bias", c, &b)) ||
      (rc = need(h, prefix + ".running_mean", c, &m)) || (rc = need(h, prefix + ".running_var", c, &v)))
    return rc;
  alpha->resize(c);
  beta->resize(c);
  for (int i = 0; i < c; ++i) {
    // same association as ATen's CPU eval path: alpha = w * invstd, beta = b - mean * alpha (fp32)
    const float invstd = 1.0f / std::sqrt(v->data[i] + 1e-3f);
    (*alpha)[i] = g->data[i] * invstd;
    (*beta)[i] = b->data[i] - m->data[i] * (*alpha)[i];
  }
  return 0;
}

int upload_affine(vasr_handle* h, const std::vector<float>& scale, const std::vector<float>& shift, ConvLayer* L) {
  const int rc = upload(h, scale, &L->d_scale);
  return rc ? rc : upload(h, shift, &L->d_shift);
}

// the BatchNorm under `prefix` as L's epilogue, padded to c_pad rows
// perm (optional): channel i's affine goes to row perm[i] (a grouped layer's block-diagonal form: the channel shuffle)
int fold_bn(vasr_handle* h, const std::string& prefix, int c, int c_pad, ConvLayer* L, const std::vector<int>* perm = nullptr) {
  std::vector<float> alpha, beta, sc(c_pad, 0.f), sh(c_pad, 0.f);
  if (int rc = bn_affine(h, prefix, c, &alpha, &beta)) return rc;
  for (int i = 0; i < c; ++i) {
    const int o = perm ? (*perm)[i] : i;
    sc[o] = alpha[i];
    sh[o] = beta[i];
  }
  return upload_affine(h, sc, sh, L);
}

// a normalized block's GEMMs store their raw output: scale 1, shift 0 (GroupNorm follows in encoder_norm.hip)
int unit_affine(vasr_handle* h, int c, int c_pad, ConvLayer* L) {
  std::vector<float> sc(c_pad, 0.f), sh(c_pad, 0.f);
  std::fill_n(sc.begin(), c, 1.f);
  return upload_affine(h, sc, sh, L);
}

// BatchNorm under `prefix` folded into L's epilogue, or (norm_g > 0) the unit affine of a layer GroupNorm follows
int conv_affine(vasr_handle* h, int norm_g, const std::string& prefix, int c, int c_pad, ConvLayer* L,
                const std::vector<int>* perm = nullptr) {
  return norm_g ? unit_affine(h, c, c_pad, L) : fold_bn(h, prefix, c, c_pad, L, perm);
}

// GroupNorm(G, c) under `prefix` (weight / bias [c]); shuffle: the groups of a grouped block's channel shuffle (1: none)
int load_norm(vasr_handle* h, const std::string& prefix, int c, int G, int shuffle, NormLayer* L) {
  const HostTensor *g, *b;
  int rc;
  if ((rc = need(h, prefix + ".weight", c, &g)) || (rc = need(h, prefix + ".bias", c, &b))) return rc;
  const NormTables t = norm_tables(g->data.data(), b->data.data(), c, G, shuffle);
  L->c = c;
  L->groups = G;
  h->norm_c_max = std::max(h->norm_c_max, c);
  h->norm_g_max = std::max(h->norm_g_max, G);
  if ((rc = upload(h, t.gamma, &L->d_gamma)) || (rc = upload(h, t.beta, &L->d_beta)) || (rc = upload(h, t.group_of, &L->d_group_of)))
    return rc;
  return upload(h, t.members, &L->d_members);
}

// the channel shuffle of a grouped block (parts/jasper.py:135-150): pre-shuffle channel p = g * (c / G) + j is stored at
// j * G + g
std::vector<int> shuffle_perm(int c, int G) {
  std::vector<int> perm(c);
  const int mg = c / G;
  for (int p = 0; p < c; ++p) perm[p] = (p % mg) * G + p / mg;
  return perm;
}

// The fragment packs of a row-major [cout][K] matrix into L (L->m_pad rows): split -- the 3 x bf16 and 2 x fp16 packs of the
// split GEMMs; fp32 -- the exact-fp32 kernel's pack
int upload_packs(vasr_handle* h, const float* w, int cout, int K, ConvLayer* L, bool fp32, bool split) {
  int rc;
  if (split) {
    std::vector<unsigned short> w3((size_t)K * L->m_pad * 3);
    pack_pointwise_weights_bf16x3(w, cout, K, L->m_pad, w3.data());
    if ((rc = upload(h, w3, &L->d_w3))) return rc;
    std::vector<unsigned short> w16((size_t)K * L->m_pad * 2);
    L->w16_inv = pack_pointwise_weights_f16x2(w, cout, K, L->m_pad, w16.data());
    if ((rc = upload(h, w16, &L->d_w16))) return rc;
  }
  if (!fp32) return 0;
  std::vector<float> wt((size_t)K * L->m_pad, 0.f);
  pack_pointwise_weights(w, cout, K, L->m_pad, wt.data());
  return upload(h, wt, &L->d_w);
}

// 1x1 convs + BNs over sources concatenated along K as ONE reduction:
//   sum_p BN_p(W_p x_p) = [a_0*W_0 | a_1*W_1 | ...] [x_0 ; x_1 ; ...] + sum_p b_p        (parts/jasper.py:428-439)
// Two sources: a JasperBlock's last sub-block GEMM and its residual GEMM (k1_split = K1 of the dual-source kernel); more:
// the panes of a dense residual (one source, the pane buffer; k1_split = 0).
struct SumSrc { std::string w_key, bn; int k; };
int pack_sum_1x1(vasr_handle* h, const std::vector<SumSrc>& src, int cout, int k1_split, ConvLayer* L) {
  int K = 0, rc;
  for (const SumSrc& s : src) K += s.k;
  L->cin = K;
  L->cout = cout;
  L->m_pad = (int)align_up(cout, 128);
  std::vector<float> w((size_t)cout * K), sc(L->m_pad, 1.f), sh(L->m_pad, 0.f);
  int off = 0;
  for (const SumSrc& s : src) {
    const HostTensor* ws;
    std::vector<float> a, b;
    if ((rc = need(h, s.w_key, (size_t)cout * s.k, &ws)) || (rc = bn_affine(h, s.bn, cout, &a, &b))) return rc;
    for (int m = 0; m < cout; ++m) {
      for (int k = 0; k < s.k; ++k) w[(size_t)m * K + off + k] = a[m] * ws->data[(size_t)m * s.k + k];
      sh[m] += b[m];
    }
    off += s.k;
  }
  if ((rc = upload_packs(h, w.data(), cout, K, L, true, pointwise_split_supported(L->m_pad, K, k1_split)))) return rc;
  return upload_affine(h, sc, sh, L);
}

// [cout][cin][kernel] -> the implicit GEMM's [cout][kernel * cin] (k = tap * cin + c) -> the three fragment packs (fp32: no
// fp32 pack)
int pack_conv_data(vasr_handle* h, const float* w, const std::string& key, int cout, int cin, int kernel, ConvLayer* L,
                   bool fp32 = true, bool split = true) {
  L->m_pad = (int)align_up(cout, 128);
  if (!conv_split_supported(L->m_pad, cin))
    return fail(VASR_ERR_UNSUPPORTED, "%s: in_channels %d of a %d-tap conv is not a multiple of 64", key.c_str(), cin, kernel);
  const int K = kernel * cin;
  L->cin = K;
  L->cout = cout;
  L->conv_cin = cin;
  std::vector<float> g((size_t)cout * K);
  pack_conv_gemm_weights(w, cout, cin, kernel, g.data());
  return upload_packs(h, g.data(), cout, K, L, fp32, split);
}

int pack_conv(vasr_handle* h, const std::string& key, int cout, int cin, int kernel, ConvLayer* L) {
  const HostTensor* w;
  int rc;
  if ((rc = need(h, key, (size_t)cout * cin * kernel, &w))) return rc;
  return pack_conv_data(h, w->data.data(), key, cout, cin, kernel, L);
}

// [cout][cin][1] -> MFMA A-fragment order (fp32: no fp32 pack)
int pack_pointwise_data(vasr_handle* h, const float* w, const std::string& key, int cout, int cin, ConvLayer* L,
                        bool fp32 = true, bool split = true) {
  // (a K depth of 32 would select the 128 x 256 tile of the fp32 kernel, whose last time tile assumes a 256-frame pitch)
  if (cin % 64) return fail(VASR_ERR_UNSUPPORTED, "%s: in_channels %d is not a multiple of 64", key.c_str(), cin);
  L->cin = cin;
  L->cout = cout;
  L->m_pad = (int)align_up(cout, 128);
  return upload_packs(h, w, cout, cin, L, fp32, split && pointwise_split_supported(L->m_pad, cin, 0));
}

int pack_pointwise(vasr_handle* h, const std::string& key, int cout, int cin, ConvLayer* L) {
  const HostTensor* w;
  int rc;
  if ((rc = need(h, key, (size_t)cout * cin, &w))) return rc;
  return pack_pointwise_data(h, w->data.data(), key, cout, cin, L);
}

// A grouped main-branch conv, weight [cout][cin / groups][kernel] under `key`, BN under `bn`, followed by the reference's
// GroupShuffle (parts/jasper.py:135-150, :396-399: output channel j * G + g = pre-shuffle channel g * (cout / G) + j).
//   BD: the block-diagonal dense form -- weight [cout][cin][kernel], zero outside each group's block, its rows and its folded
//       BN permuted by the shuffle, so that the dense kernels store the shuffled order directly (beside a grouped L: the fp32
//       pack only, for the fp32 mode);
//   L:  the grouped split GEMM's packs (L->groups = G; the [cout][kernel * cin / G] matrix, BN in pre-shuffle order) when
//       grouped_split_supported and not VASR_NO_GROUPED, else a copy of BD.
// conv: the implicit-GEMM form (a K-tap or strided conv), else a 1x1.
int pack_grouped(vasr_handle* h, const std::string& key, const std::string& bn, int cout, int cin, int kernel, int G, bool conv,
                 ConvLayer* L, ConvLayer* BD, int norm_g) {
  const HostTensor* w;
  int rc;
  const int cg = cin / G, mg = cout / G;
  if ((rc = need(h, key, (size_t)cout * cg * kernel, &w))) return rc;
  std::vector<float> dense((size_t)cout * cin * kernel, 0.f);
  const std::vector<int> perm = shuffle_perm(cout, G);
  for (int p = 0; p < cout; ++p) {
    const int g = p / mg, o = perm[p];
    for (int c = 0; c < cg; ++c)
      for (int t = 0; t < kernel; ++t)
        dense[((size_t)o * cin + g * cg + c) * kernel + t] = w->data[((size_t)p * cg + c) * kernel + t];
  }
  // grouped: BD only serves the fp32 mode -- its fp32 pack alone; else BD is the product form, every pack
  const bool grouped = !h->sw.no_grouped && grouped_split_supported(cout, cin, G);
  if ((rc = conv ? pack_conv_data(h, dense.data(), key, cout, cin, kernel, BD, true, !grouped)
                 : pack_pointwise_data(h, dense.data(), key, cout, cin, BD, true, !grouped)) ||
      (rc = conv_affine(h, norm_g, bn, cout, BD->m_pad, BD, &perm)))
    return rc;
  if (!grouped) {
    *L = *BD;
    *BD = ConvLayer{};
    return 0;
  }
  if ((rc = conv ? pack_conv_data(h, w->data.data(), key, cout, cg, kernel, L, false)
                 : pack_pointwise_data(h, w->data.data(), key, cout, cg, L, false)) ||
      (rc = conv_affine(h, norm_g, bn, cout, L->m_pad, L)))
    return rc;
  L->groups = G;
  return 0;
}

// ModuleList indices of block B's sub-layers (encoder.{i}.mconv.{j}) in the reference's construction order
// (parts/jasper.py:214-288, :329-400): per sub-layer its conv -- a separable one's depthwise conv, then the 1x1 at conv + 1 --,
// the BN, a GroupShuffle when groups > 1, activation + dropout except after the last sub-layer, and a SqueezeExcite when the
// block has SE and no residual.  The one place this arithmetic lives: weight checks, SE prefixes and build_encoder read it.
struct SubKeys { int conv, bn, se; };   // se = -1: none
std::vector<SubKeys> mconv_layout(const Block& B) {
  std::vector<SubKeys> out;
  int j = 0;
  for (int r = 0; r < B.d.repeat; ++r) {
    SubKeys k{j, j + (B.d.separable ? 2 : 1), -1};
    j = k.bn + 1 + (B.groups > 1 ? 1 : 0);
    if (r != B.d.repeat - 1) j += 2;
    if (B.se_r && !B.d.residual) k.se = j++;
    out.push_back(k);
  }
  return out;
}

// State-dict prefix of entry j of block i's main branch (mconv_layout), and of entry `entry` of its residual pane q's list:
// 0 the 1x1 conv, 1 its BatchNorm or GroupNorm, 2 its SqueezeExcite (parts/jasper.py:264-288)
std::string mconv_key(size_t i, int j) {
  char key[64];
  snprintf(key, sizeof key, "encoder.%zu.mconv.%d", i, j);
  return key;
}
std::string res_key(size_t i, int q, int entry) {
  char key[64];
  snprintf(key, sizeof key, "encoder.%zu.res.%d.%d", i, q, entry);
  return key;
}
// the 1x1 convs of block B's residual: one per pane a dense block sums, else one
int residual_panes(const Block& B) { return B.dense_panes >= 2 ? B.dense_panes : 1; }

// State-dict prefixes of block i's SqueezeExcite modules: with residual, entry 2 of every residual pane's list; without, the
// entry after each sub-layer's conv + BN (+ activation and dropout, except after the last one) -- which shifts the mconv
// indices of everything behind it
std::vector<std::string> se_prefixes(const vasr_handle* h, size_t i) {
  const Block& B = h->blocks[i];
  std::vector<std::string> out;
  if (!B.se_r) return out;
  if (B.d.residual) {
    for (int q = 0; q < residual_panes(B); ++q) out.push_back(res_key(i, q, 2));
    return out;
  }
  for (const SubKeys& k : mconv_layout(B)) out.push_back(mconv_key(i, k.se));
  return out;
}

// vasr_finalize's first check (before anything touches the device): every SE has a non-empty hidden layer, a width the
// kernels cover, and both of its weights
int check_se(vasr_handle* h) {
  for (size_t i = 0; i < h->blocks.size(); ++i) {
    const Block& B = h->blocks[i];
    if (!B.se_r) continue;
    const int c = B.d.filters, hid = c / B.se_r;
    if (hid == 0)
      return fail(VASR_ERR_INVALID, "block %zu: se_reduction_ratio %d leaves no hidden unit of %d channels", i, B.se_r, c);
    if (!se_supported(c, hid))
      return fail(VASR_ERR_UNSUPPORTED, "block %zu: squeeze-and-excitation over %d channels (at most 1024)", i, c);
    const HostTensor* t;
    int rc;
    for (const std::string& pre : se_prefixes(h, i))
      if ((rc = need(h, pre + ".fc.0.weight", (size_t)hid * c, &t)) || (rc = need(h, pre + ".fc.2.weight", (size_t)c * hid, &t)))
        return rc;
  }
  return 0;
}

// a weight present with exactly this shape (missing: VASR_ERR_STATE, any other shape: VASR_ERR_INVALID)
int need_shape(const vasr_handle* h, const std::string& key, std::initializer_list<int64_t> shape, const HostTensor** out) {
  const HostTensor* t = find(h, key);
  if (!t) return fail(VASR_ERR_STATE, "missing weight '%s'", key.c_str());
  if (!std::equal(t->shape.begin(), t->shape.end(), shape.begin(), shape.end())) {
    std::string want, got;
    for (int64_t d : shape) want += (want.empty() ? "" : ", ") + std::to_string(d);
    for (int64_t d : t->shape) got += (got.empty() ? "" : ", ") + std::to_string(d);
    return fail(VASR_ERR_INVALID, "weight '%s' has shape [%s], expected [%s]", key.c_str(), got.c_str(), want.c_str());
  }
  *out = t;
  return 0;
}

// vasr_finalize's check of groups / heads (before anything touches the device): nn.Conv1d's divisibility (C_in and C_out by
// groups), heads dividing the channels of a separable block (the reference's view(-1, heads, T); on a block that is not
// separable the reference never hands heads to a conv, and neither does this library), the encoder's width rule for grouped
// blocks (filters a multiple of 128, as build_encoder requires of every block), and every main-branch conv weight present
// in its grouped / shared shape under the key the shuffle entries shift it to
int check_groups(vasr_handle* h) {
  int cin = h->feat_in;
  for (size_t i = 0; i < h->blocks.size(); ++i) {
    const Block& B = h->blocks[i];
    const vasr_block_desc& d = B.d;
    const int G = B.groups, H = d.separable ? B.heads : 0, k = d.kernel % 2 ? d.kernel : d.kernel + 1;
    if (G > 1 || H > 0) {
      if (G > 1 && d.filters % 128)
        return fail(VASR_ERR_UNSUPPORTED, "block %zu: filters %d is not a multiple of 128", i, d.filters);
      const std::vector<SubKeys> lay = mconv_layout(B);
      int c = cin;
      const HostTensor* t;
      int rc;
      for (int r = 0; r < d.repeat; ++r) {
        if (c % G || d.filters % G)
          return fail(VASR_ERR_INVALID, "block %zu: groups %d does not divide in_channels %d and out_channels %d", i, G, c, d.filters);
        if (H > 0 && c % H)
          return fail(VASR_ERR_INVALID, "block %zu: heads %d does not divide the %d channels", i, H, c);
        const std::string key = mconv_key(i, lay[r].conv) + ".conv.weight";
        if (d.separable) {
          if ((rc = need_shape(h, key, {H > 0 ? H : c, 1, k}, &t)) ||
              (rc = need_shape(h, mconv_key(i, lay[r].conv + 1) + ".conv.weight", {d.filters, c / G, 1}, &t)))
            return rc;
        } else if ((rc = need_shape(h, key, {d.filters, c / G, k}, &t))) {
          return rc;
        }
        c = d.filters;
      }
    }
    cin = d.filters;
  }
  return 0;
}

// State-dict prefixes of block i's GroupNorms: each main-branch conv's norm entry (mconv_layout), then each residual pane's
// entry 1 (conv, norm (, SE))
std::vector<std::string> norm_prefixes(const vasr_handle* h, size_t i) {
  const Block& B = h->blocks[i];
  std::vector<std::string> out;
  for (const SubKeys& k : mconv_layout(B)) out.push_back(mconv_key(i, k.bn));
  if (B.d.residual)
    for (int q = 0; q < residual_panes(B); ++q) out.push_back(res_key(i, q, 1));
  return out;
}

// vasr_finalize's check of GroupNorm blocks (before anything touches the device): the group count divides the block's
// filters (nn.GroupNorm's ValueError), and every norm's weight and bias are there with shape [filters] -- both refusals
// VASR_ERR_INVALID
int check_norm(vasr_handle* h) {
  for (size_t i = 0; i < h->blocks.size(); ++i) {
    const Block& B = h->blocks[i];
    if (!B.norm_g) continue;
    const int c = B.d.filters;
    if (!norm_supported(c, B.norm_g))
      return fail(VASR_ERR_INVALID, "block %zu: norm_groups %d does not divide the %d channels", i, B.norm_g, c);
    for (const std::string& pre : norm_prefixes(h, i))
      for (const char* leaf : {".weight", ".bias"}) {
        const std::string key = pre + leaf;
        const HostTensor* t = find(h, key);
        if (!t) return fail(VASR_ERR_INVALID, "block %zu: missing GroupNorm weight '%s'", i, key.c_str());
        if (t->shape.size() != 1 || t->shape[0] != c)
          return fail(VASR_ERR_INVALID, "block %zu: GroupNorm weight '%s' is not of shape [%d]", i, key.c_str(), c);
      }
  }
  return 0;
}

int load_se(vasr_handle* h, const std::string& pre, int c, int ratio, SeLayer* L) {
  const HostTensor *w1, *w2;
  int rc;
  L->c = c;
  L->hidden = c / ratio;
  if ((rc = need(h, pre + ".fc.0.weight", (size_t)L->hidden * c, &w1)) || (rc = need(h, pre + ".fc.2.weight", (size_t)c * L->hidden, &w2)))
    return rc;
  if ((rc = upload(h, w1->data, &L->d_w1))) return rc;
  h->se_c_max = std::max(h->se_c_max, c);
  return upload(h, w2->data, &L->d_w2);
}

int build_frontend(vasr_handle* h) {
  const vasr_frontend_desc& fe = h->fe;
  const int nfft = fe.n_fft, nb = nfft / 2 + 1;
  std::vector<float> win(nfft, 0.f);
  const int off = (nfft - fe.win_length) / 2;  // torch.stft centres the window inside n_fft
  for (int i = 0; i < fe.win_length; ++i) win[off + i] = h->fe_window[i];
  std::vector<float> tw256(512), tw512(2 * 258, 0.f);
  for (int m = 0; m < 256; ++m) {
    tw256[2 * m] = (float)std::cos(-2.0 * M_PI * m / 256.0);
    tw256[2 * m + 1] = (float)std::sin(-2.0 * M_PI * m / 256.0);
  }
  for (int k = 0; k <= 256; ++k) {
    tw512[2 * k] = (float)std::cos(-2.0 * M_PI * k / 512.0);
    tw512[2 * k + 1] = (float)std::sin(-2.0 * M_PI * k / 512.0);
  }
  std::vector<float> mw((size_t)fe.n_mels * kMelTaps, 0.f);
  std::vector<int32_t> lo(fe.n_mels, 0);
  for (int f = 0; f < fe.n_mels; ++f) {
    const float* row = &h->fe_fb[(size_t)f * nb];
    int first = -1, last = -1;
    for (int k = 0; k < nb; ++k)
      if (row[k] != 0.f) { if (first < 0) first = k; last = k; }
    if (first < 0) { lo[f] = 0; continue; }
    if (last - first + 1 > kMelTaps)
      return fail(VASR_ERR_UNSUPPORTED, "mel filter %d spans %d bins (> %d)", f, last - first + 1, kMelTaps);
    lo[f] = first;
    for (int k = first; k <= last; ++k) mw[(size_t)f * kMelTaps + (k - first)] = row[k];
  }
  float *d_win, *d_t256, *d_t512, *d_mw;
  int32_t* d_lo;
  int rc;
  if ((rc = upload(h, win, &d_win)) || (rc = upload(h, tw256, &d_t256)) || (rc = upload(h, tw512, &d_t512)) ||
      (rc = upload(h, mw, &d_mw)) || (rc = upload(h, lo, &d_lo)))
    return rc;
  h->ft = FrontendTables{d_win, d_t256, d_t512, d_mw, d_lo, h->fe.log_guard_clamp ? 1 : 0};
  return 0;
}

int build_encoder(vasr_handle* h) {
  int cin = h->feat_in, step = 0, rc;
  h->steps.clear();
  h->c_mid_max = cin;
  for (size_t i = 0; i < h->blocks.size(); ++i) {
    Block& B = h->blocks[i];
    const vasr_block_desc& d = B.d;
    int k = d.kernel;
    if (k % 2 == 0) k += 1;  // compute_new_kernel_size (parts/jasper.py:52-57)
    int pad;
    if ((rc = same_pad(k, d.stride, d.dilation, &pad))) return rc;
    B.first_step = step;
    B.subs.resize(d.repeat);
    int c = cin;
    const std::vector<SubKeys> lay = mconv_layout(B);
    for (int r = 0; r < d.repeat; ++r) {
      SubBlock& S = B.subs[r];
      const int j = lay[r].conv;
      const std::string bn = mconv_key(i, lay[r].bn);
      S.separable = d.separable != 0;
      if (S.separable) {
        const HostTensor* w;
        if ((rc = need(h, mconv_key(i, j) + ".conv.weight", (size_t)(B.heads > 0 ? B.heads : c) * k, &w))) return rc;
        // heads: the [H][1][K] weight shared by channel c % H (MaskedConv1d's view(-1, heads, T)), expanded to [C][K] here so
        // that every depthwise kernel, tap table and the fused kernel's taps see per-channel weights
        std::vector<float> dw_heads;
        if (B.heads > 0) {
          dw_heads.resize((size_t)c * k);
          for (int ch = 0; ch < c; ++ch)
            std::copy_n(&w->data[(size_t)(ch % B.heads) * k], k, &dw_heads[(size_t)ch * k]);
        }
        const std::vector<float>& dwv = B.heads > 0 ? dw_heads : w->data;
        S.dw.cin = S.dw.cout = c;
        S.dw.kernel = k; S.dw.stride = d.stride; S.dw.dilation = d.dilation; S.dw.pad = pad;
        S.dw.step = step++;
        h->steps.push_back(LenStep{k, d.stride, d.dilation, pad});
        if ((rc = upload(h, dwv, &S.dw.d_w))) return rc;
        S.dw.tap_tsz = d.stride == 1 ? depthwise_mfma_table_size(k, d.dilation) : 0;
        if (S.dw.tap_tsz) {
          std::vector<unsigned int> tab((size_t)c * S.dw.tap_tsz);
          std::vector<float> inv(c);
          for (int ch = 0; ch < c; ++ch)
            inv[ch] = pack_depthwise_taps_f16x2(&dwv[(size_t)ch * k], k, d.dilation, S.dw.tap_tsz, &tab[(size_t)ch * S.dw.tap_tsz]);
          if ((rc = upload(h, tab, &S.dw.d_taps)) || (rc = upload(h, inv, &S.dw.d_tap_inv))) return rc;
        }
        if (fused_dwpw_supported(c, d.filters, k, d.stride, d.dilation)) {
          std::vector<float> ft((size_t)(c / 2) * fused_dwpw_taps_per_pair(k) * 2);
          S.dw.f_l1 = pack_fused_taps(dwv.data(), c, k, ft.data());
          if ((rc = upload(h, ft, &S.dw.d_ftaps))) return rc;
        }
        const std::string key = mconv_key(i, j + 1) + ".conv.weight";
        if (B.groups > 1) {
          if ((rc = pack_grouped(h, key, bn, d.filters, c, 1, B.groups, false, &S.pw, &S.pw_bd, B.norm_g))) return rc;
        } else if ((rc = pack_pointwise(h, key, d.filters, c, &S.pw))) {
          return rc;
        }
        S.pw.step = step++;
        h->steps.push_back(LenStep{1, 1, 1, 0});
      } else {
        const std::string key = mconv_key(i, j) + ".conv.weight";
        const bool conv = !(k == 1 && d.stride == 1);   // K-tap / strided: implicit GEMM (encoder_pw_split.hip, encoder_pw.hip CONV)
        if (B.groups > 1) {
          if ((rc = pack_grouped(h, key, bn, d.filters, c, k, B.groups, conv, &S.pw, &S.pw_bd, B.norm_g))) return rc;
        } else if ((rc = conv ? pack_conv(h, key, d.filters, c, k, &S.pw) : pack_pointwise(h, key, d.filters, c, &S.pw))) {
          return rc;
        }
        if (conv) {
          S.pw.kernel = k; S.pw.stride = d.stride; S.pw.dilation = d.dilation; S.pw.pad = pad;
          h->steps.push_back(LenStep{k, d.stride, d.dilation, pad});
        } else {
          h->steps.push_back(LenStep{1, 1, 1, 0});
        }
        S.pw.step = step++;
      }
      // (pack_grouped has folded a grouped layer's BN, in both of its forms)
      if (B.groups == 1 && (rc = conv_affine(h, B.norm_g, bn, d.filters, S.pw.m_pad, &S.pw))) return rc;
      if (S.pw_bd.d_w) {          // the block-diagonal form runs the same geometry
        S.pw_bd.kernel = S.pw.kernel; S.pw_bd.stride = S.pw.stride; S.pw_bd.dilation = S.pw.dilation; S.pw_bd.pad = S.pw.pad;
        S.pw_bd.step = S.pw.step;
      }
      // GroupNorm entry, before the GroupShuffle: its channels are stored shuffled
      if (B.norm_g && (rc = load_norm(h, bn, d.filters, B.norm_g, B.groups, &S.norm))) return rc;
      // SqueezeExcite entry (parts/jasper.py:233-234, :250-251)
      if (lay[r].se >= 0 && (rc = load_se(h, mconv_key(i, lay[r].se), d.filters, B.se_r, &S.se))) return rc;
      c = d.filters;
    }
    B.has_res = d.residual != 0;
    // with SE or GroupNorm a dense residual's panes cannot be summed before those, so each pane is its own GEMM (max mode: the
    // panes are combined by max, which one GEMM over all of them cannot do)
    const bool per_pane = (B.se_r || B.norm_g || h->res_max) && B.dense_panes >= 2;
    if (B.has_res && B.dense_panes >= 2 && !per_pane) {
      // dense residual: one GEMM over the run's first dense_panes panes (parts/jasper.py:428-439 for each pane)
      std::vector<SumSrc> src;
      for (int q = 0; q < B.dense_panes; ++q)
        src.push_back(SumSrc{res_key(i, q, 0) + ".conv.weight", res_key(i, q, 1), h->blocks[i - B.dense_panes + 1 + q].pane_c});
      for (const SumSrc& s : src)
        if (s.k % 64) return fail(VASR_ERR_UNSUPPORTED, "%s: in_channels %d is not a multiple of 64", s.w_key.c_str(), s.k);
      B.res.resize(1);
      B.res[0].pane_off = 0;
      if ((rc = pack_sum_1x1(h, src, d.filters, 0, &B.res[0].w))) return rc;
    } else if (B.has_res) {
      B.res.resize(residual_panes(B));
      for (int q = 0; q < (int)B.res.size(); ++q) {
        ResGemm& G = B.res[q];
        int k2 = cin;
        if (per_pane) {
          const Block& P = h->blocks[i - B.dense_panes + 1 + q];
          k2 = P.pane_c;
          G.pane_off = P.pane_off;
        } else if (B.res_pane0) {
          G.pane_off = 0;
        }
        // conv, its BN or GroupNorm (not grouped, not shuffled), its SE
        if ((rc = pack_pointwise(h, res_key(i, q, 0) + ".conv.weight", d.filters, k2, &G.w)) ||
            (rc = conv_affine(h, B.norm_g, res_key(i, q, 1), d.filters, G.w.m_pad, &G.w)) ||
            (B.norm_g && (rc = load_norm(h, res_key(i, q, 1), d.filters, B.norm_g, 1, &G.norm))) ||
            (B.se_r && (rc = load_se(h, res_key(i, q, 2), d.filters, B.se_r, &G.se))))
          return rc;
      }
      // fold the residual branch into the last sub-block's GEMM when both reductions tile evenly
      const SubBlock& last = B.subs.back();
      const int k1 = last.pw.cin, k2 = cin;
      const int chunk = d.filters % 512 == 0 ? 128 : (d.filters % 256 == 0 ? 64 : 32);
      // (grouped blocks: the main branch's grouped reduction and the residual's dense one share no K)
      if (d.stride == 1 && k1 % chunk == 0 && k2 % chunk == 0 && h->sw.fused_residual && !last.pw.conv_cin &&
          !B.res_pane0 && !B.se_r && B.groups == 1 && !B.norm_g && !h->res_max) {   // (the fold sums: add mode only)
        const SumSrc s1{mconv_key(i, lay.back().conv + (last.separable ? 1 : 0)) + ".conv.weight", mconv_key(i, lay.back().bn), k1};
        const SumSrc s2{res_key(i, 0, 0) + ".conv.weight", res_key(i, 0, 1), k2};
        if ((rc = pack_sum_1x1(h, {s1, s2}, d.filters, k1, &B.fused))) return rc;
        B.fused_res = true;
        B.fused_k1 = k1;
      }
    }
    if (d.filters % 128)
      return fail(VASR_ERR_UNSUPPORTED, "block %zu: filters %d is not a multiple of 128", i, d.filters);
    cin = d.filters;
    // mid-pipeline buffers hold every block output but the last one, a last-block residual, and the sub-layer outputs (and
    // their depthwise outputs in D) inside a last block of more than one sub-layer: only the last sub-layer of the last
    // block writes the encoder output directly
    if ((i + 1 < h->blocks.size() || B.has_res || B.subs.size() > 1) && cin > h->c_mid_max) h->c_mid_max = cin;
  }
  h->c_last = cin;
  return upload(h, h->steps, &h->d_steps);
}

int build_decoder(vasr_handle* h) {
  int rc;
  if ((rc = pack_pointwise(h, "decoder_layers.0.weight", h->num_classes, h->dec_feat_in, &h->dec))) return rc;
  const HostTensor* b;
  if ((rc = need(h, "decoder_layers.0.bias", h->num_classes, &b))) return rc;
  std::vector<float> sc(h->dec.m_pad, 1.f), sh(h->dec.m_pad, 0.f);
  for (int i = 0; i < h->num_classes; ++i) sh[i] = b->data[i];
  return upload_affine(h, sc, sh, &h->dec);
}

// vasr_finalize's check of the classification head (before anything touches the device): it reads what the encoder writes, and
// both of its weights are there -- the Linear's [num_classes][feat_in] and [num_classes]
int check_classifier(const vasr_handle* h) {
  if (h->has_encoder && h->blocks.back().d.filters != h->cls_feat_in)
    return fail(VASR_ERR_INVALID, "classifier feat_in %d, the encoder's last block has %d filters", h->cls_feat_in,
                h->blocks.back().d.filters);
  const HostTensor* t;
  int rc;
  if ((rc = need_shape(h, "decoder_layers.0.weight", {h->cls_classes, h->cls_feat_in}, &t))) return rc;
  return need_shape(h, "decoder_layers.0.bias", {h->cls_classes}, &t);
}

int build_classifier(vasr_handle* h) {
  int rc;
  if ((rc = upload(h, find(h, "decoder_layers.0.weight")->data, &h->d_cls_w))) return rc;
  return upload(h, find(h, "decoder_layers.0.bias")->data, &h->d_cls_b);
}

// ---------------- workspace plan ----------------
struct WsPlan {
  size_t lens_tab, amax, se, norm, seq, melp, bufP, bufQ, bufD, bufR, bufS, pane, encp, logits, pred, total;
  int64_t T, Tp0, T1, Tp1;
  int amax_stride;   // slots per utterance of one maxima table (kAmaxTabs tables: [tab][B][amax_stride] u32)
};

int64_t enc_frames(const vasr_handle* h, int64_t t) {
  for (const Block& B : h->blocks)
    for (const SubBlock& S : B.subs) t = conv_out_frames(t, S.separable ? S.dw : S.pw);
  return t;
}

WsPlan plan_ws(const vasr_handle* h, int batch, int64_t T) {
  WsPlan p{};
  p.T = T;
  p.Tp0 = pad_frames(T);
  p.T1 = h->has_encoder ? enc_frames(h, T) : T;
  // the first (strided) block may still run at T frames inside: size by the larger pitch
  p.Tp1 = pad_frames(p.T1);
  const int64_t tp_mid = h->has_encoder ? pad_frames(conv_out_frames(T, h->blocks[0].subs[0].separable
                                                                          ? h->blocks[0].subs[0].dw
                                                                          : h->blocks[0].subs[0].pw))
                                        : p.Tp1;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
  p.lens_tab = take((h->steps.size() + 2) * (size_t)batch * 4);   // + the row-independent frame counts
  // maxima tables of the fp16-split arithmetic (AmaxTab): in flight at any time are the block input's, the current
  // kernel's input's and its output's -- kAmaxTabs = 4 rotate.  Capacity: the most slots any producer may use.
  p.amax_stride = 64;
  if (h->has_encoder) {
    int64_t t = T;
    for (const Block& B : h->blocks)
      for (const SubBlock& S : B.subs) {
        if (S.separable) {
          t = conv_out_frames(t, S.dw);
          p.amax_stride = std::max(p.amax_stride, depthwise_amax_slots(S.dw.cin, pad_frames(t)));
        } else if (S.pw.conv_cin) {
          t = conv_out_frames(t, S.pw);
          p.amax_stride = std::max(p.amax_stride, 256);   // launch_amax: the maxima of an encoder input no kernel published
        }
        p.amax_stride = std::max(p.amax_stride, pointwise_amax_slots(S.pw.m_pad, pad_frames(t)));
      }
    if (h->pane_c_max) p.amax_stride = std::max(p.amax_stride, 256);   // launch_amax over the pane buffer
    if (h->se_c_max) p.amax_stride = std::max(p.amax_stride, 256);     // launch_se republishes up to 256 slots
    if (h->norm_c_max) p.amax_stride = std::max(p.amax_stride, 256);   // launch_norm too
  }
  p.amax = take((size_t)kAmaxTabs * batch * p.amax_stride * 4);
  p.se = take((size_t)2 * batch * h->se_c_max * 4);   // SE row sums and scales, [B][c] each
  // GroupNorm row means and M2 [B][c] each, group means and 1 / std [B][G] each
  p.norm = take((size_t)2 * batch * (h->norm_c_max + h->norm_g_max) * 4);
  p.seq = take((size_t)batch * 8);
  p.melp = take((size_t)batch * (h->has_encoder ? h->feat_in : 64) * p.Tp0 * 4);
  const size_t mid = (size_t)batch * h->c_mid_max * std::max(tp_mid, p.Tp1) * 4;
  p.bufP = take(h->has_encoder ? mid : 0);
  p.bufQ = take(h->has_encoder ? mid : 0);
  p.bufD = take(h->has_encoder ? mid : 0);
  p.bufR = take(h->has_encoder ? mid : 0);
  p.bufS = take(h->has_encoder ? mid : 0);
  // dense-residual panes [B][pane_c_max][ld]: ld = the pitch of the run's first block input, which every block of the run
  // keeps (no stride inside a run; run_encoder checks it)
  p.pane = take(h->pane_c_max ? (size_t)batch * h->pane_c_max * std::max({p.Tp0, tp_mid, p.Tp1}) * 4 : 0);
  const int c_enc = h->has_encoder ? h->c_last : h->dec_feat_in;
  p.encp = take((size_t)batch * c_enc * p.Tp1 * 4);
  p.logits = take(h->has_decoder ? (size_t)batch * h->num_classes * p.Tp1 * 4 : 0);
  p.pred = take((size_t)batch * p.T1 * 8);
  p.total = o;
  return p;
}

// Brackets one launch (or a short launch group) with HIP events on the launch stream.
struct ProfScope {
  vasr_handle* h; hipStream_t st; hipEvent_t a{}, b{}; int cls; double flops, bytes;
  static hipEvent_t get(vasr_handle* h) {
    hipEvent_t e;
    if (!h->ev_pool.empty()) { e = h->ev_pool.back(); h->ev_pool.pop_back(); return e; }
    if (hipEventCreate(&e) != hipSuccess) e = nullptr;   // a null event makes the record / elapsed calls fail loudly
    return e;
  }
  // Single-launch classes (depthwise, pointwise) hand the event pair to the launch itself (g_probe: the dispatch
  // packet's begin / end timestamps); multi-launch groups (front end, head) are bracketed on the stream.
  // flops / bytes: the ALGORITHMIC work of the bracketed launch (2 M N K of a GEMM; read x + write y of a depthwise or
  // fused layer), summed per class by vasr_profile_end so that a rate is always work-that-ran over time-it-took
  ProfScope(vasr_handle* h_, int cls_, hipStream_t st_, double flops_ = 0.0, double bytes_ = 0.0)
      : h(h_), st(st_), cls(cls_), flops(flops_), bytes(bytes_) {
    if (!h->profiling) return;
    a = get(h); b = get(h);
    if (cls == 1 || cls == 2 || cls == 4) g_probe = LaunchProbe{a, b};
    else (void)hipEventRecord(a, st);
  }
  ~ProfScope() {
    if (!h->profiling) return;
    if (cls == 1 || cls == 2 || cls == 4) {
      if (g_probe.start) {   // no instrumented launch happened inside the scope
        g_probe = LaunchProbe{};
        (void)hipEventRecord(a, st);
        (void)hipEventRecord(b, st);
      }
    } else {
      (void)hipEventRecord(b, st);
    }
    h->prof.push_back({a, b, cls, flops, bytes});
  }
};
enum { kProfFrontend = 0, kProfDepthwise = 1, kProfPointwise = 2, kProfHead = 3, kProfFused = 4 };

// GEMM dispatch: exact-fp32 MFMA kernel, or the 3 x bf16 split kernel when selected and the layer has that pack.
// Returns 1 when the launch published a.amax_y (only the split kernel does), 0 when not, < 0 on error.
// dry (vasr_plan_buffers): nothing is launched, the return value is the one the launch would give.
int run_pointwise(vasr_handle* h, PwArgs& a, const ConvLayer& W, hipStream_t st, bool dry = false) {
  if (dry) return h->gemm_mode >= 1 && W.d_w3 && a.amax_y.p != nullptr ? 1 : 0;
  if (h->gemm_mode >= 1 && W.d_w3) {
    int arith = h->gemm_mode == 2 ? 1 : 0;
    a.wt = reinterpret_cast<const float*>(W.d_w3);
    // fp16 split: needs the maxima of every source this GEMM reads; a source without them keeps the 3 x bf16 form
    if (h->gemm_mode == 3 && W.d_w16 && a.amax_x.p && (!a.x2 || a.amax_x2.p)) {
      arith = 2;
      a.wt = reinterpret_cast<const float*>(W.d_w16);
      a.w_inv_scale = W.w16_inv;
    }
    const int e = launch_pointwise_split(a, arith, st, &a.amax_y.n);
    if (e) return fail(VASR_ERR_HIP, "pointwise GEMM: %s", hipGetErrorString((hipError_t)e));
    return a.amax_y.p != nullptr ? 1 : 0;
  }
  a.wt = W.d_w;
  launch_pointwise(a, st);
  return 0;
}

// pw_args (vasr_host.h) of layer W's fp32 pack (run_pointwise picks the pack that runs) over a padded internal tensor
PwArgs pw_args(const vasr_handle* h, const ConvLayer& W, const float* x, float* y, int64_t ld, int64_t frames, int batch) {
  PwArgs a = vasr::pw_args(W.d_w, W.d_scale, W.d_shift, W.m_pad, W.cin, x, y, ld, frames, batch);
  a.busy_cus = h->busy_cus;
  return a;
}

// Whether a 256-channel separable sub-block of a batch [B][256][ld] takes the fused depthwise -> pointwise kernel
// (encoder_fused.hip), and on which tile: 128 or 64 frames per workgroup, 0 = depthwise and GEMM as two kernels.  It does when
// there are enough 128-frame tiles to fill the chip (one workgroup per tile, all channels); VASR_FUSED=0 is the A/B switch.
int fused_tile_cols(const vasr_handle* h, int batch, int64_t ld) {
  if (!h->sw.fused) return 0;
  // One workgroup per CU (159 KB of LDS), one 128-frame tile each: it pays when the tiles fill whole rounds of the chip
  // (measured, fused vs two kernels: 64 x 10 s = 256 tiles -3.4 % per step, 512 x 30 s = 6144 tiles -4 %; but 32 x 10 s = 128
  // tiles +2.6 %, 64 x 10.3 s = 320 tiles = 1.25 rounds +3 %, 16 x 10 s = 64 tiles +4.6 %).  Smaller batches take the kernel's
  // 64-frame form (round 4) while THOSE tiles fit one round and occupy at least 3/8 of the chip -- 12 to 32 utterances of
  // 10 s; measured against two kernels, ms per step: 15x5 B = 12 / 16 / 20 / 24 / 32: -3.8 / -4.8 / -8.3 / -7.7 / -6.7 %, 12x1
  // (BASELINE configs[1]) B = 16 / 20 / 24 / 32: -3.1 / -5.1 / -5.0 / -4.3 %; B = 8: +-0; B = 1-4: +5 ... +9 % (one tile is 14 us
  // of latency against 4 + 7 us for the two kernels spread over the chip); 36-44 utterances (1.1-1.4 rounds): +0.8 ... +1.6 %.
  const int fused_min_tiles = h->sw.fused_min_tiles, fused_tile = h->sw.fused_tile;
  const int n_cu = h->n_cu;
  // (units a concurrent kernel of the caller's holds -- the overlapped beam search -- take no workgroups: 256 tiles on the
  // 192 CUs a 64-utterance search leaves free are 1.33 rounds)
  const int f_cus = h->busy_cus > 0 && h->busy_cus < n_cu - 32 ? n_cu - h->busy_cus : n_cu;
  const int64_t f_tiles = (int64_t)batch * (ld / kTimeTile);
  // WHETHER a sub-block is fused is a function of the batch's shape ALONE (the whole chip's unit count): the fused and the
  // two-kernel form round differently, and the busy-unit hint follows a concurrent kernel's progress -- with the hint in this
  // decision the log-probs of one and the same batch depended on whether the previous search had finished (round 6,
  // tests/devtools/stress_beam_overlap.py: 196 of 11 594 overlapped batches differed from their serial run).  The hint only
  // picks the TILE WIDTH of a sub-block that is fused anyway: 64- and 128-frame tiles give the same bits.
  const int f_rule = fused_tile_choice(f_tiles, n_cu);
  int f_auto = f_rule ? f_rule : 128;
  if (f_rule && f_cus < n_cu) {
    // lock-stepped rounds on the free units: a 64-frame tile costs ~0.6 of a 128-frame one (17 vs 29.7 us a round); 256 tiles on
    // the 192 units a 64-utterance search leaves: 2 rounds of 128 frames = 2.0 against 3 rounds of 64 = 1.8
    const int64_t r128 = (f_tiles + f_cus - 1) / f_cus, r64 = (2 * f_tiles + f_cus - 1) / f_cus;
    f_auto = 0.6 * (double)r64 < (double)r128 ? 64 : 128;
  }
  const bool f_fill = fused_min_tiles > 0 ? f_tiles >= fused_min_tiles : (fused_tile ? f_rule == fused_tile : f_rule != 0);
  if (!f_fill) return 0;
  return fused_tile == 64 || fused_tile == 128 ? fused_tile : f_auto;
}

// Encoder over an input [B][feat_in][x_ld]; writes [B][c_last][out_ld] (T1 valid frames).
// enc_amax (optional): receives the maxima table of the encoder output when one was published (fp16-split mode, padded
// output pitch), for the CTC head of the fused path; the table lives in the workspace until the next encoder pass.
// rec (vasr_plan_buffers): a dry pass -- nothing is launched and no device memory is touched, every launch the pass would
// make is recorded as (kind, dst, src, src2, res) in buffer numbers (vasr_host.h); ws is then any base address.
struct PlanRec { std::vector<int32_t> v; };
int run_encoder(vasr_handle* h, const float* x, int64_t x_ld, int64_t T, const int64_t* seq, int batch,
                float* out, int64_t out_ld, float* enc_len, char* ws, const WsPlan& p, hipStream_t st,
                AmaxTab* enc_amax = nullptr, const int64_t* wav_len = nullptr, const int32_t** own_frames = nullptr,
                bool chain_done = false, PlanRec* rec = nullptr) {
  const bool dry = rec != nullptr;
  int32_t* lens_tab = reinterpret_cast<int32_t*>(ws + p.lens_tab);
  auto lens = [&](int step) { return lens_tab + (size_t)step * batch; };
  // row-independent mode (fused path): everything the CTC head sees of a row must depend on that row alone, also the
  // fp16 scale of its input -- the encoder output's maxima are then taken over the frames an unbatched call on the row
  // would produce, and the head zeroes the columns behind them (they are not decoded in this mode)
  const bool own = h->row_independent && wav_len != nullptr;
  // (the fused path has run the chain as extra workgroups of its normalisation launch: launch_normalize_chain)
  if (!chain_done && !dry)
    launch_len_chain(seq, batch, h->d_steps, (int)h->steps.size(), lens_tab, enc_len, st, own ? wav_len : nullptr,
                     h->fe.hop_length, (int)p.T1);
  const int32_t* own_tab = own ? lens((int)h->steps.size() + 1) : nullptr;
  if (own_frames) *own_frames = own_tab;
  float* bufs[4] = {reinterpret_cast<float*>(ws + p.bufP), reinterpret_cast<float*>(ws + p.bufQ),
                    reinterpret_cast<float*>(ws + p.bufR), reinterpret_cast<float*>(ws + p.bufS)};
  float* D = reinterpret_cast<float*>(ws + p.bufD);
  // Where the sub-block outputs go (vasr_host.h BufRotation), and the check every launch passes before it is made: its
  // destination is none of its own sources, not the live block input, not the live R, not the pane buffer
  BufRotation rot;
  rot.inplace = h->sw.buf_inplace;
  const float* pane_lo = reinterpret_cast<const float*>(ws + p.pane);
  const float* pane_hi = reinterpret_cast<const float*>(ws + p.encp);
  auto buf_of = [&](const float* q) -> int {
    if (!q) return kBufNone;
    for (int i = 0; i < kBufRot; ++i) if (q == bufs[i]) return i;
    if (q == D) return kBufD;
    if (q == out) return kBufOut;
    if (q == x) return kBufIn;
    return h->pane_c_max && q >= pane_lo && q < pane_hi ? kBufPane : kBufNone;
  };
  auto check_dst = [&](int kind, const float* dst, const float* sx, const float* sx2, const float* sr) -> int {
    const int d = buf_of(dst), a = buf_of(sx), b = buf_of(sx2), r = buf_of(sr);
    if (const char* why = rot.refuse(kind, d, a, b, r))
      return fail(VASR_ERR_STATE, "encoder buffers: %s (launch kind %d: dst %d, src %d, src2 %d, res %d)", why, kind, d, a, b, r);
    return 0;
  };
  auto commit = [&](int kind, const float* dst, const float* sx, const float* sx2, const float* sr) {
    const int d = buf_of(dst), a = buf_of(sx), b = buf_of(sx2), r = buf_of(sr);
    rot.launched(d, a, b, r);
    if (rec) rec->v.insert(rec->v.end(), {kind, d, a, b, r});
  };
  auto note = [&](int kind, const float* dst, const float* sx, const float* sx2, const float* sr) -> int {
    if (int rc = check_dst(kind, dst, sx, sx2, sr)) return rc;
    commit(kind, dst, sx, sx2, sr);
    return 0;
  };
  // the rotation buffer the next sub-block output goes to (over_cur: the launch does not read the current tensor)
  auto next_dst = [&](bool over_cur) -> float* {
    const int d = rot.pick(over_cur);
    return d >= 0 ? bufs[d] : nullptr;   // (nullptr: no dead buffer -- check_dst refuses it)
  };
  const float* cur = x;
  int64_t cur_ld = x_ld, cur_T = T;
  // fp16-split GEMMs: maxima rows, indexed by the length-chain step of the conv that produced the tensor
  const bool want_amax = h->gemm_mode == 3;
  unsigned int* amax_base = reinterpret_cast<unsigned int*>(ws + p.amax);
  AmaxTab cur_amax{}, blk_amax{};   // maxima of `cur` / of the block input over each utterance's valid frames (p == nullptr: not known)
  // a table that neither the block input's nor the current tensor's maxima live in (the third candidate is always free)
  auto free_tab = [&](const AmaxTab& also_busy) {
    for (int i = 0; i < kAmaxTabs; ++i) {
      unsigned int* q = amax_base + (size_t)i * batch * p.amax_stride;
      if (q != cur_amax.p && q != blk_amax.p && q != also_busy.p) return AmaxTab{q, p.amax_stride, 0};
    }
    return AmaxTab{};
  };
  int64_t pane_ld = 0;   // pitch of the current dense run's panes: its first block's input pitch
  // squeeze-and-excitation of a tensor [B][L.c][ld] a GEMM has just stored (encoder_se.hip): pool over t < pool_lens[b],
  // then y = act(x * s) (acc: y += x * s) over the stored columns, zero from zero_lens[b] on (nullptr: none)
  float* se_sums = reinterpret_cast<float*>(ws + p.se);
  float* se_scale = se_sums + (size_t)batch * h->se_c_max;
  auto run_se = [&](const SeLayer& L, const float* sx, float* sy, int64_t ld, int64_t frames, int store_cols,
                    const int32_t* pool_lens, const int32_t* zero_lens, int relu, int acc, AmaxTab* am,
                    const int32_t* lens_y) -> int {
    SeLaunch a{};
    a.x = sx; a.y = sy; a.ld = ld; a.bs = 0; a.channels = L.c; a.hidden = L.hidden; a.batch = batch;
    a.frames = (int)frames; a.store_cols = store_cols; a.lens = pool_lens; a.w1 = L.d_w1; a.w2 = L.d_w2;
    a.sums = se_sums; a.scale = se_scale; a.zero_lens = zero_lens; a.relu = relu; a.act = h->act; a.accumulate = acc;
    a.amax_y = am; a.lens_y = lens_y;
    if (int rc = note(kPlanSe, sy, sx, nullptr, nullptr)) return rc;
    if (dry) return 0;
    ProfScope ps(h, kProfDepthwise, st, 4.0 * L.c * L.hidden * (double)batch,
                 4.0 * (acc ? 4.0 : 3.0) * L.c * (double)store_cols * batch);
    const int e = launch_se(a, st);
    if (e) return fail(VASR_ERR_HIP, "squeeze-and-excitation: %s", hipGetErrorString((hipError_t)e));
    return 0;
  };
  // GroupNorm of a tensor [B][L.c][ld] a GEMM has just stored raw (encoder_norm.hip): statistics over t < stat_lens[b],
  // then y = act(norm(x) (+ add)) over the stored columns, zero from zero_lens[b] on (nullptr: none); add has pitch add_ld
  float* nrm_ws = reinterpret_cast<float*>(ws + p.norm);
  auto run_norm = [&](const NormLayer& L, const float* nx, float* ny, const float* add, int64_t ld, int64_t add_ld,
                      int64_t frames, int store_cols, const int32_t* stat_lens, const int32_t* zero_lens, int relu, AmaxTab* am,
                      const int32_t* lens_y) -> int {
    NormLaunch a{};
    a.x = nx; a.y = ny; a.add = add; a.ld = ld; a.ld_add = add_ld; a.bs = 0;
    a.channels = L.c; a.groups = L.groups; a.batch = batch; a.frames = (int)frames; a.store_cols = store_cols;
    a.lens = stat_lens; a.group_of = L.d_group_of; a.members = L.d_members; a.gamma = L.d_gamma; a.beta = L.d_beta;
    a.row_mean = nrm_ws; a.row_m2 = nrm_ws + (size_t)batch * h->norm_c_max;
    a.g_mean = nrm_ws + (size_t)2 * batch * h->norm_c_max; a.g_rstd = a.g_mean + (size_t)batch * h->norm_g_max;
    a.zero_lens = zero_lens; a.relu = relu; a.act = h->act; a.amax_y = am; a.lens_y = lens_y;
    if (int rc = note(kPlanNorm, ny, nx, nullptr, add)) return rc;
    if (dry) return 0;
    // (counted with the depthwise class, as the SE passes are: statistics and affine, ~5 flops per element; two reads for
    // the statistics, a read and a write to apply)
    ProfScope ps(h, kProfDepthwise, st, 5.0 * L.c * (double)frames * batch,
                 4.0 * (add ? 5.0 : 4.0) * L.c * (double)store_cols * batch);
    const int e = launch_norm(a, st);
    if (e) return fail(VASR_ERR_HIP, "group norm: %s", hipGetErrorString((hipError_t)e));
    return 0;
  };
  for (size_t i = 0; i < h->blocks.size(); ++i) {
    Block& B = h->blocks[i];
    const bool last_block = i + 1 == h->blocks.size();
    const float* blk_in = cur;
    const int64_t blk_ld = cur_ld;
    blk_amax = cur_amax;
    // the block input stays where it is (the fused residual reads it until the block's last GEMM), an unfused residual result
    // takes the third rotation buffer that is not the block input, the sub-block outputs go where the rotation sends them
    const int blk_buf = buf_of(blk_in);
    rot.begin_block(blk_buf < kBufRot ? blk_buf : kBufNone, B.has_res && !B.fused_res);
    float* R = bufs[rot.pp[2]];
    float* panes = reinterpret_cast<float*>(ws + p.pane);
    const int64_t pane_bs = (int64_t)h->pane_c_max * cur_ld;   // batch stride of the pane buffer, elements
    if (B.keep_input && B.pane == 0) pane_ld = cur_ld;
    // every pane of a run has one pitch (no stride inside a run: vasr_create), which the buffer's layout relies on
    if ((B.keep_input || B.dense_panes >= 2 || B.res_pane0) && cur_ld != pane_ld)
      return fail(VASR_ERR_UNSUPPORTED, "block %zu: dense-residual panes of different pitches (%lld, %lld)", i, (long long)pane_ld,
                  (long long)cur_ld);
    if (B.keep_input) {
      // this block's input is pane B.pane of its dense run (parts/jasper.py:446-447: xs + [out])
      if (int rc = note(kPlanPaneCopy, panes + (int64_t)B.pane_off * cur_ld, cur, nullptr, nullptr)) return rc;
      if (!dry)
        HIP_TRY(hipMemcpy2DAsync(panes + (int64_t)B.pane_off * cur_ld, (size_t)pane_bs * 4, cur, (size_t)B.pane_c * cur_ld * 4,
                                 (size_t)B.pane_c * cur_ld * 4, batch, hipMemcpyDeviceToDevice, st));
    }
    // residual panes' masks: the block input lengths; a last block's residual keeps its padding columns (the encoder output's)
    const int32_t* res_zero = last_block ? nullptr : lens(B.first_step);
    // The residual branch, sum_p (max_p) SE_p(N_p(BN_p(W_p mask(x_p)))) over the block's residual GEMMs (parts/jasper.py:428-441),
    // every source masked with the block-input lengths -- unless it is folded into the last sub-block's GEMM.  Entry 0's GEMM
    // writes R and is normalized / rescaled in place, every later one's goes through D and is combined onto R by its last pass;
    // max without SE: every later GEMM takes max(R, its result) into R itself (each element of R is read and then stored by
    // the one thread that owns it, encoder_pw*.hip)
    for (size_t q = 0; q < B.res.size() && !B.fused_res; ++q) {
      const ResGemm& G = B.res[q];
      const ConvLayer& W = G.w;
      const bool gemm_max = h->res_max && !G.se.d_w1 && q > 0;
      float* Rq = (q == 0 || gemm_max) ? R : D;
      // the block input -- or panes of the dense run: its own panes, or, right after the run, the run's input (pane 0)
      const float* px = G.pane_off >= 0 ? panes + (int64_t)G.pane_off * cur_ld : cur;
      PwArgs a = pw_args(h, W, px, Rq, cur_ld, cur_T, batch);
      a.lens = lens(B.first_step);
      if (gemm_max) { a.res = R; a.ldr = cur_ld; a.res_max = 1; }
      if (G.pane_off < 0) {
        a.amax_x = blk_amax;
      } else {
        a.bsx = pane_bs;
        if (want_amax) {   // fp16 split: one scale from the maxima of all the channels the GEMM reads
          a.amax_x = free_tab(AmaxTab{});
          if (!dry) launch_amax(px, cur_ld, W.cin, (int)cur_T, lens(B.first_step), batch, &a.amax_x, st, pane_bs);
        }
      }
      if (int rc = note(kPlanResGemm, Rq, px, nullptr, a.res)) return rc;
      {
        ProfScope ps(h, kProfPointwise, st, 2.0 * W.cin * W.cout * (double)cur_T * batch,
                     4.0 * W.m_pad * (double)cur_ld * batch);   // bytes of class 2 = what the GEMM STORES (its epilogue's share of the time)
        if (run_pointwise(h, a, W, st, dry) < 0) return VASR_ERR_HIP;
      }
      // GroupNorm, then the residual branch's SqueezeExcite (parts/jasper.py:275-280)
      if (G.norm.d_gamma && run_norm(G.norm, Rq, G.se.d_w1 ? Rq : R, (!G.se.d_w1 && q > 0) ? R : nullptr, cur_ld, cur_ld, cur_T,
                                     (int)cur_ld, lens(B.first_step), res_zero, 0, nullptr, nullptr))
        return VASR_ERR_HIP;
      if (G.se.d_w1 && run_se(G.se, Rq, R, cur_ld, cur_T, (int)cur_ld, lens(B.first_step), res_zero, 0,
                              q > 0 ? (h->res_max ? 2 : 1) : 0, nullptr, nullptr))
        return VASR_ERR_HIP;
    }
    for (size_t r = 0; r < B.subs.size(); ++r) {
      SubBlock& S = B.subs[r];
      const bool last_sub = r + 1 == B.subs.size();
      const bool enc_out = last_block && last_sub;   // this sub-layer writes the encoder output
      const float* gx = cur;
      int64_t gx_ld = cur_ld, g_T = cur_T;
      const int32_t* g_lens = nullptr;
      AmaxTab gx_amax = cur_amax;
      // ---- fused depthwise -> pointwise kernel (encoder_fused.hip): 256-channel sub-blocks in the fp16-split arithmetic ----
      int f_cols = 0;
      const bool fuse_res = last_sub && B.fused_res;
      const ConvLayer& WF = fuse_res ? B.fused : S.pw;
      // (not in row-independent mode: whether a sub-block is fused depends on the batch's tile count, and the two forms
      // round differently -- that mode promises bit-identical rows whatever the batch)
      // (a sub-layer whose output feeds an SE: the fused kernel does not produce its row sums)
      if (!h->row_independent && S.separable && S.dw.d_ftaps && h->gemm_mode == 3 && want_amax && cur_amax.p && WF.d_w16 &&
          !S.se.d_w1 && B.groups == 1 && !S.norm.d_gamma &&   // (no grouped form of the fused kernel, no raw store)
          !(last_sub && B.has_res && !B.fused_res) &&
          // a folded residual must come from a 256-channel block input (K = 256 + 256): the kernel's second K range is 4 chunks
          (fuse_res ? (blk_amax.p && blk_ld == cur_ld && WF.cin == 2 * S.dw.cin && B.fused_k1 == S.dw.cin) : WF.cin == S.dw.cin) &&
          cur_ld % kTimeTile == 0 && !enc_out && (f_cols = fused_tile_cols(h, batch, cur_ld)) != 0) {
        float* dst = next_dst(false);   // (the kernel reads cur)
        if (int rc = check_dst(kPlanFused, dst, cur, fuse_res ? blk_in : nullptr, nullptr)) return rc;
        FusedLaunch f{};
        f.x = cur; f.ldx = cur_ld; f.lens_in = lens(S.dw.step); f.lens_out = lens(S.dw.step + 1);
        f.taps = S.dw.d_ftaps; f.dw_l1 = S.dw.f_l1; f.amax_x = cur_amax;
        f.wt = WF.d_w16; f.w_inv_scale = WF.w16_inv; f.scale = WF.d_scale; f.shift = WF.d_shift;
        f.y = dst; f.ldy = cur_ld; f.frames = (int)cur_T; f.relu = 1; f.act = h->act;
        f.amax_y = free_tab(cur_amax); f.lens_y = lens(S.pw.step + 1);
        if (fuse_res) { f.x2 = blk_in; f.ldx2 = blk_ld; f.lens2 = lens(B.first_step); f.amax_x2 = blk_amax; }
        f.batch = batch; f.kernel = S.dw.kernel;
        f.tile_cols = f_cols;
        f.waves = h->sw.fused_waves;
        int e = 0;   // (a dry pass: every shape that reaches this point has an instantiation)
        if (!dry) {
          ProfScope ps(h, kProfFused, st, 2.0 * WF.cin * WF.cout * (double)cur_T * batch,
                       4.0 * (2.0 + (fuse_res ? 1.0 : 0.0)) * S.dw.cin * (double)cur_T * batch);
          e = launch_fused_dwpw(f, st, &f.amax_y.n);
        }
        if (e > 0) return fail(VASR_ERR_HIP, "fused dw -> pw: %s", hipGetErrorString((hipError_t)e));
        if (e == 0) {
          commit(kPlanFused, dst, cur, f.x2, nullptr);
          rot.wrote(buf_of(dst));
          cur = dst;
          cur_amax = f.amax_y;
          continue;
        }
        // shape not covered after all: the two-kernel path below (nothing was committed)
      }
      if (S.separable) {
        const int64_t t_out = conv_out_frames(cur_T, S.dw);
        const int64_t ld_out = pad_frames(t_out);
        ProfScope ps(h, kProfDepthwise, st, 2.0 * S.dw.kernel * S.dw.cin * (double)t_out * batch,
                     4.0 * ((double)S.dw.cin * cur_T + (double)S.dw.cin * t_out) * batch + 4.0 * S.dw.cin * S.dw.kernel);
        AmaxTab am = want_amax ? free_tab(AmaxTab{}) : AmaxTab{};
        // fp16-split mode with the input's maxima at hand: the Toeplitz form on the matrix pipe (in the pipeline, per
        // 512-channel layer: 22.8 / 23.7 / 23.8 / 28.1 us at K = 51 / 63 / 75 / 87 x 2 against 25.6 / 28.4 / 31.0 / 35.5 us
        // of packed FMAs; 256 channels, K = 33 / 39: 12.8 / 12.6 against 13.3 / 13.4), else packed FMAs.
        // VASR_DW_MFMA=0 keeps the packed-FMA kernels.
        const bool dw_mfma = h->sw.dw_mfma;
        if (int rc = note(kPlanDepthwise, D, cur, nullptr, nullptr)) return rc;
        int e = dry ? 0 : -1;
        if (!dry && want_amax && dw_mfma && cur_amax.p && S.dw.d_taps)
          e = launch_depthwise_mfma(cur, cur_ld, S.dw.d_taps, S.dw.d_tap_inv, lens(S.dw.step), lens(S.dw.step + 1), cur_amax,
                                    batch, S.dw.cin, S.dw.kernel, S.dw.dilation, D, ld_out, am.p ? &am : nullptr, st);
        if (e > 0) return fail(VASR_ERR_HIP, "depthwise (MFMA): %s", hipGetErrorString((hipError_t)e));
        if (e < 0 && launch_depthwise(cur, cur_ld, (int)cur_T, S.dw.d_w, lens(S.dw.step), lens(S.dw.step + 1), batch, S.dw.cin,
                                      S.dw.kernel, S.dw.stride, S.dw.dilation, S.dw.pad, D, ld_out, st, am.p ? &am : nullptr))
          return fail(VASR_ERR_WORKSPACE, "maxima table too small for depthwise layer of block %zu", i);
        gx = D; gx_ld = ld_out; g_T = t_out; gx_amax = am;
      } else {
        g_lens = lens(S.pw.step);  // block input is unmasked: predicate inside the GEMM
        if (S.pw.conv_cin) {
          g_T = conv_out_frames(cur_T, S.pw);
          // fp16 split: an encoder input no kernel published maxima of (the mel features) gets them here -- over all of its
          // channels (a grouped conv's conv_cin is one group's)
          if (want_amax && !gx_amax.p) {
            gx_amax = free_tab(AmaxTab{});
            if (!dry) launch_amax(cur, cur_ld, S.pw.conv_cin * S.pw.groups, (int)cur_T, g_lens, batch, &gx_amax, st);
          }
        }
      }
      // (the GEMM of the two-kernel separable path reads D: it may store over the current tensor)
      float* dst = next_dst(S.separable);
      // (a K-tap conv's output has its own pitch: stride 2 halves the frames)
      int64_t dst_ld = S.pw.conv_cin ? pad_frames(g_T) : gx_ld;
      if (enc_out) { dst = out; dst_ld = out_ld; }
      // a grouped layer in the fp32 mode: its block-diagonal form (encoder_pw.hip has no grouped kernel)
      const ConvLayer& W = fuse_res ? B.fused : (S.pw.groups > 1 && h->gemm_mode == 0 ? S.pw_bd : S.pw);
      PwArgs a = pw_args(h, W, gx, dst, gx_ld, g_T, batch);
      a.groups = W.groups;
      a.lens = g_lens;
      // (a normalized block: the GEMM stores its raw output, the GroupNorm pass adds the residual)
      const bool nrm = S.norm.d_gamma != nullptr;
      a.res = (last_sub && B.has_res && !B.fused_res && !nrm) ? R : nullptr;
      a.ldy = dst_ld; a.ldr = blk_ld;
      // se and not residual: the last sub-layer's SE comes before the block's output activation (parts/jasper.py:250-251, mout)
      const int act = (last_sub && S.se.d_w1) ? 0 : 1;
      a.relu = nrm ? 0 : act;
      a.act = h->act;
      a.res_max = h->res_max;   // (max with GroupNorm is refused: vasr_finalize)
      a.store_cols = (dst_ld % kTimeTile == 0) ? (int)dst_ld : (int)g_T;  // port tensors are not padded
      if (W.conv_cin) {
        a.conv_cin = W.conv_cin; a.conv_stride = W.stride; a.conv_dil = W.dilation; a.conv_pad = W.pad;
        a.conv_cols = pad_frames(g_T);
      }
      // the depthwise output is zero past its lens_out, a masked input past its mask: tiles out there skip their K loop
      a.zero_from = S.separable ? lens(S.dw.step + 1) : g_lens;
      if (fuse_res) { a.x2 = blk_in; a.lens2 = lens(B.first_step); a.K1 = B.fused_k1; a.ldx2 = blk_ld; }
      if ((a.res || fuse_res || (nrm && last_sub && B.has_res)) && (blk_ld != gx_ld || (W.conv_cin && g_T != cur_T)))
        return fail(VASR_ERR_UNSUPPORTED, "block %zu: residual across a strided block", i);
      a.amax_x = gx_amax;
      a.amax_x2 = fuse_res ? blk_amax : AmaxTab{};
      // this GEMM's output is masked at lens(S.pw.step + 1) by whatever reads it next
      // (the encoder output's maxima are only wanted by the fused path's CTC head, which reads every column < T')
      if (want_amax && (!enc_out || enc_amax)) {
        a.amax_y = free_tab(gx_amax);
        a.lens_y = enc_out ? own_tab : lens(S.pw.step + 1);
      }
      if (int rc = note(kPlanGemm, dst, gx, a.x2, a.res)) return rc;
      int published;
      {
        ProfScope ps(h, kProfPointwise, st, 2.0 * W.cin * W.cout * (double)g_T * batch, 4.0 * W.m_pad * (double)dst_ld * batch);
        published = run_pointwise(h, a, W, st, dry);
      }
      if (published < 0) return VASR_ERR_HIP;
      rot.wrote(buf_of(dst));
      // GroupNorm of the conv's output over its own lengths, then the activation (the last sub-layer's: after the residual
      // sum, or after its SE); the normalized tensor's maxima replace the ones the GEMM published
      if (nrm) {
        if (run_norm(S.norm, dst, dst, (last_sub && B.has_res) ? R : nullptr, dst_ld, blk_ld, g_T, a.store_cols,
                     lens(S.pw.step + 1), enc_out ? nullptr : lens(S.pw.step + 1), act, published ? &a.amax_y : nullptr,
                     a.lens_y))
          return VASR_ERR_HIP;
      }
      // se and not residual: SE after the sub-layer, pooled over the conv's output lengths; the rescaled tensor's maxima
      // replace the ones the GEMM published
      if (S.se.d_w1) {
        if (run_se(S.se, dst, dst, dst_ld, g_T, a.store_cols, lens(S.pw.step + 1), enc_out ? nullptr : lens(S.pw.step + 1),
                   last_sub ? 1 : 0, 0, published ? &a.amax_y : nullptr, a.lens_y))
          return VASR_ERR_HIP;
      }
      cur = dst; cur_ld = dst_ld; cur_T = g_T;
      cur_amax = published ? a.amax_y : AmaxTab{};
    }
  }
  if (enc_amax) *enc_amax = cur_amax;
  return dry ? 0 : check_launch("encoder");
}

int run_decoder(vasr_handle* h, const float* encp, int64_t ld, int64_t T1, int batch, float* logits, float* logp,
                int64_t* pred, hipStream_t st, AmaxTab enc_amax = AmaxTab{}, const int32_t* own_frames = nullptr) {
  PwArgs a = pw_args(h, h->dec, encp, logits, ld, T1, batch);
  a.lens = own_frames;   // (row-independent mode): columns past the row's own frame count are read as zero
  a.m_store = h->num_classes;
  ProfScope ps(h, kProfHead, st);
  // split GEMM unless fp32 mode is selected: the fp16 form when the encoder published its output's maxima (fused path),
  // else 3 x bf16 (port tensors of the per-module entry point carry none)
  a.amax_x = enc_amax;
  if (run_pointwise(h, a, h->dec, st) < 0) return VASR_ERR_HIP;
  launch_logsoftmax_argmax(logits, ld, (int64_t)h->num_classes * ld, batch, (int)T1, h->num_classes, logp, pred, st);
  return check_launch("decoder");
}

}  // namespace

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
    // Dense residual panes, as the reference builds and runs them: every residual_dense block appends its input width to ONE
    // list shared by all blocks (jasper.py:152-161) and keeps a copy (parts/jasper.py:264); a dense block with residual sums a
    // 1x1 conv of each entry's pane, xs[p], and hands xs + [out] on, any other block [out] alone (:428-448).  A layout in
    // which a block's copy is longer than the pane list reaching it raises IndexError in the reference: refused here.
    std::vector<int> xs_c{d->feat_in};   // channels of the panes reaching the next block
    int dense_seen = 0, cin = d->feat_in, origin = 0;   // origin: the block whose input is pane 0 of that list
    for (int i = 0; i < d->n_blocks; ++i) {
      Block& B = h->blocks[i];
      const vasr_block_desc& b = B.d;
      if (!b.residual_dense && b.residual && xs_c.size() > 1) {
        if (xs_c[0] != cin || b.stride > 1) {
          return fail(VASR_ERR_INVALID, "block %d: a residual block after a dense run takes its residual from the run's input "
                      "(%d channels, block input %d%s) -- the reference fails here", i, xs_c[0], cin, b.stride > 1 ? ", strided" : "");
        }
        B.res_pane0 = true;
        h->blocks[origin].keep_input = true;
        h->pane_c_max = std::max(h->pane_c_max, xs_c[0]);
      }
      if (b.residual_dense) {
        ++dense_seen;
        if (b.residual && dense_seen > (int)xs_c.size()) {
          return fail(VASR_ERR_INVALID, "block %d: residual_dense block number %d sees %zu residual pane(s): dense blocks must form one "
                      "contiguous run of residual blocks (the reference fails in JasperBlock.forward)", i, dense_seen, xs_c.size());
        }
        if (b.residual && b.stride > 1) {
          return fail(VASR_ERR_INVALID, "block %d: a strided block cannot take a dense residual (its panes have other lengths)", i);
        }
        B.pane = (int)xs_c.size() - 1;
        B.pane_c = cin;
        for (int q = 0; q < B.pane; ++q) B.pane_off += xs_c[q];
        if (b.residual) B.dense_panes = dense_seen;
      }
      if (b.residual_dense && b.residual) {
        xs_c.push_back(b.filters);
      } else {
        xs_c.assign(1, b.filters);
        origin = i + 1;
      }
      cin = b.filters;
    }
    // a pane buffer only where some block sums two or more panes; that block's panes are the inputs of the blocks before it
    for (int i = 0; i < d->n_blocks; ++i) {
      Block& B = h->blocks[i];
      if (B.dense_panes < 2) continue;
      h->pane_c_max = std::max(h->pane_c_max, B.pane_off + B.pane_c);
      for (int q = 0; q < B.dense_panes; ++q) h->blocks[i - B.dense_panes + 1 + q].keep_input = true;
    }
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

// vasr_finalize's checks of the encoder, before anything touches the device
static int check_encoder(vasr_handle* h) {
  int rc;
  if (h->res_max)
    for (size_t i = 0; i < h->blocks.size(); ++i)
      if (h->blocks[i].norm_g)
        return fail(VASR_ERR_UNSUPPORTED, "block %zu: residual_mode max with group, instance or layer normalization", i);
  if ((rc = check_groups(h)) || (rc = check_se(h))) return rc;
  return check_norm(h);
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
  if (samples <= h->fe.n_fft / 2)
    return fail(VASR_ERR_INVALID, "reflect padding needs more than n_fft/2 = %d samples (got %lld)",
                h->fe.n_fft / 2, (long long)samples);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int T = (int)vasr_mel_frames(h, samples);
  launch_seq_len(d_len, batch, h->fe.hop_length, d_seq, st);
  launch_stft_logmel(h->ft, d_wav, false, batch, samples, h->row_independent ? d_len : nullptr, h->fe.hop_length,
                     h->fe.preemph, h->fe.log_guard, d_mel, T, T, st);
  launch_normalize(d_mel, T, d_seq, batch, h->fe.n_mels, T, h->fe.normalize == 1, st);
  if (h->fe.normalize == 2) launch_normalize_all(d_mel, T, d_seq, batch, h->fe.n_mels, T, st);
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
  const Block& b0 = h->blocks[0];
  if (b0.subs[0].separable && !b0.has_res)
    // block 0 reads the port tensor in place (the generic depthwise kernel copes with the unpadded pitch)
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

int vasr_error_counts_i32(const int32_t* d_hyp, int64_t hyp_width, const int32_t* d_hyp_len, const int32_t* d_ref,
                          int64_t ref_width, const int32_t* d_ref_len, int batch, const int32_t* h_space_ids, int n_space,
                          int32_t* d_counts, vasr_stream stream) {
  // every refusal comes before a device is touched
  if (!d_hyp || !d_hyp_len || !d_ref || !d_ref_len || !d_counts) return fail(VASR_ERR_INVALID, "error_counts: NULL pointer");
  if (batch <= 0 || hyp_width < 0 || ref_width < 0)
    return fail(VASR_ERR_INVALID, "error_counts: batch %d, widths %lld / %lld", batch, (long long)hyp_width, (long long)ref_width);
  if (n_space < 0 || n_space > kMetricsMaxSpace || (n_space > 0 && !h_space_ids))
    return fail(VASR_ERR_INVALID, "error_counts: n_space %d outside 0..%d (or no ids given)", n_space, kMetricsMaxSpace);
  if (reinterpret_cast<uintptr_t>(d_counts) & 15) return fail(VASR_ERR_INVALID, "error_counts: d_counts is not 16-byte aligned");
  if (hyp_width > kMetricsMaxWidth || ref_width > kMetricsMaxWidth)
    return fail(VASR_ERR_UNSUPPORTED, "error_counts: rows of %lld / %lld ids, at most %d per side", (long long)hyp_width,
                (long long)ref_width, kMetricsMaxWidth);
  SpaceIds sp{};
  sp.n = n_space;
  for (int k = 0; k < n_space; ++k) sp.id[k] = h_space_ids[k];
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
  if (n_space < 0 || n_space > kMetricsMaxSpace || (n_space > 0 && !h_space_ids))
    return fail(VASR_ERR_INVALID, "error_ops: n_space %d outside 0..%d (or no ids given)", n_space, kMetricsMaxSpace);
  if (reinterpret_cast<uintptr_t>(d_ops_counts) & 15) return fail(VASR_ERR_INVALID, "error_ops: d_ops_counts is not 16-byte aligned");
  if (hyp_width > kMetricsMaxWidth || ref_width > kMetricsMaxWidth)
    return fail(VASR_ERR_UNSUPPORTED, "error_ops: rows of %lld / %lld ids, at most %d per side", (long long)hyp_width,
                (long long)ref_width, kMetricsMaxWidth);
  if (d_script && (hyp_width > kMetricsMaxScriptWidth || ref_width > kMetricsMaxScriptWidth))
    return fail(VASR_ERR_UNSUPPORTED, "error_ops: rows of %lld / %lld ids with a script, at most %d per side (counts alone: %d)",
                (long long)hyp_width, (long long)ref_width, kMetricsMaxScriptWidth, kMetricsMaxWidth);
  SpaceIds sp{};
  sp.n = n_space;
  for (int k = 0; k < n_space; ++k) sp.id[k] = h_space_ids[k];
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
  if (n_space < 0 || n_space > kMetricsMaxSpace || (n_space > 0 && !h_space_ids))
    return fail(VASR_ERR_INVALID, "nbest_error_counts: n_space %d outside 0..%d (or no ids given)", n_space, kMetricsMaxSpace);
  if ((reinterpret_cast<uintptr_t>(d_slot_counts) | reinterpret_cast<uintptr_t>(d_counts)) & 15)
    return fail(VASR_ERR_INVALID, "nbest_error_counts: d_slot_counts / d_counts is not 16-byte aligned");
  if (nbest > kMetricsMaxNbest)
    return fail(VASR_ERR_UNSUPPORTED, "nbest_error_counts: nbest %d, at most %d", nbest, kMetricsMaxNbest);
  if (width > kMetricsMaxWidth || ref_width > kMetricsMaxWidth)
    return fail(VASR_ERR_UNSUPPORTED, "nbest_error_counts: rows of %lld / %lld ids, at most %d per side", (long long)width,
                (long long)ref_width, kMetricsMaxWidth);
  SpaceIds sp{};
  sp.n = n_space;
  for (int k = 0; k < n_space; ++k) sp.id[k] = h_space_ids[k];
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

int vasr_ctc_loss_f32(const float* d_logp, const int32_t* d_frames, int batch, int64_t frames, int num_classes, int blank,
                      const int32_t* d_tgt, int64_t tgt_width, const int32_t* d_tgt_len, float* d_loss, vasr_stream stream) {
  // every refusal comes before a device is touched
  if (!d_logp || !d_frames || !d_tgt || !d_tgt_len || !d_loss) return fail(VASR_ERR_INVALID, "ctc_loss: NULL pointer");
  if (batch <= 0 || frames < 0 || tgt_width < 0)
    return fail(VASR_ERR_INVALID, "ctc_loss: batch %d, frames %lld, tgt_width %lld", batch, (long long)frames, (long long)tgt_width);
  if (num_classes < 2 || blank < 0 || blank >= num_classes)
    return fail(VASR_ERR_INVALID, "ctc_loss: num_classes %d (at least 2), blank %d outside [0, num_classes)", num_classes, blank);
  if (tgt_width > kCtcLossMaxWidth)
    return fail(VASR_ERR_UNSUPPORTED, "ctc_loss: targets of %lld ids, at most %d", (long long)tgt_width, kCtcLossMaxWidth);
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
  if (batch <= 0 || frames < 0 || tgt_width < 0)
    return fail(VASR_ERR_INVALID, "ctc_align: batch %d, frames %lld, tgt_width %lld", batch, (long long)frames, (long long)tgt_width);
  if (num_classes < 2 || blank < 0 || blank >= num_classes)
    return fail(VASR_ERR_INVALID, "ctc_align: num_classes %d (at least 2), blank %d outside [0, num_classes)", num_classes, blank);
  if (!d_workspace) return fail(VASR_ERR_INVALID, "ctc_align: NULL workspace");
  if (tgt_width > kCtcLossMaxWidth)
    return fail(VASR_ERR_UNSUPPORTED, "ctc_align: targets of %lld ids, at most %d", (long long)tgt_width, kCtcLossMaxWidth);
  const size_t need = ctc_align_workspace_bytes(batch, frames, (int)tgt_width);
  if (workspace_bytes < need)
    return fail(VASR_ERR_INVALID, "ctc_align: workspace of %zu bytes, %zu needed (vasr_ctc_align_workspace_bytes)", workspace_bytes, need);
  const int rc = launch_ctc_align(d_logp, d_frames, batch, frames, num_classes, blank, d_tgt, (int)tgt_width, d_tgt_len, d_score,
                                  d_start, d_end, d_tok_logp, d_path, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  if (rc) return fail(VASR_ERR_HIP, "ctc_align: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
  return check_launch("ctc_align");
}

// One contiguous slice of the batch through the whole path on one stream.
static int transcribe_part(vasr_handle* h, const void* d_wav, bool pcm16, const int64_t* d_len, int batch, int64_t samples,
                           int64_t* d_pred, int32_t* d_ids, int32_t* d_id_len, float* d_logp, float* d_enc_len,
                           char* ws, hipStream_t st) {
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

// How many slices the batch is cut into; slice i runs on its own internal stream so that one slice's
// HBM-bound kernels (depthwise, epilogue stores) overlap another slice's MFMA-bound GEMM main loops.
static int n_slices(const vasr_handle* h, int batch) {
  int n = h->slices;
  if (n < 1) n = 1;
  if (n > kMaxSlices) n = kMaxSlices;
  while (n > 1 && batch / n < 8) --n;   // tiny batches: one slice (the kernels would not fill the chip anyway)
  return n;
}

static size_t sliced_workspace_bytes(const vasr_handle* h, int batch, int64_t T) {
  const int n = n_slices(h, batch);
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    const int lo = (int)((int64_t)batch * i / n), hi = (int)((int64_t)batch * (i + 1) / n);
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
  if (samples <= h->fe.n_fft / 2)
    return fail(VASR_ERR_INVALID, "reflect padding needs more than n_fft/2 = %d samples (got %lld)",
                h->fe.n_fft / 2, (long long)samples);
  const int64_t T = vasr_mel_frames(h, samples);
  const size_t need_bytes = sliced_workspace_bytes(h, batch, T);
  if (ws_bytes < need_bytes) return fail(VASR_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, need_bytes);
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
    const int lo = (int)((int64_t)batch * i / n), hi = (int)((int64_t)batch * (i + 1) / n);
    hipStream_t st = h->slice_stream[i];
    HIP_TRY(hipStreamWaitEvent(st, h->slice_fork, 0));
    int rc = transcribe_part(h, static_cast<const char*>(d_wav) + (int64_t)lo * samples * (pcm16 ? 2 : 4), pcm16, d_len + lo, hi - lo, samples,
                             d_pred ? d_pred + (int64_t)lo * T1 : nullptr, d_ids ? d_ids + (int64_t)lo * T1 : nullptr,
                             d_id_len ? d_id_len + lo : nullptr,
                             d_logp ? d_logp + (int64_t)lo * T1 * h->num_classes : nullptr,
                             d_enc_len ? d_enc_len + lo : nullptr, ws + off, st);
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
  if (samples <= h->fe.n_fft / 2)
    return fail(VASR_ERR_INVALID, "reflect padding needs more than n_fft/2 = %d samples (got %lld)",
                h->fe.n_fft / 2, (long long)samples);
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
    launch_seq_len(d_len, batch, h->fe.hop_length, seq_raw, st);
    launch_stft_logmel(h->ft, d_wav, false, batch, samples, h->row_independent ? d_len : nullptr, h->fe.hop_length,
                       h->fe.preemph, h->fe.log_guard, mel_raw, c.Tp, (int)c.T, st);
    launch_normalize(mel_raw, c.Tp, seq_raw, batch, h->fe.n_mels, (int)c.T, h->fe.normalize == 1, st);
    if (h->fe.normalize == 2) launch_normalize_all(mel_raw, c.Tp, seq_raw, batch, h->fe.n_mels, (int)c.T, st);
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

int vasr_set_slices(vasr_handle* h, int slices) {
  if (!h || slices < 1 || slices > kMaxSlices) return fail(VASR_ERR_INVALID, "slices must be 1..%d", kMaxSlices);
  h->slices = slices;
  return 0;
}

#ifdef VASR_DEVTOOLS
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
      const int nb = (int)((int64_t)batch * (i + 1) / n) - (int)((int64_t)batch * i / n);
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
    const Block& b0 = e->blocks[0];
    const bool in_place = b0.subs[0].separable && !b0.has_res;
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
#endif

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
