// What vasr_create and vasr_finalize make of a model description and its state dict: weight lookup, BatchNorm folding, the
// weight packs, the state-dict key layout, the checks that come before anything touches the device, and the device tables.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "vasr_model.h"

namespace vasr {

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

}  // namespace

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

// vasr_create: which block inputs are kept as panes of a dense residual, and where in the pane buffer
int layout_dense_panes(vasr_handle* h) {
  const int n_blocks = (int)h->blocks.size();
  // Dense residual panes, as the reference builds and runs them: every residual_dense block appends its input width to ONE
  // list shared by all blocks (jasper.py:152-161) and keeps a copy (parts/jasper.py:264); a dense block with residual sums a
  // 1x1 conv of each entry's pane, xs[p], and hands xs + [out] on, any other block [out] alone (:428-448).  A layout in
  // which a block's copy is longer than the pane list reaching it raises IndexError in the reference: refused here.
  std::vector<int> xs_c{h->feat_in};   // channels of the panes reaching the next block
  int dense_seen = 0, cin = h->feat_in, origin = 0;   // origin: the block whose input is pane 0 of that list
  for (int i = 0; i < n_blocks; ++i) {
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
  for (int i = 0; i < n_blocks; ++i) {
    Block& B = h->blocks[i];
    if (B.dense_panes < 2) continue;
    h->pane_c_max = std::max(h->pane_c_max, B.pane_off + B.pane_c);
    for (int q = 0; q < B.dense_panes; ++q) h->blocks[i - B.dense_panes + 1 + q].keep_input = true;
  }
  return 0;
}

// vasr_finalize's checks of the encoder, before anything touches the device
int check_encoder(vasr_handle* h) {
  int rc;
  if (h->res_max)
    for (size_t i = 0; i < h->blocks.size(); ++i)
      if (h->blocks[i].norm_g)
        return fail(VASR_ERR_UNSUPPORTED, "block %zu: residual_mode max with group, instance or layer normalization", i);
  if ((rc = check_groups(h)) || (rc = check_se(h))) return rc;
  return check_norm(h);
}

}  // namespace vasr
