// The encoder pass: its workspace plan, the profiling bracket around each launch, the GEMM dispatch, and run_encoder itself --
// one pass over the blocks that launches (or, dry, records) every kernel -- with the CTC head's pass behind it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vasr_model.h"

namespace vasr {

// the first conv of a sub-block (a separable one's depthwise conv): the one that sets its output's frames -- and the first
// conv of the first block, which the encoder's input runs through
static const ConvLayer& first_conv(const SubBlock& S) { return S.separable ? S.dw : S.pw; }
static const ConvLayer& first_conv(const vasr_handle* h) { return first_conv(h->blocks[0].subs[0]); }

int64_t enc_frames(const vasr_handle* h, int64_t t) {
  for (const Block& B : h->blocks)
    for (const SubBlock& S : B.subs) t = conv_out_frames(t, first_conv(S));
  return t;
}

WsPlan plan_ws(const vasr_handle* h, int batch, int64_t T) {
  WsPlan p{};
  p.T = T;
  p.Tp0 = pad_frames(T);
  p.T1 = h->has_encoder ? enc_frames(h, T) : T;
  // the first (strided) block may still run at T frames inside: size by the larger pitch
  p.Tp1 = pad_frames(p.T1);
  const int64_t tp_mid = h->has_encoder ? pad_frames(conv_out_frames(T, first_conv(h))) : p.Tp1;
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

// ProfScope (vasr_model.h)
hipEvent_t ProfScope::get(vasr_handle* h) {
  hipEvent_t e;
  if (!h->ev_pool.empty()) { e = h->ev_pool.back(); h->ev_pool.pop_back(); return e; }
  if (hipEventCreate(&e) != hipSuccess) e = nullptr;   // a null event makes the record / elapsed calls fail loudly
  return e;
}
// Single-launch classes (depthwise, pointwise) hand the event pair to the launch itself (g_probe: the dispatch
// packet's begin / end timestamps); multi-launch groups (front end, head) are bracketed on the stream.
// flops / bytes: the ALGORITHMIC work of the bracketed launch (2 M N K of a GEMM; read x + write y of a depthwise or
// fused layer), summed per class by vasr_profile_end so that a rate is always work-that-ran over time-it-took
ProfScope::ProfScope(vasr_handle* h_, int cls_, hipStream_t st_, double flops_, double bytes_)
    : h(h_), st(st_), cls(cls_), flops(flops_), bytes(bytes_) {
  if (!h->profiling) return;
  a = get(h); b = get(h);
  if (cls == 1 || cls == 2 || cls == 4) g_probe = LaunchProbe{a, b};
  else (void)hipEventRecord(a, st);
}
ProfScope::~ProfScope() {
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

namespace {

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

// One encoder pass (run_encoder): where the current tensor, the block input and their maxima live, and the steps of a block.
// Every step launches as it goes -- or, dry, only records what it would launch.
struct EncoderPass {
  vasr_handle* h;
  char* ws;
  const WsPlan& p;
  hipStream_t st;
  int batch;
  PlanRec* rec;
  const bool dry;
  const float* x;      // the encoder input
  float* out;          // the encoder output, pitch out_ld
  int64_t out_ld;
  AmaxTab* enc_amax;
  int32_t* lens_tab;
  const int32_t* own_tab = nullptr;   // row-independent mode: the frames an unbatched call on each row would produce
  float* bufs[4];
  float* D;
  // Where the sub-block outputs go (vasr_host.h BufRotation), and the check every launch passes before it is made: its
  // destination is none of its own sources, not the live block input, not the live R, not the pane buffer
  BufRotation rot;
  const float *pane_lo, *pane_hi;
  const float* cur;
  int64_t cur_ld, cur_T;
  // fp16-split GEMMs: maxima rows, indexed by the length-chain step of the conv that produced the tensor
  const bool want_amax;
  unsigned int* amax_base;
  AmaxTab cur_amax{}, blk_amax{};   // maxima of `cur` / of the block input over each utterance's valid frames (p == nullptr: not known)
  int64_t pane_ld = 0;   // pitch of the current dense run's panes: its first block's input pitch
  float *se_sums, *se_scale;   // SE row sums and scales
  float* nrm_ws;               // GroupNorm statistics
  // the block being run (run() sets them)
  size_t blk_i = 0;
  bool last_block = false;
  const float* blk_in = nullptr;
  int64_t blk_ld = 0;
  float* R = nullptr;        // the residual branch's result
  float* panes = nullptr;
  int64_t pane_bs = 0;       // batch stride of the pane buffer, elements
  const int32_t* res_zero = nullptr;

  EncoderPass(vasr_handle* h_, const float* x_, int64_t x_ld, int64_t T, int batch_, float* out_, int64_t out_ld_, char* ws_,
              const WsPlan& p_, hipStream_t st_, AmaxTab* enc_amax_, PlanRec* rec_)
      : h(h_), ws(ws_), p(p_), st(st_), batch(batch_), rec(rec_), dry(rec_ != nullptr), x(x_), out(out_), out_ld(out_ld_),
        enc_amax(enc_amax_), lens_tab(reinterpret_cast<int32_t*>(ws_ + p_.lens_tab)),
        bufs{reinterpret_cast<float*>(ws_ + p_.bufP), reinterpret_cast<float*>(ws_ + p_.bufQ),
             reinterpret_cast<float*>(ws_ + p_.bufR), reinterpret_cast<float*>(ws_ + p_.bufS)},
        D(reinterpret_cast<float*>(ws_ + p_.bufD)), pane_lo(reinterpret_cast<const float*>(ws_ + p_.pane)),
        pane_hi(reinterpret_cast<const float*>(ws_ + p_.encp)), cur(x_), cur_ld(x_ld), cur_T(T), want_amax(h_->gemm_mode == 3),
        amax_base(reinterpret_cast<unsigned int*>(ws_ + p_.amax)), se_sums(reinterpret_cast<float*>(ws_ + p_.se)),
        se_scale(se_sums + (size_t)batch_ * h_->se_c_max), nrm_ws(reinterpret_cast<float*>(ws_ + p_.norm)) {
    rot.inplace = h->sw.buf_inplace;
  }

  int32_t* lens(int step) const { return lens_tab + (size_t)step * batch; }
  int buf_of(const float* q) const {
    if (!q) return kBufNone;
    for (int i = 0; i < kBufRot; ++i) if (q == bufs[i]) return i;
    if (q == D) return kBufD;
    if (q == out) return kBufOut;
    if (q == x) return kBufIn;
    return h->pane_c_max && q >= pane_lo && q < pane_hi ? kBufPane : kBufNone;
  }
  int check_dst(int kind, const float* dst, const float* sx, const float* sx2, const float* sr) const {
    const int d = buf_of(dst), a = buf_of(sx), b = buf_of(sx2), r = buf_of(sr);
    if (const char* why = rot.refuse(kind, d, a, b, r))
      return fail(VASR_ERR_STATE, "encoder buffers: %s (launch kind %d: dst %d, src %d, src2 %d, res %d)", why, kind, d, a, b, r);
    return 0;
  }
  void commit(int kind, const float* dst, const float* sx, const float* sx2, const float* sr) {
    const int d = buf_of(dst), a = buf_of(sx), b = buf_of(sx2), r = buf_of(sr);
    rot.launched(d, a, b, r);
    if (rec) rec->v.insert(rec->v.end(), {kind, d, a, b, r});
  }
  int note(int kind, const float* dst, const float* sx, const float* sx2, const float* sr) {
    if (int rc = check_dst(kind, dst, sx, sx2, sr)) return rc;
    commit(kind, dst, sx, sx2, sr);
    return 0;
  }
  // the rotation buffer the next sub-block output goes to (over_cur: the launch does not read the current tensor)
  float* next_dst(bool over_cur) const {
    const int d = rot.pick(over_cur);
    return d >= 0 ? bufs[d] : nullptr;   // (nullptr: no dead buffer -- check_dst refuses it)
  }
  // a table that neither the block input's nor the current tensor's maxima live in (the third candidate is always free)
  AmaxTab free_tab(const AmaxTab& also_busy) const {
    for (int i = 0; i < kAmaxTabs; ++i) {
      unsigned int* q = amax_base + (size_t)i * batch * p.amax_stride;
      if (q != cur_amax.p && q != blk_amax.p && q != also_busy.p) return AmaxTab{q, p.amax_stride, 0};
    }
    return AmaxTab{};
  }

  // squeeze-and-excitation of a tensor [B][L.c][ld] a GEMM has just stored (encoder_se.hip): pool over t < pool_lens[b],
  // then y = act(x * s) (acc: y += x * s) over the stored columns, zero from zero_lens[b] on (nullptr: none)
  int run_se(const SeLayer& L, const float* sx, float* sy, int64_t ld, int64_t frames, int store_cols, const int32_t* pool_lens,
             const int32_t* zero_lens, int relu, int acc, AmaxTab* am, const int32_t* lens_y) {
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
  }
  // GroupNorm of a tensor [B][L.c][ld] a GEMM has just stored raw (encoder_norm.hip): statistics over t < stat_lens[b],
  // then y = act(norm(x) (+ add)) over the stored columns, zero from zero_lens[b] on (nullptr: none); add has pitch add_ld
  int run_norm(const NormLayer& L, const float* nx, float* ny, const float* add, int64_t ld, int64_t add_ld, int64_t frames,
               int store_cols, const int32_t* stat_lens, const int32_t* zero_lens, int relu, AmaxTab* am, const int32_t* lens_y) {
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
  }

  // a block whose input is a pane of a dense run: the run's one pitch, and the copy into the pane buffer
  int keep_pane(const Block& B) {
    if (B.keep_input && B.pane == 0) pane_ld = cur_ld;
    // every pane of a run has one pitch (no stride inside a run: vasr_create), which the buffer's layout relies on
    if ((B.keep_input || B.dense_panes >= 2 || B.res_pane0) && cur_ld != pane_ld)
      return fail(VASR_ERR_UNSUPPORTED, "block %zu: dense-residual panes of different pitches (%lld, %lld)", blk_i,
                  (long long)pane_ld, (long long)cur_ld);
    if (B.keep_input) {
      // this block's input is pane B.pane of its dense run (parts/jasper.py:446-447: xs + [out])
      if (int rc = note(kPlanPaneCopy, panes + (int64_t)B.pane_off * cur_ld, cur, nullptr, nullptr)) return rc;
      if (!dry)
        HIP_TRY(hipMemcpy2DAsync(panes + (int64_t)B.pane_off * cur_ld, (size_t)pane_bs * 4, cur, (size_t)B.pane_c * cur_ld * 4,
                                 (size_t)B.pane_c * cur_ld * 4, batch, hipMemcpyDeviceToDevice, st));
    }
    return 0;
  }

  // The residual branch, sum_p (max_p) SE_p(N_p(BN_p(W_p mask(x_p)))) over the block's residual GEMMs (parts/jasper.py:428-441),
  // every source masked with the block-input lengths -- unless it is folded into the last sub-block's GEMM.  Entry 0's GEMM
  // writes R and is normalized / rescaled in place, every later one's goes through D and is combined onto R by its last pass;
  // max without SE: every later GEMM takes max(R, its result) into R itself (each element of R is read and then stored by
  // the one thread that owns it, encoder_pw*.hip)
  int residual_branch(const Block& B) {
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
    return 0;
  }

  // Whether sub-block S of block B takes the fused depthwise -> pointwise kernel (encoder_fused.hip): 256-channel sub-blocks in
  // the fp16-split arithmetic.  Returns the kernel's tile width (fused_tile_cols), 0: depthwise and GEMM as two kernels.
  // WF: the GEMM's weights (fuse_res: with the block's residual folded in as a second K range).
  int fused_cols(const Block& B, const SubBlock& S, bool last_sub, bool enc_out, bool fuse_res, const ConvLayer& WF) const {
    int f_cols = 0;
    // (not in row-independent mode: whether a sub-block is fused depends on the batch's tile count, and the two forms
    // round differently -- that mode promises bit-identical rows whatever the batch)
    // (a sub-layer whose output feeds an SE: the fused kernel does not produce its row sums)
    if (!h->row_independent && S.separable && S.dw.d_ftaps && h->gemm_mode == 3 && want_amax && cur_amax.p && WF.d_w16 &&
        !S.se.d_w1 && B.groups == 1 && !S.norm.d_gamma &&   // (no grouped form of the fused kernel, no raw store)
        !(last_sub && B.has_res && !B.fused_res) &&
        // a folded residual must come from a 256-channel block input (K = 256 + 256): the kernel's second K range is 4 chunks
        (fuse_res ? (blk_amax.p && blk_ld == cur_ld && WF.cin == 2 * S.dw.cin && B.fused_k1 == S.dw.cin) : WF.cin == S.dw.cin) &&
        cur_ld % kTimeTile == 0 && !enc_out && (f_cols = fused_tile_cols(h, batch, cur_ld)) != 0)
      return f_cols;
    return 0;
  }

  // The fused kernel for sub-block S, where fused_cols allows it.  1: taken, its output is the current tensor; 0: not taken --
  // not allowed, or the shape is not covered after all -- and nothing was committed; < 0: an error
  int try_fused(const Block& B, const SubBlock& S, bool last_sub, bool enc_out, bool fuse_res) {
    const ConvLayer& WF = fuse_res ? B.fused : S.pw;
    const int f_cols = fused_cols(B, S, last_sub, enc_out, fuse_res, WF);
    if (!f_cols) return 0;
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
    if (e < 0) return 0;   // shape not covered after all: the two-kernel path (nothing was committed)
    commit(kPlanFused, dst, cur, f.x2, nullptr);
    rot.wrote(buf_of(dst));
    cur = dst;
    cur_amax = f.amax_y;
    return 1;
  }

  // One sub-layer of block B: the fused kernel where it applies, else its depthwise conv and 1x1 GEMM as two kernels (or its
  // K-tap conv as one implicit GEMM), then its GroupNorm and SqueezeExcite
  int sub_block(const Block& B, const SubBlock& S, bool last_sub) {
    const bool enc_out = last_block && last_sub;   // this sub-layer writes the encoder output
    const bool fuse_res = last_sub && B.fused_res;
    if (const int taken = try_fused(B, S, last_sub, enc_out, fuse_res)) return taken < 0 ? taken : 0;
    const float* gx = cur;
    int64_t gx_ld = cur_ld, g_T = cur_T;
    const int32_t* g_lens = nullptr;
    AmaxTab gx_amax = cur_amax;
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
        return fail(VASR_ERR_WORKSPACE, "maxima table too small for depthwise layer of block %zu", blk_i);
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
      return fail(VASR_ERR_UNSUPPORTED, "block %zu: residual across a strided block", blk_i);
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
    return 0;
  }

  // every block: its input's pane copy, its residual branch, its sub-layers
  int run() {
    for (blk_i = 0; blk_i < h->blocks.size(); ++blk_i) {
      const Block& B = h->blocks[blk_i];
      last_block = blk_i + 1 == h->blocks.size();
      blk_in = cur;
      blk_ld = cur_ld;
      blk_amax = cur_amax;
      // the block input stays where it is (the fused residual reads it until the block's last GEMM), an unfused residual result
      // takes the third rotation buffer that is not the block input, the sub-block outputs go where the rotation sends them
      const int blk_buf = buf_of(blk_in);
      rot.begin_block(blk_buf < kBufRot ? blk_buf : kBufNone, B.has_res && !B.fused_res);
      R = bufs[rot.pp[2]];
      panes = reinterpret_cast<float*>(ws + p.pane);
      pane_bs = (int64_t)h->pane_c_max * cur_ld;
      if (int rc = keep_pane(B)) return rc;
      // residual panes' masks: the block input lengths; a last block's residual keeps its padding columns (the encoder output's)
      res_zero = last_block ? nullptr : lens(B.first_step);
      if (int rc = residual_branch(B)) return rc;
      for (size_t r = 0; r < B.subs.size(); ++r)
        if (int rc = sub_block(B, B.subs[r], r + 1 == B.subs.size())) return rc;
    }
    return 0;
  }
};

}  // namespace

// Encoder over an input [B][feat_in][x_ld]; writes [B][c_last][out_ld] (T1 valid frames).
// enc_amax (optional): receives the maxima table of the encoder output when one was published (fp16-split mode, padded
// output pitch), for the CTC head of the fused path; the table lives in the workspace until the next encoder pass.
// rec (vasr_plan_buffers): a dry pass -- nothing is launched and no device memory is touched, every launch the pass would
// make is recorded as (kind, dst, src, src2, res) in buffer numbers (vasr_host.h); ws is then any base address.
int run_encoder(vasr_handle* h, const float* x, int64_t x_ld, int64_t T, const int64_t* seq, int batch, float* out,
                int64_t out_ld, float* enc_len, char* ws, const WsPlan& p, hipStream_t st, AmaxTab* enc_amax,
                const int64_t* wav_len, const int32_t** own_frames, bool chain_done, PlanRec* rec) {
  EncoderPass pass(h, x, x_ld, T, batch, out, out_ld, ws, p, st, enc_amax, rec);
  // row-independent mode (fused path): everything the CTC head sees of a row must depend on that row alone, also the
  // fp16 scale of its input -- the encoder output's maxima are then taken over the frames an unbatched call on the row
  // would produce, and the head zeroes the columns behind them (they are not decoded in this mode)
  const bool own = h->row_independent && wav_len != nullptr;
  // (the fused path has run the chain as extra workgroups of its normalisation launch: launch_normalize_chain)
  if (!chain_done && !pass.dry)
    launch_len_chain(seq, batch, h->d_steps, (int)h->steps.size(), pass.lens_tab, enc_len, st, own ? wav_len : nullptr,
                     h->fe.hop_length, (int)p.T1);
  pass.own_tab = own ? pass.lens((int)h->steps.size() + 1) : nullptr;
  if (own_frames) *own_frames = pass.own_tab;
  if (int rc = pass.run()) return rc;
  if (enc_amax) *enc_amax = pass.cur_amax;
  return pass.dry ? 0 : check_launch("encoder");
}

// The CTC head over the encoder output [B][dec_feat_in][ld]: its GEMM, then log-softmax and arg-max in one launch
int run_decoder(vasr_handle* h, const float* encp, int64_t ld, int64_t T1, int batch, float* logits, float* logp,
                int64_t* pred, hipStream_t st, AmaxTab enc_amax, const int32_t* own_frames) {
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

}  // namespace vasr
