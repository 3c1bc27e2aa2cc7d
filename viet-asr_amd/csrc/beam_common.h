// Device-side pieces shared by the beam-search kernels (beam_wave.hip: one wavefront per utterance, batches;
// beam_group.hip: an utterance on four wavefronts of a compute unit, the serving latency): hashing,
// order-preserving score bits, the hashed back-off n-gram model (KenLM BaseScore semantics, pyctcdecode's LanguageModel.score
// on top), log(r >= 1) in fp64 without the library call, wavefront-wide scans / reductions on the DPP data path -- and the
// steps of the search both kernels run (beam layout, children, LM scoring, radix-select digits, final pass and trace-back).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "vasr_internal.h"

namespace vasr {
namespace beam_detail {

constexpr int kMaxCtx = 4;      // LM order <= 5
constexpr int kMaxClasses = 128;
constexpr int kMaxBeams = 128;
constexpr unsigned long long kFnvOffset = 1469598103934665603ull, kFnvPrime = 1099511628211ull;
constexpr double kFix = 17592186044416.0;  // 2^44

__host__ __device__ inline unsigned long long hmix(unsigned long long h, unsigned long long v) {
  return (h ^ (v + 1)) * kFnvPrime;
}
__device__ inline long long ord64(double d) {  // order-preserving map double -> signed 64
  long long b = __double_as_longlong(d);
  return b >= 0 ? b : (long long)(0x8000000000000000ull ^ (unsigned long long)~b) ;
}
__device__ inline double unord64(long long o) {
  long long b = o >= 0 ? o : (long long)~(0x8000000000000000ull ^ (unsigned long long)o);
  return __longlong_as_double(b);
}

// The n-gram model on the device (vasr_lm_create, include/vasr.h): two open-addressing tables of 16-BYTE entries in
// HBM -- one load returns key and value -- with power-of-two capacities 2^lg, linear probing from the home slot
// lm_home(key, lg) = ((u32)(key ^ key >> 32) * 0x9E3779B1) >> (32 - lg)  (the keys are FNV-style products of small word ids:
// their entropy sits in bits 0-24 and 40+, any plain bit field of them clusters -- a first version that used bits 17.. sent
// 20 000 unigrams to 256 home slots and probe chains ran to thousands of entries):
//   vocabulary  {u64 key = hash of the word's label ids | 1, i32 word id, u32 flags: bit 0 = member of pyctcdecode's unigram set}
//   n-grams     {u64 key | 1, f32 log10 p, f32 log10 back-off}; the key of (w_1 .. w_n) is folded from the LAST word
//               backwards, key = hmix(... hmix(hmix(offset, w_n), w_{n-1}) ..., w_1): the keys of all suffixes of a history
//               come out of one chain, and a back-off walk needs every one of them.
// and, when the decoder was built with a unigram list (pyctcdecode's behaviour for an ".arpa" path: LanguageModel's
// unigram_set + CharTrie), the NODES of the character trie as a set of 64-bit keys:
//   trie        2^tlg buckets of TWO u64 keys (16 bytes, one load): key = hash of a word PREFIX's label ids | 1 -- the rolling
//               hash every beam already carries for its pending word -- for every non-empty prefix of every word of the
//               unigram set; home bucket lm_home(key, tlg), linear probing over buckets, a bucket with a free cell ends the walk.
struct LmView {
  const uint4* vocab; int vcap, vlg;      // capacity 2^vlg
  const uint4* ngram; int ncap, nlg;
  const ulonglong2* trie; int tlg;        // trie == nullptr: no unigram list (every partial word is "OOV")
  int order, bos, eos, unk;
  float alpha, beta, unk_offset;
};

inline LmView make_lm_view(const BeamLm* lm) {
  LmView v{};
  if (!lm) return v;
  v.vocab = static_cast<const uint4*>(lm->vocab); v.vcap = lm->vcap; v.ngram = static_cast<const uint4*>(lm->ngram);
  v.ncap = lm->ncap; v.order = lm->order; v.bos = lm->bos;
  v.vlg = 31 - __builtin_clz((unsigned)lm->vcap); v.nlg = 31 - __builtin_clz((unsigned)lm->ncap);
  v.trie = static_cast<const ulonglong2*>(lm->trie);
  v.tlg = lm->trie ? 31 - __builtin_clz((unsigned)lm->tbuckets) : 0;
  v.eos = lm->eos; v.unk = lm->unk; v.alpha = lm->alpha; v.beta = lm->beta; v.unk_offset = lm->unk_offset;
  return v;
}

__device__ inline unsigned long long entry_key(const uint4& e) { return ((unsigned long long)e.y << 32) | e.x; }
__host__ __device__ inline int lm_home(unsigned long long k, int lg) {
  return (int)((((unsigned)k ^ (unsigned)(k >> 32)) * 0x9E3779B1u) >> (32 - lg));
}

// word id of a committed word (-1: not in the n-gram model's vocabulary); *in_set: member of the unigram set (entry flags bit 0)
__device__ __forceinline__ int lm_word_id(const LmView& lm, unsigned long long whash, bool* in_set) {
  const unsigned long long k = whash | 1ull;
  *in_set = false;
  for (int i = lm_home(k, lm.vlg), n = 0; n < lm.vcap; ++n, i = (i + 1) & (lm.vcap - 1)) {
    const uint4 e = lm.vocab[i];
    const unsigned long long ek = entry_key(e);
    if (ek == k) { *in_set = (e.w & 1u) != 0u; return (int)e.z; }
    if (ek == 0) break;
  }
  return -1;  // out of vocabulary
}

// pygtrie CharTrie.has_node(partial word) on the key set: `first` is the home bucket, requested by the caller long before
// the answer is needed (the expand step issues it, the score step -- a table phase and, in the four-wavefront kernel, a
// barrier later -- consumes it); only a FULL bucket that holds neither the key nor a free cell sends the lane on (the next
// bucket is 16 bytes further: as a rule the same cache line).
__device__ __forceinline__ ulonglong2 trie_first(const LmView& lm, unsigned long long whash) {
  return lm.trie[lm_home(whash | 1ull, lm.tlg)];
}
__device__ __forceinline__ bool trie_has_node(const LmView& lm, unsigned long long whash, ulonglong2 first) {
  const unsigned long long k = whash | 1ull;
  const int nb = 1 << lm.tlg;
  int i = lm_home(k, lm.tlg);
  ulonglong2 e = first;
  for (int n = 0; n < nb; ++n) {
    if (e.x == k || e.y == k) return true;
    if (e.x == 0ull || e.y == 0ull) return false;
    i = (i + 1) & (nb - 1);
    e = lm.trie[i];
  }
  return false;
}

// the rest of a probe chain whose first entry `e` was neither the key nor empty (rare at <= 50 % load)
__device__ __forceinline__ bool lm_probe_on(const LmView& lm, unsigned long long k, uint4 e, float2* out) {
  int i = lm_home(k, lm.nlg);
  for (int c = 0; c < lm.ncap; ++c) {
    const unsigned long long ek = entry_key(e);
    if (ek == k) { *out = make_float2(__uint_as_float(e.z), __uint_as_float(e.w)); return true; }
    if (ek == 0) return false;
    i = (i + 1) & (lm.ncap - 1);
    e = lm.ngram[i];
  }
  return false;
}

// KenLM BaseScore on a full history: log10 p(w | ctx) with back-off.  The walk "longest n-gram, else back-off weight of
// its context + the next shorter one" needs the entries of (ctx[s..], w) and of (ctx[s..]) for every start s: their
// keys come from two incremental chains and ALL first probes are requested before any is looked at -- one trip to
// L2 / HBM for the whole walk instead of one per step (ten dependent trips for a trigram model whose words are unseen
// together; the LM was 3 100 of the 14 600 cycles of an average frame).
__device__ __forceinline__ float lm_base_score(const LmView& lm, const int* ctx, int w) {
  int ids[kMaxCtx];               // usable history, most recent LAST
  int n = 0;
  for (int i = 0; i < kMaxCtx; ++i)
    if (ctx[i] >= 0 && kMaxCtx - i <= lm.order - 1) ids[n++] = ctx[i];
  // kf[j]: key of (ids[n-j .. n-1], w), j = 0 .. n (j history words);  kc[j]: key of (ids[n-j .. n-1]), j = 1 .. n
  unsigned long long kf[kMaxCtx + 1], kc[kMaxCtx + 1];
  uint4 ef[kMaxCtx + 1], ec[kMaxCtx + 1];
  unsigned long long hf = hmix(kFnvOffset, (unsigned long long)w), hc = kFnvOffset;
  kf[0] = hf | 1ull;
  kc[0] = 0;
#pragma unroll
  for (int j = 1; j <= kMaxCtx; ++j) {
    if (j <= n) {
      const unsigned long long id = (unsigned long long)ids[n - j];
      hf = hmix(hf, id); hc = hmix(hc, id);
      kf[j] = hf | 1ull; kc[j] = hc | 1ull;
    } else { kf[j] = 0; kc[j] = 0; }
  }
#pragma unroll
  for (int j = 0; j <= kMaxCtx; ++j) {
    ef[j] = make_uint4(0, 0, 0, 0); ec[j] = make_uint4(0, 0, 0, 0);
    if (j <= n) ef[j] = lm.ngram[lm_home(kf[j], lm.nlg)];
    if (j >= 1 && j <= n) ec[j] = lm.ngram[lm_home(kc[j], lm.nlg)];
  }
  float score = 0.f;
  bool done = false;
#pragma unroll
  for (int j = kMaxCtx; j >= 0; --j) {          // longest first
    if (j > n || done) continue;
    float2 v;
    if (lm_probe_on(lm, kf[j], ef[j], &v)) { score += v.x; done = true; continue; }
    if (j == 0) break;
    if (lm_probe_on(lm, kc[j], ec[j], &v)) score += v.y;     // back-off weight of the context
  }
  if (!done) {   // unigram missing: fall back to <unk>
    const unsigned long long ku = hmix(kFnvOffset, (unsigned long long)lm.unk) | 1ull;
    float2 v;
    if (lm_probe_on(lm, ku, lm.ngram[lm_home(ku, lm.nlg)], &v)) score += v.x; else score += -100.f;
  }
  return score;
}

// pyctcdecode LanguageModel.score (alpha * log10 * ln10 + beta, unk offset, optional </s>).  The unk offset: "word not in
// kenlm_model", and -- with a (non-empty) unigram set -- also "word not in unigram_set" (a word of the model whose 1-gram line
// carries no back-off weight is outside the set pyctcdecode reads from the ARPA file: oracle/beam_oracle.py header)
__device__ __forceinline__ float lm_word_score(const LmView& lm, const int* ctx, unsigned long long whash, bool eos, int* wid_out) {
  bool in_set;
  int wid = lm_word_id(lm, whash, &in_set);
  const bool oov = wid < 0;
  if (oov) wid = lm.unk;
  float s = lm_base_score(lm, ctx, wid);
  if (oov || (lm.trie != nullptr && !in_set)) s += lm.unk_offset;
  if (eos) {
    int c2[kMaxCtx];
    for (int i = 0; i < kMaxCtx - 1; ++i) c2[i] = ctx[i + 1];
    c2[kMaxCtx - 1] = wid;
    s += lm_base_score(lm, c2, lm.eos);
  }
  *wid_out = wid;
  return lm.alpha * s * 2.302585092994046f + lm.beta;
}

// pyctcdecode LanguageModel.score_partial_token: unk_offset * is_oov, stretched by len / 6 beyond six characters.  is_oov: 1.0
// without a character trie, else "the partial word is not a node of it" (the beams carry that as a meta bit)
__device__ inline float partial_penalty(float unk_offset, int wlen, bool is_oov) {
  if (wlen <= 0 || !is_oov) return 0.f;
  float u = unk_offset;
  if (wlen > 6) u = u * (float)wlen / 6.0f;
  return u;
}

// log(r) for r in [1, 2^20): exponent split + atanh series (10 odd terms at |s| <= 0.1716: < 1e-16 relative).
// The library log costs ~2400 cycles per wavefront here, every merged prefix needs one per frame.
__device__ inline double log_ge1(double r) {
  long long bits = __double_as_longlong(r);
  int e = (int)((bits >> 52) & 0x7ff) - 1023;
  double m = __longlong_as_double((bits & 0x000fffffffffffffll) | 0x3ff0000000000000ll);   // [1, 2)
  if (m > 1.4142135623730951) { m *= 0.5; e += 1; }                                         // [0.7071, 1.4142]
  // 1/(m+1): hardware estimate + two Newton steps (full IEEE division is ~25 fp64 instructions, 8 cycles each)
  const double d = m + 1.0;
  double r1 = __builtin_amdgcn_rcp(d);
  r1 = fma(fma(-d, r1, 1.0), r1, r1);
  r1 = fma(fma(-d, r1, 1.0), r1, r1);
  const double s = (m - 1.0) * r1, z = s * s;
  double p = 1.0 / 21.0;
  p = fma(p, z, 1.0 / 19.0); p = fma(p, z, 1.0 / 17.0); p = fma(p, z, 1.0 / 15.0); p = fma(p, z, 1.0 / 13.0);
  p = fma(p, z, 1.0 / 11.0); p = fma(p, z, 1.0 / 9.0); p = fma(p, z, 1.0 / 7.0); p = fma(p, z, 1.0 / 5.0);
  p = fma(p, z, 1.0 / 3.0); p = fma(p, z, 1.0);
  return fma((double)e, 0.6931471805599453, 2.0 * s * p);
}

// Wavefront-wide inclusive scan / max on the DPP data path (row shifts + row broadcasts, ~20 VALU instructions).
// The __shfl_up / __shfl_xor forms go through ds_bpermute: six dependent LDS round trips, ~700 cycles per scan, and
// the frame loop runs five or more of them.
template <int CTRL>
__device__ inline int dpp_mov(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }

__device__ inline int wave_scan_incl(int v) {
  const int lane = threadIdx.x & 63, rl = lane & 15;
  int x = v, t;
  t = dpp_mov<0x111>(x); if (rl >= 1) x += t;              // row_shr:1
  t = dpp_mov<0x112>(x); if (rl >= 2) x += t;              // row_shr:2
  t = dpp_mov<0x114>(x); if (rl >= 4) x += t;              // row_shr:4
  t = dpp_mov<0x118>(x); if (rl >= 8) x += t;              // row_shr:8
  t = dpp_mov<0x142>(x); if ((lane & 31) >= 16) x += t;    // row_bcast:15
  t = dpp_mov<0x143>(x); if (lane >= 32) x += t;           // row_bcast:31
  return x;
}

__device__ inline unsigned wave_max_u32(unsigned v) {
  const int lane = threadIdx.x & 63, rl = lane & 15;
  unsigned x = v, t;
  t = (unsigned)dpp_mov<0x111>((int)x); if (rl >= 1) x = max(x, t);
  t = (unsigned)dpp_mov<0x112>((int)x); if (rl >= 2) x = max(x, t);
  t = (unsigned)dpp_mov<0x114>((int)x); if (rl >= 4) x = max(x, t);
  t = (unsigned)dpp_mov<0x118>((int)x); if (rl >= 8) x = max(x, t);
  t = (unsigned)dpp_mov<0x142>((int)x); if ((lane & 31) >= 16) x = max(x, t);
  t = (unsigned)dpp_mov<0x143>((int)x); if (lane >= 32) x = max(x, t);
  return (unsigned)__builtin_amdgcn_readlane((int)x, 63);
}

__device__ inline unsigned wave_or_u32(unsigned v) {
  const int lane = threadIdx.x & 63, rl = lane & 15;
  unsigned x = v, t;
  t = (unsigned)dpp_mov<0x111>((int)x); if (rl >= 1) x |= t;
  t = (unsigned)dpp_mov<0x112>((int)x); if (rl >= 2) x |= t;
  t = (unsigned)dpp_mov<0x114>((int)x); if (rl >= 4) x |= t;
  t = (unsigned)dpp_mov<0x118>((int)x); if (rl >= 8) x |= t;
  t = (unsigned)dpp_mov<0x142>((int)x); if ((lane & 31) >= 16) x |= t;
  t = (unsigned)dpp_mov<0x143>((int)x); if (lane >= 32) x |= t;
  return (unsigned)__builtin_amdgcn_readlane((int)x, 63);
}

// max of a signed 64-bit value over the wavefront: high words first, then the low words of the lanes that tie
__device__ inline long long wave_max_i64(long long v) {
  const unsigned long long u = (unsigned long long)v ^ 0x8000000000000000ull;
  const unsigned hi = (unsigned)(u >> 32), lo = (unsigned)u;
  const unsigned hmax = wave_max_u32(hi);
  const unsigned lmax = wave_max_u32(hi == hmax ? lo : 0u);
  return (long long)((((unsigned long long)hmax << 32) | lmax) ^ 0x8000000000000000ull);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The steps both kernels run, written once: the two kernels give the same bits because they run this code.  Templated on
// the kernel's LDS struct (beam_wave.hip WaveLds, beam_group.hip GroupLds<W>), whose beam fields have the same names and
// layout: key / whash / logit / lm_text / meta / ctx / commit_lmd / commit_wid [2][kMaxBeams] (buffer cur holds the beams of
// the current frame), the merge table tkey, sel_lgt / sel_tot / fin [kMaxBeams] and cmix [kMaxClasses].
// ---------------------------------------------------------------------------------------------------------------------------

constexpr int kTbRows = 12;               // back-pointer rows per trace-back batch (6 KB, two batches in LDS)
constexpr int kLpFrames = 8;              // frames of log-probs per staging batch
constexpr int kLpRegs = kLpFrames * kMaxClasses / 64;   // floats a lane holds of the batch in flight
constexpr int kChars = 3072;              // characters of a transcript assembled in LDS (longer ones go through HBM)

// a beam's meta word: (last + 1) [7:0] (0 = none, blank = V + 1) | wlen [23:8] | cached [24] | commit_valid [25] | pending
// word is "OOV" [26] (is_oov of pyctcdecode's score_partial_token: always with no unigram list, else "not a node of the
// character trie")
constexpr unsigned kMetaCached = 1u << 24, kMetaCommit = 1u << 25, kMetaOov = 1u << 26;
constexpr int kSrcOov = 1 << 16;          // a pair record (beam << 8 | class) carries its child's "OOV" bit here
__device__ inline int meta_last(unsigned m) { return (int)(m & 0xffu) - 1; }
__device__ inline int meta_wlen(unsigned m) { return (int)((m >> 8) & 0xffffu); }
__device__ inline unsigned make_meta(int last, int wlen, unsigned flags) {
  return (unsigned)(last + 1) | ((unsigned)min(wlen, 0xffff) << 8) | flags;
}

// Orders the LDS traffic of a wavefront's phases for the COMPILER (the hardware executes one wavefront's LDS operations in
// order): lanes read what other lanes of the same wavefront wrote, which per-thread alias analysis cannot see.
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline int lane_id() { return (int)(threadIdx.x & 63); }
__device__ inline int rank_in(unsigned long long mask) {   // set bits of `mask` below this lane
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// Table key of pair src = (beam bi << 8 | character c) -- (prefix text, last character): the prefix grows unless c is blank,
// a repeat, or a space with no word pending; the "last character" part is a per-class constant (cmix).  The expand steps
// form the same key inline, next to the home slot of the pair.
template <class L>
__device__ __forceinline__ unsigned long long pair_key(const L& S, int cur, int V, int space_id, int src) {
  const int bi = (src >> 8) & 255, c = src & 255;
  const unsigned m = S.meta[cur][bi];
  const bool grows = !(c == V || c == meta_last(m)) && !(c == space_id && meta_wlen(m) == 0);
  const unsigned long long key = S.key[cur][bi];
  return ((grows ? hmix(key, (unsigned long long)c) : key) ^ S.cmix[c]) | 1ull;
}

// One new beam at rank r from pair src = (parent bi << 8 | character c) with merged logit bits lgt: the parent's fields are
// gathered from buffer cur, the child goes to the other one, one back-pointer word per rank and frame (row t of bp).
// Returns whether c is a character (not blank).
template <class L>
__device__ __forceinline__ bool build_child(L& S, int cur, int V, int space_id, bool use_lm, unsigned int* bp, int t, int r,
                                            int src, long long lgt, bool has_space) {
  const int nxt = cur ^ 1;
  const int bi = (src >> 8) & 255, c = src & 255;
  const unsigned m = S.meta[cur][bi];
  const int last = meta_last(m), wlen = meta_wlen(m);
  const bool stay = (c == V || c == last);
  unsigned long long key = S.key[cur][bi], whash = S.whash[cur][bi];
  float lm_text = S.lm_text[cur][bi];
  const int4 ctx_p = *reinterpret_cast<const int4*>(&S.ctx[cur][bi][0]);
  int4 ctx_n = ctx_p;
  const float p_lmd = S.commit_lmd[cur][bi];
  const int p_wid = S.commit_wid[cur][bi];
  int wlen_new = wlen;
  unsigned int appended = 0;
  unsigned flags = (src & kSrcOov) ? kMetaOov : 0u;       // (the score step decided it: same pending word, same bit)
  if (stay) {
    // same text and pending word as the parent: in the LM cache if the parent was, or if this frame put it there; the
    // commit score of the pending word is inherited with them
    if ((m & kMetaCached) || (has_space && wlen > 0)) flags |= kMetaCached;
    flags |= m & kMetaCommit;
  } else if (c == space_id) {
    if (wlen > 0) {
      key = hmix(key, (unsigned long long)c);
      appended = c + 1;
      if (use_lm) {
        lm_text += p_lmd;
        ctx_n = make_int4(ctx_p.y, ctx_p.z, ctx_p.w, p_wid);
      }
      wlen_new = 0; whash = kFnvOffset;
    }
  } else {
    key = hmix(key, (unsigned long long)c);
    whash = hmix(whash, (unsigned long long)c);
    wlen_new = wlen + 1;
    appended = c + 1;
  }
  S.key[nxt][r] = key; S.whash[nxt][r] = whash;
  S.logit[nxt][r] = __longlong_as_double(lgt);
  S.lm_text[nxt][r] = lm_text;
  S.meta[nxt][r] = make_meta(c, wlen_new, flags);
  *reinterpret_cast<int4*>(&S.ctx[nxt][r][0]) = ctx_n;
  S.commit_lmd[nxt][r] = p_lmd;
  S.commit_wid[nxt][r] = p_wid;
  bp[(int64_t)t * kMaxBeams + r] = ((unsigned)bi << 8) | appended;
  return c != V;
}

// Step 2 for live beam i of a frame with ' ' among its candidates: returns whether "text + pending word" enters
// pyctcdecode's LM score cache (the log, key in *h: once per lineage), and gives the pending word the LM score a commit
// would add (commit_lmd / commit_wid, meta bit kMetaCommit: once per (text, word), children that keep both inherit it).
template <class L>
__device__ __forceinline__ bool lm_commit_step(L& S, int cur, int i, int space_id, const LmView& lm, unsigned long long* h) {
  const unsigned m = S.meta[cur][i];
  if (meta_wlen(m) == 0) return false;
  *h = hmix(S.key[cur][i], (unsigned long long)space_id) | 1ull;
  if (!(m & kMetaCommit)) {
    int ctx[kMaxCtx];
#pragma unroll
    for (int q = 0; q < kMaxCtx; ++q) ctx[q] = S.ctx[cur][i][q];
    int w;
    S.commit_lmd[cur][i] = lm_word_score(lm, ctx, S.whash[cur][i], false, &w);
    S.commit_wid[cur][i] = w;
    S.meta[cur][i] = m | kMetaCommit;
  }
  return !(m & kMetaCached);
}

// The LM part of pair (parent bi, character c)'s combined score: the LM score of the parent's committed text, pyctcdecode's
// partial-word penalty of the child's pending word and, when ' ' commits a word, its commit score (filled by step 2).  The
// child's is_oov goes into *src (kSrcOov).  wnew / tfirst: the child's pending-word hash and its trie home bucket, requested
// by the expand step (read only with a trie).  Every lane of the wavefront calls it (a ballot inside).
template <class L>
__device__ __forceinline__ float pair_lm_part(const L& S, int cur, int bi, int c, int V, int space_id, const LmView& lm,
                                              bool trie, unsigned long long wnew, ulonglong2 tfirst, int* src) {
  const unsigned m = S.meta[cur][bi];
  const int last = meta_last(m), wlen = meta_wlen(m);
  const bool stay = (c == V || c == last);
  const int wlen_new = stay ? wlen : (c == space_id ? 0 : wlen + 1);
  const float commit = S.commit_lmd[cur][bi];
  // is_oov of the child's pending word: the parent's when the word stays; once outside the trie, outside for good
  bool oov = true;
  if (trie) {
    if (stay) oov = (m & kMetaOov) != 0u;
    else if (c != space_id && !(wlen > 0 && (m & kMetaOov))) oov = !trie_has_node(lm, wnew, tfirst);
  }
  if (oov) *src |= kSrcOov;
  // partial_penalty(unk_offset, wlen_new, oov), its division only when some lane's pending word is longer than six
  // characters (as a select the compiler runs the ~12-instruction division in every frame)
  float pen = (wlen_new > 0 && oov) ? lm.unk_offset : 0.f;
  if (__ballot(wlen_new > 6) != 0ull) pen = wlen_new > 6 ? pen * (float)wlen_new / 6.0f : pen;
  return S.lm_text[cur][bi] + pen + ((!stay && c == space_id && wlen > 0) ? commit : 0.f);
}

// One digit of a radix select: the bucket that holds the want-th largest key.  Lane l owns buckets 255 - 4 l ... 252 - 4 l,
// counts cnt[0..3] (the largest digit first), and `above` keys lie in the buckets of the lanes before it; exactly one lane
// finds the bucket (more keys than wanted, want >= 1).  `want` becomes the rank inside the bucket; *whole: the whole
// bucket is taken.
__device__ __forceinline__ int radix_bucket(const int (&cnt)[4], int above, int* want, int* whole) {
  int f_bucket = -1, f_want = 0, f_whole = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (above < *want && *want <= above + cnt[j]) { f_bucket = 255 - (4 * lane_id() + j); f_want = *want - above; f_whole = cnt[j] == *want - above; }
    above += cnt[j];
  }
  const unsigned long long fm = __ballot(f_bucket >= 0);
  const int fl = __ffsll((long long)fm) - 1;
  const int bucket = __builtin_amdgcn_readlane(f_bucket, fl);
  *want = __builtin_amdgcn_readlane(f_want, fl);
  *whole = __builtin_amdgcn_readlane(f_whole, fl);
  return bucket;
}

// The first steps of the final passes (final_pass, final_pass_nbest), ONE wavefront (the caller has made every
// back-pointer row and log entry of the search visible to it): commit pending words (LM score with </s>) and leave per
// beam i < nb of buffer cur its combined final score fin[i] (S.fin), final text key fkey[i] (S.sel_lgt) and last-frame
// combined score frank[i] (S.sel_tot).  eoslog holds n_log keys; mark: an int[kTab] of the kernel's LDS that is free now,
// kTab = the size of the (empty) merge table S.tkey, whose words the pending-word lookup uses.
template <class L, int kTab>
__device__ __forceinline__ void final_scores(L& S, int (&mark)[kTab], int cur, int nb, int n_log, int space_id, bool use_lm,
                                             const LmView& lm, unsigned long long* eoslog) {
  static_assert(sizeof(S.tkey) == sizeof(unsigned long long) * kTab, "mark[] has a cell per merge-table slot");
  const int lane = lane_id();
  // Is "text + pending word" in pyctcdecode's LM cache (then its cached score, WITHOUT </s>, is what the final pass
  // uses)?  Known for beams whose own lineage put it there (`cached`); the others look their hash up in eoslog: their
  // hashes go into the (idle, empty) merge table, the wavefront walks the log and marks the hashes it meets.
  int in_cache[2] = {0, 0};
  if (use_lm) {
    int myslot[2] = {-1, -1};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = lane + 64 * j;
      if (i < nb) {
        const unsigned m = S.meta[cur][i];
        if (meta_wlen(m) > 0) {
          in_cache[j] = (m & kMetaCached) ? 1 : 0;
          if (!in_cache[j] && n_log > 0) {
            const unsigned long long k = hmix(S.key[cur][i], (unsigned long long)space_id) | 1ull;
            int q = (int)((k >> 17) & (kTab - 1));
            while (true) {
              const unsigned long long old = atomicCAS(&S.tkey[q], 0ull, k);
              if (old == 0ull || old == k) break;
              q = (q + 1) & (kTab - 1);
            }
            myslot[j] = q;
          }
        }
      }
    }
    for (int i = lane; i < kTab; i += 64) mark[i] = 0;
    wave_sync();
    for (int q = lane; q < n_log; q += 64) {
      const unsigned long long k = __hip_atomic_load(&eoslog[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int i = (int)((k >> 17) & (kTab - 1));; i = (i + 1) & (kTab - 1)) {
        const unsigned long long e = S.tkey[i];
        if (e == k) { mark[i] = 1; break; }
        if (e == 0) break;
      }
    }
    wave_sync();
#pragma unroll
    for (int j = 0; j < 2; ++j) if (myslot[j] >= 0) in_cache[j] = mark[myslot[j]];
    wave_sync();
  }
  // per beam: combined final score, final text key, last-frame combined score (pyctcdecode keeps its beams sorted by it)
  double* fin = S.fin;                                                     // [kMaxBeams]
  unsigned long long* fkey = reinterpret_cast<unsigned long long*>(S.sel_lgt);   // [kMaxBeams]
  double* frank = reinterpret_cast<double*>(S.sel_tot);                    // [kMaxBeams]
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = lane + 64 * j;
    if (i < nb) {
      const unsigned m = S.meta[cur][i];
      const int wlen = meta_wlen(m);
      double total = S.logit[cur][i];
      if (use_lm) {
        float lmv = S.lm_text[cur][i];
        if (wlen > 0) {
          int ctx[kMaxCtx], wid;
#pragma unroll
          for (int q = 0; q < kMaxCtx; ++q) ctx[q] = S.ctx[cur][i][q];
          lmv += lm_word_score(lm, ctx, S.whash[cur][i], !in_cache[j], &wid);
        }
        total += (double)lmv;
      }
      fin[i] = total;
      fkey[i] = wlen > 0 ? hmix(S.key[cur][i], (unsigned long long)space_id) : S.key[cur][i];
      frank[i] = S.logit[cur][i] + (use_lm ? (double)(S.lm_text[cur][i] + partial_penalty(lm.unk_offset, wlen, (m & kMetaOov) != 0u)) : 0.0);
    }
  }
  wave_sync();
}

// Merge by text: log-sum-exp of the LOGIT scores, as pyctcdecode does.  "abc" with the word still pending and "abc "
// with it committed are the same final text but not the same LM part (only the pending word is scored with </s>):
// pyctcdecode's _merge_beams overwrites the group's entry with every further member it meets while walking its
// score-sorted beam list, so the member with the LOWEST last-frame score provides the LM part.  merge_group: the group of
// beam i (its first member, final text key k), after final_scores: returns its combined score, *logit its logit score.
// (Exact ties -- of the last-frame scores inside a group, of the groups' merged scores -- go to the larger key, not to the
// earlier beam: the beams' order is not the same in the two kernels, see their selects.)
template <class L>
__device__ __forceinline__ double merge_group(const L& S, int cur, int nb, int i, unsigned long long k, double* logit) {
  const double* fin = S.fin;
  const unsigned long long* fkey = reinterpret_cast<const unsigned long long*>(S.sel_lgt);
  const double* frank = reinterpret_cast<const double*>(S.sel_tot);
  double m = S.logit[cur][i];
  int rep = i;
  for (int j = i + 1; j < nb; ++j)
    if (fkey[j] == k) {
      m = fmax(m, S.logit[cur][j]);
      if (frank[j] < frank[rep] || (frank[j] == frank[rep] && S.key[cur][j] > S.key[cur][rep])) rep = j;
    }
  double ssum = 0;
  for (int j = i; j < nb; ++j) if (fkey[j] == k) ssum += exp(S.logit[cur][j] - m);
  const double merged = (fin[rep] - S.logit[cur][rep]) + m + log(ssum);
  *logit = m + log(ssum);
  return merged;
}

// The final pass of utterance b, ONE wavefront: final_scores, merge identical texts, pick the best, trace it back and write
// out_ids / out_len / out_score.  The trace-back batches use the words of the (empty) merge table S.tkey; overflow: the
// search lost a merge contributor, reported as out_len = -1.
template <class L, int kTab>
__device__ __forceinline__ void final_pass(L& S, int (&mark)[kTab], int cur, int nb, int n_log, bool overflow, int space_id,
                                           bool use_lm, const LmView& lm, unsigned long long* eoslog, const unsigned int* bp,
                                           int frames, int frames_ld, int b, int32_t* out_ids, int32_t* out_len,
                                           float* out_score) {
  const int lane = lane_id();
  final_scores(S, mark, cur, nb, n_log, space_id, use_lm, lm, eoslog);
  const unsigned long long* fkey = reinterpret_cast<const unsigned long long*>(S.sel_lgt);
  // every lane takes the groups whose first member it owns; the best group is the first maximum in beam order
  double my_score = -1e300;
  unsigned long long my_key = 0;
  int my_first = 0x7fffffff;
#pragma unroll 1
  for (int i = lane; i < nb; i += 64) {
    const unsigned long long k = fkey[i];
    bool first = true;
    for (int j = 0; j < i; ++j) if (fkey[j] == k) { first = false; break; }
    if (!first) continue;
    double lg;
    const double merged = merge_group(S, cur, nb, i, k, &lg);
    if (merged > my_score || (merged == my_score && k > my_key)) { my_score = merged; my_key = k; my_first = i; }
  }
  const long long sbest = wave_max_i64(ord64(my_score));
  const long long kbest = wave_max_i64(ord64(my_score) == sbest ? (long long)(my_key ^ 0x8000000000000000ull) : (long long)0x8000000000000000ull);
  const unsigned long long wm = __ballot(ord64(my_score) == sbest && (long long)(my_key ^ 0x8000000000000000ull) == kbest);
  // lowest beam index among the lanes that hold the maximum (a lane's own groups are already in beam order)
  int bi_best = 0x7fffffff;
  for (unsigned long long q = wm; q; q &= q - 1) bi_best = min(bi_best, __builtin_amdgcn_readlane(my_first, __ffsll((long long)q) - 1));
  const double bs = unord64(sbest);

  // ---- trace back: the back-pointer rows come through LDS kTbRows at a time (one batch = one contiguous 6 KB read), the
  //      batch after the current one already requested while the current one is walked; the characters are collected in
  //      LDS and leave as one coalesced write (the workgroup kernel walked 501 dependent HBM round trips and reversed the
  //      text in HBM with one thread: 0.2 ms of a 3 ms search) ----
  unsigned int* rows = reinterpret_cast<unsigned int*>(S.tkey);            // [2][kTbRows][kMaxBeams], from the merge table on
  unsigned short* chars = reinterpret_cast<unsigned short*>(&S.key[0][0]);  // [kChars], aliases the beam keys / hashes / logits
  int32_t* out = out_ids + (int64_t)b * frames_ld;
  const bool in_lds = frames <= kChars;
  int n = 0, cur_b = bi_best;
  bool lead = true;                                          // still inside the trailing whitespace of the text
  constexpr int kRowRegs = kTbRows * kMaxBeams / 4 / 64;     // uint4 per lane and batch
  uint4 rr[kRowRegs];
  const int nbatch = (frames + kTbRows - 1) / kTbRows;       // batch j: frames (frames - (j + 1) kTbRows, frames - j kTbRows]
  auto tb_request = [&](int j) __attribute__((always_inline)) {
    const int t_hi = frames - 1 - j * kTbRows, t_lo = max(0, t_hi - kTbRows + 1), nq = (t_hi - t_lo + 1) * (kMaxBeams / 4);
    const uint4* g = reinterpret_cast<const uint4*>(bp + (int64_t)t_lo * kMaxBeams);
#pragma unroll
    for (int k = 0; k < kRowRegs; ++k) rr[k] = 64 * k + lane < nq ? g[64 * k + lane] : make_uint4(0, 0, 0, 0);
  };
  auto tb_land = [&](int j) __attribute__((always_inline)) {
    uint4* dst = reinterpret_cast<uint4*>(rows + (j & 1) * kTbRows * kMaxBeams);
#pragma unroll
    for (int k = 0; k < kRowRegs; ++k) dst[64 * k + lane] = rr[k];
  };
  if (nbatch > 0) { tb_request(0); tb_land(0); }
  for (int j = 0; j < nbatch; ++j) {
    if (j + 1 < nbatch) tb_request(j + 1);
    wave_sync();
    const int t_hi = frames - 1 - j * kTbRows, t_lo = max(0, t_hi - kTbRows + 1);
    const unsigned int* rb = rows + (j & 1) * kTbRows * kMaxBeams;
    for (int tt = t_hi - t_lo; tt >= 0; --tt) {
      const unsigned int e = rb[tt * kMaxBeams + cur_b];
      const unsigned int ch = e & 255;
      if (ch) {
        const int id = (int)ch - 1;
        if (!(lead && id == space_id)) {                      // normalise trailing whitespace
          lead = false;
          if (in_lds) chars[n] = (unsigned short)id;
          else if (lane == 0) out[frames_ld - 1 - n] = id;    // long transcripts: filled from the back, moved below
          ++n;
        }
      }
      cur_b = (int)(e >> 8);
    }
    if (j + 1 < nbatch) tb_land(j + 1);
    wave_sync();
  }
  if (in_lds) {
    for (int j = lane; j < n; j += 64) out[j] = (int)chars[n - 1 - j];
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // out[j] = out[frames_ld - n + j]: destination indices lie below the source indices and a chunk's loads complete
    // before its stores, so overlapping ranges are safe
    const int off = frames_ld - n;
    if (off > 0) {
      for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        int v = 0;
        if (j < n) v = __hip_atomic_load(&out[off + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (j < n) out[j] = v;
      }
    }
  }
  if (lane == 0) {
    out_len[b] = overflow ? -1 : n;
    out_score[b] = (float)bs;
  }
}

// The last argument of a beam kernel: out_score (float [B]) of the top-1 search, the BeamNbest outputs of the n-best one
template <bool kNbest>
using BeamResult = std::conditional_t<kNbest, BeamNbest, float* __restrict__>;

// The n-best final pass of utterance b (vasr_beam_search_nbest_f32: slot s of utterance b is ids row b nbest + s, frames_ld
// wide, and element b nbest + s of out_len and o's arrays), ONE wavefront: final_scores and merge_group as final_pass, then every text group
// whose combined score is >= best + prune, ranked by combined score, exact ties to the larger key (so slot 0 is what
// final_pass picks), and the first o.nbest of them traced back together: lane l follows slots l and l + 64 through the
// same LDS batches of back-pointer rows, writes each slot's ids from the back of its own row and then moves them to the
// front.  Slots from the count on: length 0, scores -inf; overflow: every slot's length is -1.  Per group the LDS keeps,
// by the index i of its first member: mark[i] = 1, fin[i] its combined score, S.sel_tot[i] its logit score, S.sel_lgt[i]
// its key; mark[kMaxBeams + s] is the first member of slot s (traced back: all members spell the same text).
template <class L, int kTab>
__device__ __forceinline__ void final_pass_nbest(L& S, int (&mark)[kTab], int cur, int nb, int n_log, bool overflow,
                                                 int space_id, bool use_lm, const LmView& lm, unsigned long long* eoslog,
                                                 const unsigned int* bp, int frames, int frames_ld, int b, float prune,
                                                 int32_t* out_ids, int32_t* out_len, const BeamNbest& o) {
  static_assert(kTab >= 2 * kMaxBeams, "mark[] holds the group flags and the slots' beams");
  const int lane = lane_id();
  final_scores(S, mark, cur, nb, n_log, space_id, use_lm, lm, eoslog);
  unsigned long long* fkey = reinterpret_cast<unsigned long long*>(S.sel_lgt);
  double* glogit = reinterpret_cast<double*>(S.sel_tot);
  // a lane's groups: those whose first member is beam lane or lane + 64
  bool own[2] = {false, false};
  double gsc[2] = {-1e300, -1e300}, glg[2] = {0.0, 0.0};
  unsigned long long gk[2] = {0ull, 0ull};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = lane + 64 * j;
    if (i < nb) {
      const unsigned long long k = fkey[i];
      bool first = true;
      for (int q = 0; q < i; ++q) if (fkey[q] == k) { first = false; break; }
      if (first) { own[j] = true; gk[j] = k; gsc[j] = merge_group(S, cur, nb, i, k, &glg[j]); }
    }
  }
  wave_sync();                                                             // every lane is done with fkey / frank
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = lane + 64 * j;
    if (i < kMaxBeams) {
      mark[i] = own[j] ? 1 : 0;
      if (own[j]) { S.fin[i] = gsc[j]; glogit[i] = glg[j]; fkey[i] = gk[j]; }
    }
  }
  const double best = unord64(wave_max_i64(ord64(fmax(gsc[0], gsc[1]))));
  const double thr = best + (double)prune;
  wave_sync();
  // rank by counting: groups ahead = higher combined score, or the same score and a larger key
  int rank[2] = {0, 0};
#pragma unroll 1
  for (int q = 0; q < nb; ++q) {
    if (!mark[q]) continue;
    const double sq = S.fin[q];
    const unsigned long long kq = fkey[q];
#pragma unroll
    for (int j = 0; j < 2; ++j) rank[j] += (sq > gsc[j] || (sq == gsc[j] && kq > gk[j])) ? 1 : 0;
  }
  const int nbest = o.nbest;
  bool kept[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) kept[j] = own[j] && gsc[j] >= thr && rank[j] < nbest;
  const int count = __popcll(__ballot(kept[0])) + __popcll(__ballot(kept[1]));
  const int64_t slot0 = (int64_t)b * nbest;
#pragma unroll
  for (int j = 0; j < 2; ++j)
    if (kept[j]) {
      mark[kMaxBeams + rank[j]] = lane + 64 * j;
      o.logit[slot0 + rank[j]] = glg[j];
      o.score[slot0 + rank[j]] = gsc[j];
    }
  for (int s = count + lane; s < nbest; s += 64) {
    out_len[slot0 + s] = overflow ? -1 : 0;
    o.logit[slot0 + s] = -INFINITY;
    o.score[slot0 + s] = -INFINITY;
  }
  if (lane == 0) o.count[b] = count;
  wave_sync();

  // ---- trace back, as final_pass does, lane l for slots l and l + 64 ----
  const bool two = count > 64;                               // (uniform)
  int cur_b[2], n[2] = {0, 0};
  bool act[2], lead[2] = {true, true};
  int32_t* out[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int s = lane + 64 * j;
    act[j] = s < count;
    cur_b[j] = act[j] ? mark[kMaxBeams + s] : 0;
    out[j] = out_ids + (slot0 + (act[j] ? s : 0)) * frames_ld;
  }
  unsigned int* rows = reinterpret_cast<unsigned int*>(S.tkey);            // [2][kTbRows][kMaxBeams]
  constexpr int kRowRegs = kTbRows * kMaxBeams / 4 / 64;
  uint4 rr[kRowRegs];
  const int nbatch = (frames + kTbRows - 1) / kTbRows;
  auto tb_request = [&](int j) __attribute__((always_inline)) {
    const int t_hi = frames - 1 - j * kTbRows, t_lo = max(0, t_hi - kTbRows + 1), nq = (t_hi - t_lo + 1) * (kMaxBeams / 4);
    const uint4* g = reinterpret_cast<const uint4*>(bp + (int64_t)t_lo * kMaxBeams);
#pragma unroll
    for (int k = 0; k < kRowRegs; ++k) rr[k] = 64 * k + lane < nq ? g[64 * k + lane] : make_uint4(0, 0, 0, 0);
  };
  auto tb_land = [&](int j) __attribute__((always_inline)) {
    uint4* dst = reinterpret_cast<uint4*>(rows + (j & 1) * kTbRows * kMaxBeams);
#pragma unroll
    for (int k = 0; k < kRowRegs; ++k) dst[64 * k + lane] = rr[k];
  };
  auto walk = [&](int j, unsigned int e) __attribute__((always_inline)) {
    const unsigned int ch = e & 255;
    if (ch) {
      const int id = (int)ch - 1;
      if (!(lead[j] && id == space_id)) {                   // normalise trailing whitespace
        lead[j] = false;
        out[j][frames_ld - 1 - n[j]] = id;                  // filled from the back, moved below
        ++n[j];
      }
    }
    cur_b[j] = (int)(e >> 8);
  };
  if (nbatch > 0) { tb_request(0); tb_land(0); }
  for (int j = 0; j < nbatch; ++j) {
    if (j + 1 < nbatch) tb_request(j + 1);
    wave_sync();
    const int t_hi = frames - 1 - j * kTbRows, t_lo = max(0, t_hi - kTbRows + 1);
    const unsigned int* rb = rows + (j & 1) * kTbRows * kMaxBeams;
    for (int tt = t_hi - t_lo; tt >= 0; --tt) {
      if (act[0]) walk(0, rb[tt * kMaxBeams + cur_b[0]]);
      if (two && act[1]) walk(1, rb[tt * kMaxBeams + cur_b[1]]);
    }
    if (j + 1 < nbatch) tb_land(j + 1);
    wave_sync();
  }
  // out[j][0 .. n) = out[j][frames_ld - n ..): a lane moves its own rows, 16 words at a time, every load of a chunk before
  // its stores (destination indices lie below the source indices: a chunk never overwrites what a later one reads)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!act[j]) continue;
    const int off = frames_ld - n[j];
    if (off > 0) {
      for (int c0 = 0; c0 < n[j]; c0 += 16) {
        int v[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) v[c] = c0 + c < n[j] ? out[j][off + c0 + c] : 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) if (c0 + c < n[j]) out[j][c0 + c] = v[c];
      }
    }
    out_len[slot0 + lane + 64 * j] = overflow ? -1 : n[j];
  }
}

}  // namespace beam_detail
}  // namespace vasr
