// Evaluation metrics on device id sequences.
//   error_counts : word_error_rate (nemo/collections/asr/metrics.py:30-63) with use_cer False AND True, per row:
//                  {word_edits, ref_words, char_edits, ref_chars} of one (hypothesis, reference) pair of label-id rows.
//   error_ops    : the same two tables with one predecessor per cell (the alignment rule of include/vasr.h): substitutions,
//                  deletions, insertions and hits at both levels, and on request the word-level edit script.
//   nbest counts : error_counts of every slot of the beam search's n-best list against the row's one reference, then the two
//                  minima per row (the oracle error counts) and their slots.
//
// One workgroup of 256 lanes per pair, everything in LDS, integer arithmetic only (no floating point: the Makefile's note on
// packed-FP32 next to MFMA kernels of another stream does not arise), 16-byte vector stores of the counts.
//   1. both rows are staged in LDS over their OWN lengths (ids behind a length are never read);
//   2. word starts (a non-whitespace id at position 0 or after a whitespace id -- str.split() on ids) are compacted with
//      ballot + popcount, one wavefront per side, as ctc_collapse_kernel does for frames; every word then gets its length and
//      the 64-bit fold of its ids (beam_detail::hmix, beam_common.h);
//   3. the same Levenshtein routine (unit costs, metrics.py:7-27) runs twice: over the ids, and over the words.  It walks the
//      anti-diagonals d = i + j of the (n + 1) x (m + 1) table with three rolling diagonals indexed by i and one barrier per
//      diagonal: cell (i, j) reads (i - 1, j) and (i, j - 1) from diagonal d - 1 and (i - 1, j - 1) from d - 2, and the buffer
//      written for d is the one d - 3 used, which nobody reads any more.
// Two words are equal iff their id runs are equal: the fold and the length only prefilter, equal folds are confirmed id by id.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "beam_common.h"
#include "vasr_internal.h"

namespace vasr {
namespace {

constexpr int kLanes = 256;

__device__ __forceinline__ bool is_space(const SpaceIds& sp, int32_t id) {
  bool s = false;
  for (int k = 0; k < sp.n; ++k) s |= id == sp.id[k];
  return s;
}

// LDS carve-up for row widths (wh, wr); the host sizes the launch with the same function
struct MetricsLds {
  int words_h, words_r;            // capacity: a word needs a separator, so (w + 1) / 2 at most
  size_t hash_h, hash_r, ids_h, ids_r, diag, pos_h, pos_r, bytes;
  int diag_ld;
};
__host__ __device__ inline MetricsLds metrics_lds(int wh, int wr) {
  MetricsLds l;
  l.words_h = (wh + 1) / 2;
  l.words_r = (wr + 1) / 2;
  l.diag_ld = wh + 1;
  size_t o = 0;
  l.hash_h = o; o += (size_t)l.words_h * 8;
  l.hash_r = o; o += (size_t)l.words_r * 8;
  l.ids_h = o; o += (size_t)wh * 4;
  l.ids_r = o; o += (size_t)wr * 4;
  l.diag = o; o += (size_t)3 * l.diag_ld * 4;
  l.pos_h = o; o += (size_t)l.words_h * 4;
  l.pos_r = o; o += (size_t)l.words_r * 4;
  l.bytes = o + 16;                // + the two word counts
  return l;
}

// D[n][m] of the unit-cost edit distance between sequences of n and m elements; eq(i, j): element i of the first equals
// element j of the second.  All 256 lanes call it and all get the result.  d0..d2: n + 1 ints each.
template <class Eq>
__device__ int edit_distance(int n, int m, int* d0, int* d1, int* d2, Eq eq) {
  if (n == 0) return m;
  if (m == 0) return n;
  const int tid = threadIdx.x;
  int *p2 = d0, *p1 = d1, *cur = d2;
  if (tid == 0) { p2[0] = 0; p1[0] = 1; p1[1] = 1; }   // diagonals 0 and 1
  __syncthreads();
  for (int d = 2; d <= n + m; ++d) {
    const int lo = d > m ? d - m : 0, hi = d < n ? d : n;
    for (int i = lo + tid; i <= hi; i += kLanes) {
      const int j = d - i;
      int v;
      if (i == 0) v = j;
      else if (j == 0) v = i;
      else {
        const int change = p2[i - 1] + (eq(i - 1, j - 1) ? 0 : 1);
        const int up = p1[i - 1] + 1, left = p1[i] + 1;
        v = min(change, min(up, left));
      }
      cur[i] = v;
    }
    __syncthreads();
    int* t = p2; p2 = p1; p1 = cur; cur = t;
  }
  const int r = p1[n];
  __syncthreads();                 // the buffers are free for the next call only after everybody has read the result
  return r;
}

// word starts of x[0, n) -> pos[w] = start (compacted, in order); returns the count.  One wavefront.
__device__ int find_words(const int32_t* x, int n, const SpaceIds& sp, uint32_t* pos, int lane) {
  int count = 0;
  for (int t0 = 0; t0 < n; t0 += 64) {
    const int t = t0 + lane;
    bool start = false;
    if (t < n) start = !is_space(sp, x[t]) && (t == 0 || is_space(sp, x[t - 1]));
    const unsigned long long mask = __ballot(start);
    if (start) pos[count + __popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)t;
    count += __popcll(mask);
  }
  return count;
}

// pos[w] = start | length << 16 (start < 4096, length <= 4096), hash[w] = the fold of the word's ids
__device__ void measure_words(const int32_t* x, int n, const SpaceIds& sp, uint32_t* pos, unsigned long long* hash, int words) {
  for (int w = threadIdx.x; w < words; w += kLanes) {
    const int s = (int)pos[w];
    unsigned long long h = beam_detail::kFnvOffset;
    int t = s;
    for (; t < n && !is_space(sp, x[t]); ++t) h = beam_detail::hmix(h, (unsigned long long)(uint32_t)x[t]);
    pos[w] = (uint32_t)s | ((uint32_t)(t - s) << 16);
    hash[w] = h;
  }
}

// One staged pair: both id rows in LDS over their own lengths, their words found, measured and folded.  All 256 lanes call
// stage_pair with the same arguments and leave it behind a barrier; the char-level and word-level routines below read it.
struct StagedPair {
  int n, m, nw, mw;                // ids and words per side
  const int32_t *a, *r;            // the staged ids
  const unsigned long long *hash_h, *hash_r;
  const uint32_t *pos_h, *pos_r;
  int *d0, *d1, *d2;               // the three rolling diagonals, wh + 1 ints each

  __device__ __forceinline__ bool ids_equal(int i, int j) const { return a[i] == r[j]; }
  // two words are equal iff their id runs are equal: fold and length prefilter, equal folds are confirmed id by id
  __device__ __forceinline__ bool words_equal(int i, int j) const {
    if (hash_h[i] != hash_r[j]) return false;
    const uint32_t ph = pos_h[i], pr = pos_r[j];
    const int len = (int)(ph >> 16);
    if (len != (int)(pr >> 16)) return false;
    const int32_t* x = a + (ph & 0xffffu);
    const int32_t* y = r + (pr & 0xffffu);
    for (int k = 0; k < len; ++k)
      if (x[k] != y[k]) return false;
    return true;
  }
};

// gh[0, n) and gr[0, m) (n <= wh, m <= wr, both >= 0) -> LDS carved by metrics_lds(wh, wr)
__device__ __forceinline__ StagedPair stage_pair(unsigned char* lds_raw, const int32_t* gh, int n, int wh, const int32_t* gr,
                                                 int m, int wr, const SpaceIds& sp) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const MetricsLds L = metrics_lds(wh, wr);
  unsigned long long* hash_h = reinterpret_cast<unsigned long long*>(lds_raw + L.hash_h);
  unsigned long long* hash_r = reinterpret_cast<unsigned long long*>(lds_raw + L.hash_r);
  int32_t* a = reinterpret_cast<int32_t*>(lds_raw + L.ids_h);
  int32_t* r = reinterpret_cast<int32_t*>(lds_raw + L.ids_r);
  int* d0 = reinterpret_cast<int*>(lds_raw + L.diag);
  uint32_t* pos_h = reinterpret_cast<uint32_t*>(lds_raw + L.pos_h);
  uint32_t* pos_r = reinterpret_cast<uint32_t*>(lds_raw + L.pos_r);
  int* nwords = reinterpret_cast<int*>(lds_raw + L.bytes - 16);

  for (int t = tid; t < n; t += kLanes) a[t] = gh[t];
  for (int t = tid; t < m; t += kLanes) r[t] = gr[t];
  __syncthreads();
  if (wave == 0) {
    const int c = find_words(a, n, sp, pos_h, lane);
    if (lane == 0) nwords[0] = c;
  } else if (wave == 1) {
    const int c = find_words(r, m, sp, pos_r, lane);
    if (lane == 0) nwords[1] = c;
  }
  __syncthreads();
  const int nw = nwords[0], mw = nwords[1];
  measure_words(a, n, sp, pos_h, hash_h, nw);
  measure_words(r, m, sp, pos_r, hash_r, mw);
  __syncthreads();
  return StagedPair{n, m, nw, mw, a, r, hash_h, hash_r, pos_h, pos_r, d0, d0 + L.diag_ld, d0 + 2 * L.diag_ld};
}

// {word_edits, ref_words, char_edits, ref_chars} of one pair; all lanes get the result
__device__ __forceinline__ int4 score_pair(unsigned char* lds_raw, const int32_t* gh, int n, int wh, const int32_t* gr, int m,
                                           int wr, const SpaceIds& sp) {
  const StagedPair P = stage_pair(lds_raw, gh, n, wh, gr, m, wr, sp);
  const int char_edits = edit_distance(P.n, P.m, P.d0, P.d1, P.d2, [&](int i, int j) { return P.ids_equal(i, j); });
  const int word_edits = edit_distance(P.nw, P.mw, P.d0, P.d1, P.d2, [&](int i, int j) { return P.words_equal(i, j); });
  return make_int4(word_edits, P.mw, char_edits, P.m);
}

__global__ __launch_bounds__(kLanes) void error_counts_kernel(const int32_t* __restrict__ hyp, int wh,
                                                             const int32_t* __restrict__ hyp_len,
                                                             const int32_t* __restrict__ ref, int wr,
                                                             const int32_t* __restrict__ ref_len, SpaceIds sp,
                                                             int32_t* __restrict__ counts) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  int4* out = reinterpret_cast<int4*>(counts) + b;
  const int ln = hyp_len[b], lm = ref_len[b];
  if (ln < 0 || lm < 0) {          // the beam search's id_len = -1 overflow report: passed on, not turned into a number
    if (tid == 0) *out = make_int4(-1, -1, -1, -1);
    return;
  }
  const int n = ln < wh ? ln : wh, m = lm < wr ? lm : wr;
  const int4 c = score_pair(lds_raw, hyp + b * wh, n, wh, ref + b * wr, m, wr, sp);
  if (tid == 0) *out = c;
}

// ---- the alignment rule of include/vasr.h: the same table with ONE predecessor per cell --------------------------------
// A diagonal entry is cost << 16 | substitutions along the cell's path (both <= 8192).  Along any path into (i, j)
// deletions - insertions = j - i, so the two numbers give all four counts at (n, m).
constexpr int kOpHit = 0, kOpSub = 1, kOpDel = 2, kOpIns = 3;

// The 2-bit predecessor codes of the word table, row i at words [i * ld, (i + 1) * ld), 16 cells per word.  The cells of one
// anti-diagonal lie in different rows, hence in different words, and diagonals are separated by a barrier: plain
// read-modify-write, no atomics.  ld is odd (consecutive rows fall into consecutive banks).  Zeroed before the walk.
struct OpBits {
  uint32_t* w;
  int ld;
  __device__ __forceinline__ void put(int i, int j, int code) const { w[i * ld + (j >> 4)] |= (uint32_t)code << ((j & 15) * 2); }
  __device__ __forceinline__ int get(int i, int j) const { return (int)(w[i * ld + (j >> 4)] >> ((j & 15) * 2)) & 3; }
};
struct NoBits {
  __device__ __forceinline__ void put(int, int, int) const {}
};
__host__ __device__ inline int op_bits_ld(int wr) { return (((wr + 1) / 2 + 16) / 16) | 1; }
__host__ __device__ inline size_t op_bits_bytes(int wh, int wr) { return (size_t)((wh + 1) / 2 + 1) * op_bits_ld(wr) * 4; }

// cost << 16 | substitutions of the alignment of n against m elements; the walk and the barriers of edit_distance
template <class Eq, class Bits>
__device__ int edit_ops(int n, int m, int* d0, int* d1, int* d2, Eq eq, Bits bits) {
  if (n == 0 || m == 0) return (n + m) << 16;             // all insertions, or all deletions
  const int tid = threadIdx.x;
  int *p2 = d0, *p1 = d1, *cur = d2;
  if (tid == 0) { p2[0] = 0; p1[0] = 1 << 16; p1[1] = 1 << 16; }
  __syncthreads();
  for (int d = 2; d <= n + m; ++d) {
    const int lo = d > m ? d - m : 0, hi = d < n ? d : n;
    for (int i = lo + tid; i <= hi; i += kLanes) {
      const int j = d - i;
      int v;
      if (i == 0) v = j << 16;
      else if (j == 0) v = i << 16;
      else {
        const int ne = eq(i - 1, j - 1) ? 0 : 1;
        const int diag = p2[i - 1] + ne * 0x10001, dele = p1[i] + 0x10000, ins = p1[i - 1] + 0x10000;
        const int cd = diag >> 16, cl = dele >> 16, ci = ins >> 16;
        int code;
        if (cd <= min(cl, ci)) { v = diag; code = ne ? kOpSub : kOpHit; }
        else if (cl <= ci) { v = dele; code = kOpDel; }
        else { v = ins; code = kOpIns; }
        bits.put(i, j, code);
      }
      cur[i] = v;
    }
    __syncthreads();
    int* t = p2; p2 = p1; p1 = cur; cur = t;
  }
  const int r = p1[n];
  __syncthreads();
  return r;
}

// packed result at (n, m) -> {sub, del, ins, hits}
__device__ __forceinline__ int4 split_ops(int packed, int n, int m) {
  const int cost = packed >> 16, s = packed & 0xffff;
  const int del = (cost - s + m - n) / 2;
  return make_int4(s, del, cost - s - del, m - s - del);
}

template <bool kScript>
__global__ __launch_bounds__(kLanes) void error_ops_kernel(const int32_t* __restrict__ hyp, int wh,
                                                          const int32_t* __restrict__ hyp_len,
                                                          const int32_t* __restrict__ ref, int wr,
                                                          const int32_t* __restrict__ ref_len, SpaceIds sp,
                                                          int32_t* __restrict__ ops, int32_t* __restrict__ script,
                                                          int32_t* __restrict__ script_len) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  int4* out = reinterpret_cast<int4*>(ops) + 2 * b;
  const int ln = hyp_len[b], lm = ref_len[b];
  if (ln < 0 || lm < 0) {
    if (tid == 0) {
      out[0] = make_int4(-1, -1, -1, -1);
      out[1] = make_int4(-1, -1, -1, -1);
      if (kScript) script_len[b] = -1;
    }
    return;
  }
  const int n = ln < wh ? ln : wh, m = lm < wr ? lm : wr;
  const StagedPair P = stage_pair(lds_raw, hyp + b * wh, n, wh, ref + b * wr, m, wr, sp);
  const int chars = edit_ops(P.n, P.m, P.d0, P.d1, P.d2, [&](int i, int j) { return P.ids_equal(i, j); }, NoBits{});
  int words;
  if (kScript) {
    const OpBits bits{reinterpret_cast<uint32_t*>(lds_raw + metrics_lds(wh, wr).bytes), op_bits_ld(wr)};
    if (P.nw > 0 && P.mw > 0) {    // the walk writes, and the trace-back reads, only then
      for (int k = tid; k < (P.nw + 1) * bits.ld; k += kLanes) bits.w[k] = 0;
      __syncthreads();
    }
    words = edit_ops(P.nw, P.mw, P.d0, P.d1, P.d2, [&](int i, int j) { return P.words_equal(i, j); }, bits);
    // Trace-back from (nw, mw): one lane, at most nw + mw steps, the codes last step first into the staged ids' place
    // (wh + wr ints, contiguous, no longer needed: a code says hit or substitution by itself), then all lanes turn them round.
    int32_t* rev = const_cast<int32_t*>(P.a);
    int* steps = reinterpret_cast<int*>(lds_raw + metrics_lds(wh, wr).bytes - 8);
    if (tid == 0) {
      int i = P.nw, j = P.mw, k = 0;
      while (i > 0 || j > 0) {
        const int code = i == 0 ? kOpDel : j == 0 ? kOpIns : bits.get(i, j);
        rev[k++] = code;
        if (code != kOpDel) --i;
        if (code != kOpIns) --j;
      }
      *steps = k;
      script_len[b] = k;
    }
    __syncthreads();
    const int len = *steps;
    int32_t* row = script + b * ((wh + 1) / 2 + (wr + 1) / 2);
    for (int k = tid; k < len; k += kLanes) row[k] = rev[len - 1 - k];
  } else {
    words = edit_ops(P.nw, P.mw, P.d0, P.d1, P.d2, [&](int i, int j) { return P.words_equal(i, j); }, NoBits{});
  }
  if (tid == 0) {
    out[0] = split_ops(words, P.nw, P.mw);
    out[1] = split_ops(chars, P.n, P.m);
  }
}

// ---- the n-best list against one reference per row -------------------------------------------------------------------
// workgroup (b, s): error_counts of slot s of row b against reference b; four -1 behind the count and in every slot of a row
// that cannot be scored
__global__ __launch_bounds__(kLanes) void nbest_counts_kernel(const int32_t* __restrict__ ids, int wh,
                                                             const int32_t* __restrict__ id_len,
                                                             const int32_t* __restrict__ count, int nbest,
                                                             const int32_t* __restrict__ ref, int wr,
                                                             const int32_t* __restrict__ ref_len, SpaceIds sp,
                                                             int32_t* __restrict__ slot_counts) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;    // grid (batch, nbest): no division, the file stays free of floating-point instructions
  const int s = blockIdx.y;
  const int64_t bs = b * nbest + s;
  int4* out = reinterpret_cast<int4*>(slot_counts) + bs;
  const int lm = ref_len[b];
  const int filled = count[b] < nbest ? count[b] : nbest;
  int bad = lm < 0 || filled < 1;
  for (int k = tid; k < filled; k += kLanes) bad |= id_len[b * nbest + k] < 0;
  bad = __syncthreads_or(bad);
  if (bad || s >= filled) {
    if (tid == 0) *out = make_int4(-1, -1, -1, -1);
    return;
  }
  const int ln = id_len[bs];
  const int n = ln < wh ? ln : wh, m = lm < wr ? lm : wr;
  const int4 c = score_pair(lds_raw, ids + bs * wh, n, wh, ref + b * wr, m, wr, sp);
  if (tid == 0) *out = c;
}

// one wavefront per row: the two minima over the filled slots, the lower slot among equals, in one fixed order
__global__ __launch_bounds__(64) void nbest_min_kernel(const int32_t* __restrict__ slot_counts,
                                                      const int32_t* __restrict__ count, int nbest,
                                                      int32_t* __restrict__ counts, int32_t* __restrict__ slot) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int4* in = reinterpret_cast<const int4*>(slot_counts) + b * nbest;
  const int4 first = in[0];
  if (first.x < 0) {               // slot 0 of a row that can be scored is filled: a -1 there is the row's report
    if (lane == 0) {
      if (counts) reinterpret_cast<int4*>(counts)[b] = make_int4(-1, -1, -1, -1);
      if (slot) { slot[2 * b] = -1; slot[2 * b + 1] = -1; }
    }
    return;
  }
  const int filled = count[b] < nbest ? count[b] : nbest;
  int wv = INT32_MAX, ws = INT32_MAX, cv = INT32_MAX, cs = INT32_MAX;
  for (int s = lane; s < filled; s += 64) {   // ascending slots per lane: strict < keeps the lower one
    const int4 c = in[s];
    if (c.x < wv) { wv = c.x; ws = s; }
    if (c.z < cv) { cv = c.z; cs = s; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int ov = __shfl_xor(wv, o), os = __shfl_xor(ws, o);
    if (ov < wv || (ov == wv && os < ws)) { wv = ov; ws = os; }
    const int pv = __shfl_xor(cv, o), ps = __shfl_xor(cs, o);
    if (pv < cv || (pv == cv && ps < cs)) { cv = pv; cs = ps; }
  }
  if (lane == 0) {
    if (counts) reinterpret_cast<int4*>(counts)[b] = make_int4(wv, first.y, cv, first.w);
    if (slot) { slot[2 * b] = ws; slot[2 * b + 1] = cs; }
  }
}

}  // namespace

int launch_error_counts(const int32_t* hyp, int hyp_width, const int32_t* hyp_len, const int32_t* ref, int ref_width,
                        const int32_t* ref_len, int batch, const SpaceIds& sp, int32_t* counts, hipStream_t st) {
  const MetricsLds L = metrics_lds(hyp_width, ref_width);
  if (L.bytes > 64 * 1024) {
    static std::atomic<uint64_t> lds_opted{0};   // per device (dyn_lds_opt_in); the largest carve-up is asked for once
    const hipError_t attr = dyn_lds_opt_in(reinterpret_cast<const void*>(error_counts_kernel),
                                           (int)metrics_lds(kMetricsMaxWidth, kMetricsMaxWidth).bytes, lds_opted);
    if (attr != hipSuccess) return (int)attr;
  }
  hipLaunchKernelGGL(error_counts_kernel, dim3(batch), dim3(kLanes), L.bytes, st, hyp, hyp_width, hyp_len, ref, ref_width,
                     ref_len, sp, counts);
  return 0;
}

int launch_error_ops(const int32_t* hyp, int hyp_width, const int32_t* hyp_len, const int32_t* ref, int ref_width,
                     const int32_t* ref_len, int batch, const SpaceIds& sp, int32_t* ops, int32_t* script, int32_t* script_len,
                     hipStream_t st) {
  const size_t counts_bytes = metrics_lds(hyp_width, ref_width).bytes;
  if (script) {
    const size_t bytes = counts_bytes + op_bits_bytes(hyp_width, ref_width);
    if (bytes > 64 * 1024) {
      static std::atomic<uint64_t> lds_opted{0};
      const int most = (int)(metrics_lds(kMetricsMaxScriptWidth, kMetricsMaxScriptWidth).bytes +
                             op_bits_bytes(kMetricsMaxScriptWidth, kMetricsMaxScriptWidth));
      const hipError_t attr = dyn_lds_opt_in(reinterpret_cast<const void*>(error_ops_kernel<true>), most, lds_opted);
      if (attr != hipSuccess) return (int)attr;
    }
    hipLaunchKernelGGL(error_ops_kernel<true>, dim3(batch), dim3(kLanes), bytes, st, hyp, hyp_width, hyp_len, ref, ref_width,
                       ref_len, sp, ops, script, script_len);
    return 0;
  }
  if (counts_bytes > 64 * 1024) {
    static std::atomic<uint64_t> lds_opted{0};
    const hipError_t attr = dyn_lds_opt_in(reinterpret_cast<const void*>(error_ops_kernel<false>),
                                           (int)metrics_lds(kMetricsMaxWidth, kMetricsMaxWidth).bytes, lds_opted);
    if (attr != hipSuccess) return (int)attr;
  }
  hipLaunchKernelGGL(error_ops_kernel<false>, dim3(batch), dim3(kLanes), counts_bytes, st, hyp, hyp_width, hyp_len, ref,
                     ref_width, ref_len, sp, ops, nullptr, nullptr);
  return 0;
}

int launch_nbest_error_counts(const int32_t* ids, int width, const int32_t* id_len, const int32_t* count, int nbest,
                              const int32_t* ref, int ref_width, const int32_t* ref_len, int batch, const SpaceIds& sp,
                              int32_t* slot_counts, int32_t* counts, int32_t* slot, hipStream_t st) {
  const MetricsLds L = metrics_lds(width, ref_width);
  if (L.bytes > 64 * 1024) {
    static std::atomic<uint64_t> lds_opted{0};
    const hipError_t attr = dyn_lds_opt_in(reinterpret_cast<const void*>(nbest_counts_kernel),
                                           (int)metrics_lds(kMetricsMaxWidth, kMetricsMaxWidth).bytes, lds_opted);
    if (attr != hipSuccess) return (int)attr;
  }
  hipLaunchKernelGGL(nbest_counts_kernel, dim3(batch, nbest), dim3(kLanes), L.bytes, st, ids, width, id_len, count,
                     nbest, ref, ref_width, ref_len, sp, slot_counts);
  if (counts || slot)
    hipLaunchKernelGGL(nbest_min_kernel, dim3(batch), dim3(64), 0, st, slot_counts, count, nbest, counts, slot);
  return 0;
}


}  // namespace vasr
