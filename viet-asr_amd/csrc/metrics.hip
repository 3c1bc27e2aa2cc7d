// Evaluation metrics on device id sequences.
//   error_counts : word_error_rate (nemo/collections/asr/metrics.py:30-63) with use_cer False AND True, per row:
//                  {word_edits, ref_words, char_edits, ref_chars} of one (hypothesis, reference) pair of label-id rows.
//
// One workgroup of 256 lanes per pair, everything in LDS, integer arithmetic only (no floating point: the Makefile's note on
// packed-FP32 next to MFMA kernels of another stream does not arise), one 16-byte vector store per row.
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

__global__ __launch_bounds__(kLanes) void error_counts_kernel(const int32_t* __restrict__ hyp, int wh,
                                                             const int32_t* __restrict__ hyp_len,
                                                             const int32_t* __restrict__ ref, int wr,
                                                             const int32_t* __restrict__ ref_len, SpaceIds sp,
                                                             int32_t* __restrict__ counts) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  int4* out = reinterpret_cast<int4*>(counts) + b;
  const int ln = hyp_len[b], lm = ref_len[b];
  if (ln < 0 || lm < 0) {          // the beam search's id_len = -1 overflow report: passed on, not turned into a number
    if (tid == 0) *out = make_int4(-1, -1, -1, -1);
    return;
  }
  const int n = ln < wh ? ln : wh, m = lm < wr ? lm : wr;
  const MetricsLds L = metrics_lds(wh, wr);
  unsigned long long* hash_h = reinterpret_cast<unsigned long long*>(lds_raw + L.hash_h);
  unsigned long long* hash_r = reinterpret_cast<unsigned long long*>(lds_raw + L.hash_r);
  int32_t* a = reinterpret_cast<int32_t*>(lds_raw + L.ids_h);
  int32_t* r = reinterpret_cast<int32_t*>(lds_raw + L.ids_r);
  int* d0 = reinterpret_cast<int*>(lds_raw + L.diag);
  int *d1 = d0 + L.diag_ld, *d2 = d1 + L.diag_ld;
  uint32_t* pos_h = reinterpret_cast<uint32_t*>(lds_raw + L.pos_h);
  uint32_t* pos_r = reinterpret_cast<uint32_t*>(lds_raw + L.pos_r);
  int* nwords = reinterpret_cast<int*>(lds_raw + L.bytes - 16);

  const int32_t* gh = hyp + b * wh;
  const int32_t* gr = ref + b * wr;
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

  const int char_edits = edit_distance(n, m, d0, d1, d2, [&](int i, int j) { return a[i] == r[j]; });
  const int word_edits = edit_distance(nw, mw, d0, d1, d2, [&](int i, int j) {
    if (hash_h[i] != hash_r[j]) return false;
    const uint32_t ph = pos_h[i], pr = pos_r[j];
    const int len = (int)(ph >> 16);
    if (len != (int)(pr >> 16)) return false;
    const int32_t* x = a + (ph & 0xffffu);
    const int32_t* y = r + (pr & 0xffffu);
    for (int k = 0; k < len; ++k)
      if (x[k] != y[k]) return false;
    return true;
  });
  if (tid == 0) *out = make_int4(word_edits, mw, char_edits, m);
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

}  // namespace vasr
