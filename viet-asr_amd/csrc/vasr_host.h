// Host-side helpers every host source shares (vasr_api.cpp, model_build.cpp, encoder_run.cpp, api_stages.cpp,
// vasr_devtools.cpp) that do not need the handle -- that is vasr_model.h; the kernels' launch interface is vasr_internal.h.
#pragma once
#include <vector>

#include "vasr.h"
#include "vasr_internal.h"

namespace vasr {

int fail(int code, const char* fmt, ...);   // sets vasr_last_error(); returns code
int check_launch(const char* what);         // hipGetLastError() after the launches of `what`

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fail(VASR_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// GroupNorm(G, c) tables of encoder_norm.hip (NormLaunch): gamma / beta and the group of every STORED channel, members = the
// stored channels of each group in pre-shuffle order; shuffle > 1: the channel shuffle of a grouped block stores pre-shuffle
// channel p = g * (c / shuffle) + j at j * shuffle + g (parts/jasper.py:135-150), 1: in place
struct NormTables {
  std::vector<float> gamma, beta;
  std::vector<int32_t> group_of, members;
};
NormTables norm_tables(const float* gamma, const float* beta, int c, int G, int shuffle);

// The PwArgs fields every GEMM site shares: weights [M][K] (wt in the fragment order of the kernel that runs), x [B][K][ld] ->
// y [B][M][ld] with `frames` valid columns, every row and column stored, no mask, no residual, no activation
inline PwArgs pw_args(const void* wt, const float* scale, const float* shift, int M, int K, const float* x, float* y,
                      int64_t ld, int64_t frames, int batch) {
  PwArgs a{};
  a.wt = static_cast<const float*>(wt); a.scale = scale; a.shift = shift; a.x = x; a.y = y;
  a.M = M; a.K = K; a.batch = batch; a.m_store = M;
  a.ldx = ld; a.ldy = ld; a.frames = (int)frames; a.store_cols = (int)ld;
  return a;
}

// ---- where run_encoder's tensors live ----
// Buffer numbers of one encoder pass, as run_encoder's checks and the plan getter (vasr_plan_buffers) name them: the four
// rotation buffers of the workspace plan (bufP, bufQ, bufR, bufS), the depthwise / residual scratch D, the dense-residual
// pane buffer, the encoder's input and its output; kBufNone: no such operand.
enum { kBufRot = 4, kBufD = 4, kBufPane = 5, kBufIn = 6, kBufOut = 7, kBufNone = -1 };
// Launch kinds of a plan record (kind, dst, src, src2, res).  SE, GroupNorm and a max-mode residual GEMM onto R work in place
// by design (dst == src, dst == res); every other kind's dst differs from all of its sources.
enum { kPlanPaneCopy = 0, kPlanDepthwise = 1, kPlanGemm = 2, kPlanFused = 3, kPlanResGemm = 4, kPlanSe = 5, kPlanNorm = 6 };

// Which rotation buffer the next sub-block output goes to.  A buffer is the live block input (the folded residual reads it
// until the block's last GEMM), the live residual result R of an unfused residual branch, the current tensor, or dead; the
// pane buffer and D are not rotation buffers and are never handed out.  Two forms:
//   pingpong: the block's outputs alternate between the first two buffers that are not the block input, in index order;
//   inplace:  a GEMM that reads D (the two-kernel separable path) stores over the current tensor, which the depthwise kernel
//             has just finished reading -- unless that is the block input; every other launch (a block's first sub-block, the
//             fused kernel, GEMMs that read the current tensor) takes the dead buffer touched most recently, lowest index
//             first among equals.  A block of sub-blocks that all take the two-kernel path then lives in its input, one
//             output buffer and D: every store lands on lines that were read or written one or two kernels earlier.
// R is the third buffer that is not the block input, in both forms.  pick() is pure; wrote() commits a launch.
struct BufRotation {
  enum Role { kDead = 0, kBlockIn, kRes, kCur };
  bool inplace = false;
  Role role[kBufRot] = {};
  int64_t touched[kBufRot] = {-1, -1, -1, -1};   // launch number of the last read or write
  int64_t tick = 0;
  int flip = 0, cur = kBufNone, blk_in = kBufNone, res = kBufNone;
  int pp[3] = {0, 1, 2};   // the buffers that are not the block input, in index order

  // blk: the block input's buffer (kBufNone: the encoder's own input); live_res: the block runs an unfused residual branch
  void begin_block(int blk, bool live_res) {
    int n = 0;
    for (int i = 0; i < kBufRot; ++i) {
      role[i] = i == blk ? kBlockIn : kDead;
      if (i != blk && n < 3) pp[n++] = i;
    }
    blk_in = cur = (blk >= 0 && blk < kBufRot) ? blk : kBufNone;
    res = live_res ? pp[2] : kBufNone;
    if (live_res) role[pp[2]] = kRes;
    flip = 0;
  }
  // over_cur: the launch does not read the current tensor (its GEMM reads D), so it may store over it
  int pick(bool over_cur) const {
    if (!inplace) return pp[flip];
    if (over_cur && cur >= 0 && role[cur] == kCur) return cur;
    int best = kBufNone;
    for (int i = 0; i < kBufRot; ++i)
      if (role[i] == kDead && (best < 0 || touched[i] > touched[best])) best = i;
    return best;
  }
  void touch(int b) { if (b >= 0 && b < kBufRot) touched[b] = tick; }
  // one launch: its operands count as touched now
  void launched(int dst, int x, int x2, int r) { ++tick; touch(dst); touch(x); touch(x2); touch(r); }
  // the launch that stored the sub-block's output into rotation buffer dst: it becomes the current tensor
  void wrote(int dst) {
    if (cur >= 0 && role[cur] == kCur) role[cur] = kDead;
    cur = dst >= 0 && dst < kBufRot ? dst : kBufNone;   // (the encoder output is no rotation buffer)
    if (cur >= 0) role[cur] = kCur;
    flip ^= 1;
  }
  // nullptr, or what is wrong with a launch of `kind` storing to dst: a destination that is one of the launch's own sources,
  // the live block input, the live R (but for the residual branch's own passes) or the pane buffer
  const char* refuse(int kind, int dst, int x, int x2, int r) const {
    const bool in_place = kind == kPlanSe || kind == kPlanNorm;
    if (dst == kBufNone) return "no destination";
    if (!in_place && (dst == x || dst == x2)) return "destination is a source of the launch";
    if (kind != kPlanResGemm && kind != kPlanNorm && dst == r) return "destination is the launch's residual operand";
    if (dst == kBufPane && kind != kPlanPaneCopy) return "destination is the pane buffer";
    if (dst == kBufIn) return "destination is the encoder input";
    if (dst >= 0 && dst < kBufRot) {
      if (role[dst] == kBlockIn) return "destination is the live block input";
      if (role[dst] == kRes && kind != kPlanResGemm && kind != kPlanSe && kind != kPlanNorm) return "destination is the live residual R";
    }
    return nullptr;
  }
};

}  // namespace vasr
