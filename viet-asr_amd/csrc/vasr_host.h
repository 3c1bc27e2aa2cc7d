// Host-side helpers vasr_api.cpp shares with vasr_devtools.cpp (the kernels' launch interface is vasr_internal.h).
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

}  // namespace vasr
