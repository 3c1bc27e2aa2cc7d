// Pointwise (1x1) convolution as an fp32 MFMA GEMM with the BatchNorm / residual / ReLU epilogue,
// for gfx950.
//
// Replaces, per JasperBlock sub-block (reference nemo/collections/asr/parts/jasper.py):
//   MaskedConv1d(Cin, Cout, 1) (:113-132, :374-384)  ->  BatchNorm1d(eps=1e-3) eval (:392)
//   [-> + residual branch output (:438-439)]  ->  ReLU (:405 / mout :444)
// and the CTC head's Conv1d(1024, V+1, 1, bias=True) (jasper.py:249).
//
//   Y[b][m][t] = act( scale[m] * sum_k W[m][k] * Xm[b][k][t] + shift[m] (+ R[b][m][t]) )
//
// Exact-fp32 arithmetic on the matrix cores: v_mfma_f32_32x32x2_f32 accumulates as a k-ordered
// fmaf chain (gfx950 has no TF32/xf32), which keeps greedy argmax parity with the fp32 reference.
//
// Structure ("weights stream, activations stay"):
//   * 8 wavefronts per workgroup, each owning a 64(M) x 64(T) output block = 2x2 MFMA tiles
//     (64 accumulator VGPRs).  Wave grid WM x WN = 8x1 / 4x2 / 2x4 so one workgroup covers
//     512x64, 256x128 or 128x256 outputs: for the 256- and 512-channel layers ONE workgroup
//     computes every output channel of its time tile, so each activation element is fetched
//     from HBM exactly once per layer.
//   * The activation (B) operand goes through LDS in 32 KB K-chunks, double buffered: one
//     barrier per chunk (64..256 MFMAs per wave between barriers).
//   * The weight (A) operand never touches LDS: weights are pre-packed at vasr_finalize() in MFMA
//     fragment order ([m-tile][k-group][lane][4]) so that every lane fetches its operands for four
//     k-steps with one coalesced 16-byte load straight from L2, one k-group ahead of use.
//   * Work-group ids are remapped so that neighbours in (m-block, time-tile) order share an XCD
//     (private L2 per XCD; block b lands on XCD b % 8).
//   * CONV (PwArgs::conv_cin > 0): a non-separable K-tap MaskedConv1d as an implicit GEMM over the reduction index
//     k = tap * C_in + c (encoder_pw_split.hip has the same form): row k of a chunk is x[c] read at column
//     t * stride + tap * dil - pad, zero outside [0, lens[b]).
#include <cstdlib>

#include "vasr_internal.h"
#include "vasr_device.h"

namespace vasr {

namespace {

constexpr int kChunkFloats = 8192;  // 32 KB of activations per LDS buffer

// WM x WN wave grid, each wave TM (1 or 2) m-tiles of 32 rows by 2 n-tiles of 32 columns
template <int WM, int TM>
struct PwGeom {
  static constexpr int WN = 8 / WM;
  static constexpr int BM = 32 * TM * WM;
  static constexpr int BN = 64 * WN;
  static constexpr int BKC = kChunkFloats / BN;  // 128 / 64 / 32 rows of K per chunk
  static constexpr int GROUPS = BKC / 8;         // k-groups (8 k = 4 MFMA k-steps) per chunk
  static constexpr int ROWS_PER_PASS = 512 / (BN / 4);
  static constexpr int PASSES = BKC / ROWS_PER_PASS;  // == 4 dwordx4 per thread per chunk
};

// DUAL: the reduction runs over two activation tensors back to back -- rows [0, K1) from a.x, rows [K1, K)
// from a.x2 (masked with a.lens2).  Used to fold a JasperBlock's residual 1x1 conv into its last sub-block's GEMM
// (weights [s1*W1 | s2*W2] concatenated along K, shift h1 + h2), which removes the residual tensor round trip.
// EPI: epilogue_kind (vasr_internal.h), the shared Epilogue<EPI> of vasr_device.h
template <int WM, int TM, bool MASK, bool RES, bool DUAL, bool CONV = false, int EPI = 0>
__global__ __launch_bounds__(512, 4) void pw_gemm_kernel(PwArgs a, int blocks_m, int tiles_t, int n_blocks) {
  using G = PwGeom<WM, TM>;
  __shared__ v4f Bs4[2][kChunkFloats / 4];

  const int bid = xcd_remap(blockIdx.x, n_blocks);
  const int mb = bid % blocks_m;
  const int nt = bid / blocks_m;
  const int b = nt / tiles_t;
  const int t0 = (nt % tiles_t) * G::BN;
  const int m0 = mb * G::BM;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = (wave / G::WN) * 32 * TM, wn = (wave % G::WN) * 64;
  const int kh = lane >> 5, l31 = lane & 31;
  const int len = MASK ? a.lens[b] : 0;
  const int len2 = DUAL ? a.lens2[b] : 0;

  // B staging: thread -> (row, 4 consecutive columns) of the [BKC][BN] chunk
  constexpr int C4 = G::BN / 4;
  const int ld_row = tid / C4, ld_c4 = tid % C4;
  const int K1 = DUAL ? a.K1 : a.K;
  const float* __restrict__ xb = CONV ? a.x + (int64_t)b * a.conv_cin * a.ldx
                                     : a.x + (a.bsx ? (int64_t)b * a.bsx : (int64_t)b * K1 * a.ldx) + t0 + ld_c4 * 4;
  const float* __restrict__ xb2 = DUAL ? a.x2 + (int64_t)b * (a.K - K1) * a.ldx2 + t0 + ld_c4 * 4 : nullptr;
  // A fragments: packed [M/32][K/8][64 lanes] float4, this wave's TM m-tiles
  const int kgroups = a.K / 8;
  const v4f* __restrict__ ap0 = reinterpret_cast<const v4f*>(a.wt) + ((int64_t)((m0 + wm) / 32) * kgroups) * 64 + lane;
  const v4f* __restrict__ ap1 = ap0 + (TM > 1 ? (int64_t)kgroups * 64 : 0);

  f32x16 acc[TM][2];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  v4f rb[G::PASSES];
  auto gload = [&](int k0) {
    if constexpr (CONV) {
#pragma unroll
      for (int p = 0; p < G::PASSES; ++p) {
        const int k = k0 + ld_row + G::ROWS_PER_PASS * p, tap = k / a.conv_cin, c = k - tap * a.conv_cin;
        const float* __restrict__ row = xb + (int64_t)c * a.ldx;
        v4f v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = (t0 + ld_c4 * 4 + e) * a.conv_stride + tap * a.conv_dil - a.conv_pad;
          const bool ok = col >= 0 && col < len;
          const float x = row[ok ? col : 0];
          v[e] = ok ? x : 0.f;
        }
        rb[p] = v;
      }
      return;
    }
    const bool second = DUAL && k0 >= K1;      // chunk-uniform: K1 is a multiple of the chunk depth
    const float* __restrict__ src = second ? xb2 + (int64_t)(k0 - K1) * a.ldx2 : xb + (int64_t)k0 * a.ldx;
    const int64_t ld = second ? a.ldx2 : a.ldx;
    const bool mask = second || MASK;
    const int ml = second ? len2 : len;
#pragma unroll
    for (int p = 0; p < G::PASSES; ++p) {
      const int kr = ld_row + G::ROWS_PER_PASS * p;
      v4f v = *reinterpret_cast<const v4f*>(src + (int64_t)kr * ld);
      if (mask) {  // MaskedConv1d: x.masked_fill(t >= lens, 0)  (jasper.py:113-118)
        const int t = t0 + ld_c4 * 4;
        if (t + 0 >= ml) v.x = 0.f;
        if (t + 1 >= ml) v.y = 0.f;
        if (t + 2 >= ml) v.z = 0.f;
        if (t + 3 >= ml) v.w = 0.f;
      }
      rb[p] = v;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int p = 0; p < G::PASSES; ++p) Bs4[buf][(ld_row + G::ROWS_PER_PASS * p) * C4 + ld_c4] = rb[p];
  };

  const int nchunks = a.K / G::BKC;
  gload(0);
  v4f a0 = ap0[0], a1 = ap1[0];
  sstore(0);
  __syncthreads();

  for (int c = 0; c < nchunks; ++c) {
    if (c + 1 < nchunks) gload((c + 1) * G::BKC);
    const float* __restrict__ Bs = reinterpret_cast<const float*>(Bs4[c & 1]) + wn + l31;
#pragma unroll
    for (int g = 0; g < G::GROUPS; ++g) {
      // fetch next k-group's weights (clamped at the very end: a harmless re-read)
      const int gi = c * G::GROUPS + g;
      const int gn = gi + 1 < kgroups ? gi + 1 : gi;
      const v4f n0 = ap0[(int64_t)gn * 64], n1 = ap1[(int64_t)gn * 64];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int kk = g * 8 + 2 * s + kh;
        const float b0 = Bs[kk * G::BN];
        const float b1 = Bs[kk * G::BN + 32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b1, acc[0][1], 0, 0, 0);
        if constexpr (TM > 1) {
          acc[TM - 1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b0, acc[TM - 1][0], 0, 0, 0);
          acc[TM - 1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b1, acc[TM - 1][1], 0, 0, 0);
        }
      }
      a0 = n0;
      a1 = n1;
    }
    if (c + 1 < nchunks) {
      sstore((c + 1) & 1);
      __syncthreads();
    }
  }

  // ---- epilogue: BN affine (+ residual) + activation; each half-wave writes 128-byte row segments ----
  // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
  if (a.relu & 2) return;  // debug: skip the epilogue (tools/bench_layers.py ablation)
  const bool full = (t0 + G::BN <= a.store_cols) && (m0 + G::BM <= a.m_store);
  const Epilogue<EPI> epi(a.relu, a.act, a.res_max);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int mq = m0 + wm + i * 32 + 8 * q + 4 * kh;
      const v4f sc = *reinterpret_cast<const v4f*>(a.scale + mq);
      const v4f sh = *reinterpret_cast<const v4f*>(a.shift + mq);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int m = mq + rr;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int t = t0 + wn + j * 32 + l31;
          // (res may be y: this thread reads the element before it stores it)
          const float v = epi.template apply<RES>(fmaf(acc[i][j][4 * q + rr], sc[rr], sh[rr]), a.res + ((int64_t)b * a.M + m) * a.ldr + t);
          if (full || (t < a.store_cols && m < a.m_store)) a.y[((int64_t)b * a.m_store + m) * a.ldy + t] = v;
        }
      }
    }
  }
}

template <int WM, int TM, int EPI>
void launch_g(const PwArgs& a, hipStream_t st) {
  using G = PwGeom<WM, TM>;
  const int blocks_m = a.M / G::BM;
  const int tiles_t = (int)(((a.conv_cin ? a.conv_cols : a.ldx) + G::BN - 1) / G::BN);
  const int n_blocks = blocks_m * tiles_t * a.batch;
  dim3 grid(n_blocks), block(512);
  const bool mask = a.lens != nullptr, res = a.res != nullptr, dual = a.x2 != nullptr;
  if (a.conv_cin && res) VASR_LAUNCH((pw_gemm_kernel<WM, TM, true, true, false, true, EPI>), grid, block, 0, st, a, blocks_m, tiles_t, n_blocks);
  else if (a.conv_cin) VASR_LAUNCH((pw_gemm_kernel<WM, TM, true, false, false, true, EPI>), grid, block, 0, st, a, blocks_m, tiles_t, n_blocks);
  else if (dual) VASR_LAUNCH((pw_gemm_kernel<WM, TM, false, false, true, false, EPI>), grid, block, 0, st, a, blocks_m, tiles_t, n_blocks);
  else if (mask && res) VASR_LAUNCH((pw_gemm_kernel<WM, TM, true, true, false, false, EPI>), grid, block, 0, st, a, blocks_m, tiles_t, n_blocks);
  else if (mask) VASR_LAUNCH((pw_gemm_kernel<WM, TM, true, false, false, false, EPI>), grid, block, 0, st, a, blocks_m, tiles_t, n_blocks);
  else if (res) VASR_LAUNCH((pw_gemm_kernel<WM, TM, false, true, false, false, EPI>), grid, block, 0, st, a, blocks_m, tiles_t, n_blocks);
  else VASR_LAUNCH((pw_gemm_kernel<WM, TM, false, false, false, false, EPI>), grid, block, 0, st, a, blocks_m, tiles_t, n_blocks);
}

template <int WM, int TM>
void launch_t(const PwArgs& a, hipStream_t st) {
  // every activation but ReLU and a max residual take epilogue 1 or 2; the ReLU / add kernels stay as they were
  switch (epilogue_kind(a.relu, a.act, a.res && a.res_max)) {
    case 2: launch_g<WM, TM, 2>(a, st); break;
    case 1: launch_g<WM, TM, 1>(a, st); break;
    default: launch_g<WM, TM, 0>(a, st);
  }
}

}  // namespace

void launch_pointwise(const PwArgs& a, hipStream_t st) {
  // M % 128 == 0 and K % 64 == 0 are guaranteed by vasr_finalize() (and checked by vasr_bench_pointwise), ldx % 128 == 0
  // by pad_frames().  The 128 x 256 tile (K % 32 shapes) assumes a 256-frame pitch, which pad_frames() stopped giving in
  // round 2: it only runs when the pitch allows it, and no caller can reach it with K % 64 != 0 any more.
  // Tile choice: cover all of M with one workgroup where possible (each activation fetched once), and keep
  // >= 2 workgroups per CU in flight: 512 ch -> 512x64 tiles, 256 ch -> 256x64 (one m-tile per wave), else 128x128.
  const int kq = a.x2 ? a.K1 : a.K;   // dual source: both parts must be whole chunks of the K depth per LDS buffer
  const bool k128 = a.K % 128 == 0 && kq % 128 == 0, k64 = a.K % 64 == 0 && kq % 64 == 0;
  if (a.M % 512 == 0 && k128) launch_t<8, 2>(a, st);
  else if (a.M % 256 == 0 && k128) launch_t<8, 1>(a, st);
  else if (a.M % 256 == 0 && k64) launch_t<4, 2>(a, st);
  else if (k64) launch_t<4, 1>(a, st);
  else launch_t<2, 2>(a, st);   // K % 32 shapes on a 256-frame pitch only (unreachable through the C ABI today)
}

// [cout][cin] row-major -> MFMA A-fragment order [m_pad/32][cin/8][64 lanes][4]:
//   lane (l31, kh), element s  <-  W[mt*32 + l31][g*8 + 2*s + kh]
void pack_pointwise_weights(const float* w, int cout, int cin, int m_pad, float* out) {
  const int kgroups = cin / 8;
  for (int mt = 0; mt < m_pad / 32; ++mt)
    for (int g = 0; g < kgroups; ++g)
      for (int lane = 0; lane < 64; ++lane)
        for (int s = 0; s < 4; ++s) {
          const int m = mt * 32 + (lane & 31), k = g * 8 + 2 * s + (lane >> 5);
          out[(((size_t)mt * kgroups + g) * 64 + lane) * 4 + s] = m < cout ? w[(size_t)m * cin + k] : 0.f;
        }
}

// [cout][cin][kernel] (Conv1d weight) -> [cout][kernel * cin], reduction index k = tap * cin + c (c_in inner)
void pack_conv_gemm_weights(const float* w, int cout, int cin, int kernel, float* out) {
  for (int m = 0; m < cout; ++m)
    for (int t = 0; t < kernel; ++t)
      for (int c = 0; c < cin; ++c) out[((size_t)m * kernel + t) * cin + c] = w[((size_t)m * cin + c) * kernel + t];
}

}  // namespace vasr
