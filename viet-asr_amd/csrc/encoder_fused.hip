// Fused depthwise + pointwise sub-block of a 256-channel JasperBlock (gfx950): ONE kernel for
//
//     MaskedConv1d(C, C, K, groups = C)  ->  MaskedConv1d(C, C, 1)  ->  BatchNorm (eval)  [-> + BN(res 1x1 conv)]  ->  ReLU
//
// (reference nemo/collections/asr/parts/jasper.py:360-373 `_get_conv_bn_layer`, masks :108-132, block forward :408-448) --
// the "fused depthwise + pointwise + BN + ReLU + residual" kernel north_star names, for the shapes where it pays: the
// C = 256 blocks of QuartzNet (K = 33 / 39; 30 of the 75 separable sub-blocks of 15x5).  The depthwise output never goes
// to HBM: 33.5 MB written + 33.5 MB read again per sub-block at 64 x 10 s, one launch and its dispatch gap.
//
// Structure (numbers for the 128-frame tile; the 64-frame form of round 4 -- template parameter BN, FTile -- halves the
// columns of every role: 8 frames per producer lane, 2 x 2 MFMA tiles per consumer, 110 KB of LDS; it is the form for
// batches whose 128-frame tiles would leave the chip half empty, encoder_run.cpp run_encoder):
// a workgroup owns ALL 256 input and output channels of a 128-frame time tile and is split by ROLE
// (wave specialisation -- one kernel, two instruction streams, no compiler-interleaved software pipeline):
//
//   wavefronts 4..7  PRODUCERS, vector ALU.  Per 64-channel chunk each takes 16 channels = 8 channel pairs.  The masked
//     input window (128 + K - 1 frames, 16-byte aligned origin) of its 16 rows goes through a wavefront-private LDS
//     window with the two channels of a pair interleaved, so that every v_pk_fma_f32 computes the same (frame, tap) of
//     both channels; lane = (pair, 16 consecutive frames): a sliding register window, 16 x K packed FMAs, taps of the
//     pair from an LDS table as 64-bit operands.  The result is scaled by the utterance's power of two, split into fp16
//     hi / lo (encoder_pw_split.hip kF16x2) and written straight into the GEMM's B-fragment image in LDS.
//   wavefronts 0..3  CONSUMERS, matrix pipe.  64 output rows x 128 columns each (2 x 4 tiles of 32x32x16, 128
//     accumulators): per 16-deep k-step 4 weight fragments from L2 (the f16x2 pack of vasr_finalize, two k-steps ahead),
//     8 B fragments from LDS, 24 MFMAs.  No staging, no conversion, no address arithmetic in this stream.
//   One LDS-only barrier per chunk hands a finished B image over (double buffered): 4 barriers per tile (8 with a
//   residual source).  The residual branch of the block's last sub-block is a second K range [256, 512) as in the
//   unfused kernel (pack_fused_residual): its chunks are produced by plain conversion of the masked block input.
//
// The fp16 split needs the utterance's scale BEFORE the depthwise output exists, so it comes from a bound instead of
// the measured maximum: max |x| of the utterance (published by x's producer, AmaxTab) times the layer's largest
// sum_k |w[c][k]| (FusedArgs::dw_l1, a constant from vasr_finalize).  The bound is 2^2 .. 2^4 loose, i.e. the split
// carries 18-20 bits where the measured maximum would give 22: still below an fp32 dot product's own rounding
// (tools/split_scale_study.py; tests hold the fused path to the same tolerance as every other arithmetic).
//
// LDS (159 744 of 163 840 bytes, one workgroup per CU by design): B images 2 x 32 KB | producer windows 4 x 13 KB
// (reused by the epilogue's transposition: 4 x 8 KB; 16 wavefronts: 8 x 6.5 KB of windows, the epilogue's 8 x 8 KB in the
// windows AND B image 0) | tap table [128 pairs][K + 1][2] f32.
//
// The 16-wavefront form of the 128-frame tile (template parameter NW = 16, 1024 threads, 128 registers a wavefront): the same
// grid, LDS plan, barrier protocol and arithmetic with TWO wavefronts of each role per SIMD, so that one covers the other's
// LDS and L2 round trips.  Consumers 0..7 own 32 rows x 128 columns (1 x 4 tiles, 64 accumulators; every accumulator gets
// the products in the order it gets them on 8 wavefronts), producers 8..15 take 8 channels = 4 pairs of a chunk -- one k-half
// of one k-step -- with 16 lanes of 8 frames per pair (the 64-frame form's lane geometry) and tap blocks of 4.  The
// windows stay wavefront-private (8 x 4 pairs x 1664 bytes, the same 53 KB).  The epilogue's 8 x 8 KB of transposition
// space no longer fit the windows alone: consumers 0..3 use B image 0, which every consumer has left before the LAST
// chunk's barrier lets any of them finish (the last chunk is read from image 1), consumers 4..7 the windows.
#include <cstdlib>

#include "vasr_internal.h"
#include "vasr_device.h"
#include <type_traits>

namespace vasr {

namespace {

constexpr int FC = 256;     // channels in = out
constexpr int FCH = 64;     // channels per chunk (4 k-steps of 16)

// Tile width BN (columns = frames per workgroup): 128 where such tiles fill the chip, 64 for the batches in between (24-47
// utterances of 10 s: 192-376 tiles of 64 frames against 96-188 of 128).  Everything below that depends on it, and on the
// wavefront count NW: 8 (one consumer and one producer per SIMD) or, for the 128-frame tile, 16 (two of each per SIMD, each
// role's rows / channels split in two: the head comment's last paragraph):
template <int BN, int NW = 8>
struct FTile {
  static_assert(BN == 128 || BN == 64, "tile width");
  static_assert(NW == 8 || (NW == 16 && BN == 128), "wavefronts per workgroup");
  static constexpr int NTHR = NW * 64;
  static constexpr int NPW = NW / 2;                       // wavefronts per role: 4 / 8
  static constexpr int MT = 8 / NPW;                       // 32-row MFMA tiles of a consumer wavefront: 2 / 1
  static constexpr int SEG = NW;                           // segments (lanes) per channel pair: 8 / 16
  static constexpr int PP = 64 / SEG;                      // channel pairs per producer wavefront and chunk: 8 / 4
  static constexpr int FPS = BN / SEG;                     // frames per producer lane: 16 / 8 (BN = 64, and 128 on 16 wavefronts)
  static constexpr int NT = BN / 32;                       // 32-column MFMA tiles of a consumer wavefront: 4 / 2
  static constexpr int KHS = BN == 128 ? 3 : 2;            // bit of the k-half in the B image's column swizzle
  static constexpr int kBimgBytes = 2 * 2 * 4 * 2 * BN * 16;   // [buf][plane][k-step][k-half][column] x 16 B = 65536 / 32768
  static constexpr int kWPitch = BN == 128 ? 1664 : 1152;  // bytes per channel pair of a producer window (= 128 mod 256)
  static constexpr int kWWave = PP * kWPitch;              // 13312 / 9216 (16 wavefronts: 6656)
  static constexpr int kWinBytes = NPW * kWWave;           // 53248 / 36864
  static constexpr int kSegBytes = FPS * 8 + 16;           // a lane's segment of its pair's window row incl. its pad: 144 / 80
};

template <int K, int BN, int NW = 8>
struct FGeom {
  using TL = FTile<BN, NW>;
  static constexpr int FPS = TL::FPS;
  static constexpr int PAD = K / 2;                              // get_same_padding, stride 1, dilation 1 (jasper.py:60-65)
  static constexpr int PADL = (PAD + 3) & ~3;                    // window origin t0 - PADL: 16-byte aligned in x
  static constexpr int OFF = PADL - PAD;
  static constexpr int W = (PADL + BN + (K - 1 - PAD) + 3) & ~3;    // window frames: 160 (K = 33), 168 (K = 39); 96 / 104 at BN = 64
  static constexpr int W4 = W / 4;
  static constexpr int NLD = (TL::PP * W4 + 63) / 64;            // (pair, float4-column) items per lane: 5 / 6 (3 / 4; 16 wavefronts: 3 / 3)
  static constexpr int NF = OFF + FPS - 1 + K;                   // frames a lane reads from its region's start
  static constexpr int NR = (NF + 1) / 2;                        // ds_read_b128 per lane (two interleaved frames each)
  static constexpr int KP = (K + 2) & ~1;                        // taps per pair in the LDS table (zero padded, even)
  // taps per block of the sliding window.  16 wavefronts have 128 registers each: a block of 4 keeps FPS + 3 frames and 4 taps
  // live with the next block's 4 + 4 in flight (30 + 16 registers against 46 + 32 for blocks of 8)
  static constexpr int TB = NW == 16 ? 4 : 8;
  static constexpr int NB = (K + TB - 1) / TB;
  static constexpr int kTapBytes = (FC / 2) * KP * 8;
  static constexpr size_t LDS = (size_t)TL::kBimgBytes + TL::kWinBytes + kTapBytes;
  // (the last segment's pad is never touched: K = 39 on 16 wavefronts fills the 1664 bytes exactly)
  static_assert((W - 4) * 8 + ((W - 4) / FPS) * 16 + 32 <= TL::kWPitch, "window row does not fit its pitch");
  static_assert(FPS * (TL::SEG - 1) + 2 * NR <= W, "a lane's reads leave the window");
  static_assert(TL::kSegBytes * (TL::SEG - 1) + (NR - 1) * 16 + ((NR - 1) / (FPS / 2)) * 16 + 16 <= TL::kWPitch, "a lane's reads leave its row");
  static_assert(NLD >= FPS / 4, "the residual rows of a lane use the staging registers of the window items");
  static_assert(LDS <= 163840, "LDS budget");
  // last b128 unit (exclusive) a tap block needs: frames < OFF + min(K, TB (blk + 1)) + FPS - 1
  static constexpr int qend(int blk) {
    const int k1 = TB * (blk + 1) < K ? TB * (blk + 1) : K;
    return (OFF + k1 + FPS - 1 + 1) / 2;
  }
};

struct FusedArgs {
  const float* x;            // [B][256][ldx] depthwise input
  int64_t ldx;
  const int32_t* lens_in;    // depthwise input mask
  const int32_t* lens_out;   // depthwise output (= pointwise input) mask
  const float* taps;         // [128 pairs][KP][2] depthwise taps, channel pairs interleaved
  float dw_l1;               // max_c sum_k |w[c][k]|
  AmaxTab amax_x;
  const uint4* wt;           // f16x2 A-fragment pack [256/32][Ktot/16][2][64] uint4
  float w_inv_scale;
  const float* scale;        // [256] BN affine (1 / h1 + h2 when the residual is folded into the weights)
  const float* shift;
  float* y;                  // [B][256][ldy]
  int64_t ldy;
  int32_t frames;            // valid columns
  int32_t relu;              // apply the activation act (kAct*)
  int32_t act;
  AmaxTab amax_y;
  const int32_t* lens_y;
  // residual source (DUAL): K range [256, 512) = masked block input
  const float* x2;
  int64_t ldx2;
  const int32_t* lens2;
  AmaxTab amax_x2;
  int32_t batch;
};

// LDS-only workgroup barrier: __syncthreads() would also drain the vector-memory counter, i.e. make the producers wait
// for the rows they have just requested for the NEXT chunk
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// B image: element (plane, k-step ks, k-half kh, column n) is one 16-byte slot (8 consecutive channels of one frame).
// The column index is swizzled inside its aligned group of 16 -- low4 ^= (n >> 4) | (kh << KHS) -- so that the producers'
// 4-byte writes (8 lanes of one pair sit 16 (8) columns apart: the same bank(s) unswizzled) and the consumers' 16-byte
// reads are both conflict free.  (BN = 64: the 8 lanes of a pair give low4 ^ j = {0, 8, 1, 9, 2, 10, 3, 11}, the other
// k-half the same set ^ 4.)
template <int BN>
__device__ __forceinline__ int bimg_slot(int n, int kh) { return (n & ~15) | ((n & 15) ^ ((n >> 4) | (kh << FTile<BN>::KHS))); }
template <int BN>
__device__ __forceinline__ constexpr int bimg_off(int buf, int plane, int ks) { return (((buf * 2 + plane) * 4 + ks) * 2) * BN * 16; }

// EPI: epilogue_kind (vasr_internal.h), the float4 form of vasr_device.h's Epilogue<EPI> without a residual tensor
template <int K, bool DUAL, int BN, int EPI = 0, int NW = 8>
__global__ __launch_bounds__(NW * 64, 1) void dwpw_fused_kernel(FusedArgs a, int tiles_t, int n_blocks) {
  using G = FGeom<K, BN, NW>;
  using TL = FTile<BN, NW>;
  constexpr int FPS = TL::FPS, NT = TL::NT, kWPitch = TL::kWPitch, kWWave = TL::kWWave;
  constexpr int NPW = TL::NPW, MT = TL::MT, PP = TL::PP, SEG = TL::SEG, NTHR = TL::NTHR;
  // the epilogue's transposition space, 8 KB per consumer: the windows hold 4 (8 wavefronts: all there are), B image 0 four more
  constexpr int kStage = 2 * 8 * BN * 4;   // two passes of 8 rows x BN columns in flight
  static_assert(NW == 16 ? 4 * kStage <= TL::kBimgBytes / 2 && 4 * kStage <= TL::kWinBytes : kStage <= kWWave,
                "the consumers' staging areas do not fit");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* bimg = smem;
  unsigned char* wins = smem + TL::kBimgBytes;
  unsigned char* tapl = smem + TL::kBimgBytes + TL::kWinBytes;

  // consecutive tiles of an utterance on one XCD: its L2 then serves the neighbouring windows' halo
  const int bid = xcd_remap(blockIdx.x, n_blocks);
  const int b = bid / tiles_t;
  const int tile = bid % tiles_t;
  const int t0 = tile * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // role index: < NPW consumes
  const int len_in = a.lens_in[b], len_out = a.lens_out[b];
  const int len2 = DUAL ? a.lens2[b] : 0;
  constexpr int NCH = (DUAL ? 2 : 1) * (FC / FCH);

  // every source is zero from zf on: such a tile multiplies nothing, its outputs are relu(shift)
  const int zf = max(len_out, DUAL ? len2 : 0);
  const bool live = t0 < zf;

  // ---- the utterance's fp16 scale, from the bound max|x| * dw_l1 (and max|x2|) ----
  float xs = 1.f, out_scale = 1.f;
  unsigned amv[8], amv2[8];
  if (live) {
    amax_request(a.amax_x.p, a.amax_x.stride, a.amax_x.n, b, lane, amv);
    if (DUAL) amax_request(a.amax_x2.p, a.amax_x2.stride, a.amax_x2.n, b, lane, amv2);
  }
  // tap table -> LDS, all wavefronts (read by the producers after the first barrier).  Called by each role AFTER it has
  // requested its first operands (rows from HBM, weight fragments from L2): the table's trip to L2 then runs inside
  // those round trips instead of in front of them (1.6 us of a 31 us kernel when it came first).
  constexpr int kTapV4 = G::kTapBytes / 16, kTapIt = (kTapV4 + NTHR - 1) / NTHR;
  auto tap_copy = [&]() {
    v4f tv[kTapIt];
#pragma unroll
    for (int i = 0; i < kTapIt; ++i) {
      const int idx = tid + i * NTHR;
      tv[i] = reinterpret_cast<const v4f*>(a.taps)[idx < kTapV4 ? idx : kTapV4 - 1];
    }
#pragma unroll
    for (int i = 0; i < kTapIt; ++i) {
      const int idx = tid + i * NTHR;
      if (idx < kTapV4) reinterpret_cast<v4f*>(tapl)[idx] = tv[i];
    }
  };

  if (wave < NPW) {
    // =========================================== consumers =========================================================
    const int kh = lane >> 5, l31 = lane & 31;
    const int wm = wave * (32 * MT);
    constexpr int ksteps = NCH * 4;
    const uint4* __restrict__ ap = a.wt + ((int64_t)(wm / 32) * ksteps) * 2 * 64 + lane;
    const int64_t a_tile = (int64_t)ksteps * 2 * 64;
    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    if (live) {
      // B-fragment addresses of the n-tiles (swizzled column, k-half): constant over the whole tile
      int boff[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) boff[j] = (kh * BN + bimg_slot<BN>(32 * j + l31, kh)) * 16;
      // Prefetch depth.  8 wavefronts: four weight-fragment sets (requested three k-steps ahead) and three B-fragment sets
      // (two n-tiles ahead), about 90 registers, because the wavefront is alone on its SIMD's matrix pipe.  16 wavefronts: the
      // partner's MFMAs run while this one waits, and 128 registers hold 64 accumulators + two sets of 8 of each kind
      constexpr int kAS = NW == 16 ? 2 : 4, kBS = NW == 16 ? 2 : 3, kBA = kBS - 1;
      static_assert(4 % kAS == 0, "the set of a k-step must be a compile-time constant");
      uint4 aw[kAS][MT][2];   // weight fragments, set = k-step % kAS, requested kAS - 1 k-steps ahead: [set][m-tile][plane]
      auto aload = [&](int s, uint4 (&dst)[MT][2]) {
        const int sc = s < ksteps ? s : ksteps - 1;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int p = 0; p < 2; ++p) dst[i][p] = ap[i * a_tile + ((int64_t)sc * 2 + p) * 64];
      };
#pragma unroll
      for (int s = 0; s < kAS - 1; ++s) aload(s, aw[s]);
      tap_copy();
      {
        unsigned mx = amax_collect(a.amax_x.p, a.amax_x.stride, a.amax_x.n, b, lane, amv);
        mx = __float_as_uint(__uint_as_float(mx) * a.dw_l1);
        if (DUAL) mx = max(mx, amax_collect(a.amax_x2.p, a.amax_x2.stride, a.amax_x2.n, b, lane, amv2));
        float inv;
        f16_scale(mx, &xs, &inv);
        out_scale = inv * a.w_inv_scale;
      }
      lds_barrier();   // tap table complete (consumers only pass through)
#pragma unroll 1
      for (int c = 0; c < NCH; c += 2) {
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {       // two chunks per trip: the LDS buffer index is a compile-time constant
          lds_barrier();                        // B image of chunk c + cc is complete
          // B fragments: kBS sets in rotation, requested kBA n-tiles ahead (8 wavefronts: TWO, 12 MFMAs -- the wavefront is
          // alone on its SIMD's matrix pipe, nobody covers an LDS round trip it waits for; 16 wavefronts: one)
          uint4 bf[kBS][2];
#pragma unroll
          for (int g0 = 0; g0 < kBA; ++g0)
#pragma unroll
            for (int p = 0; p < 2; ++p)
              bf[g0][p] = *reinterpret_cast<const uint4*>(bimg + bimg_off<BN>(cc, p, g0 / NT) + boff[g0 % NT]);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int gs = (c + cc) * 4 + s;
            aload(gs + kAS - 1, aw[(s + kAS - 1) % kAS]);   // the set k-step s - 1 has just released
            __builtin_amdgcn_sched_barrier(0);
            uint4 (&cw)[MT][2] = aw[s % kAS];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
              const int g = s * NT + j, cur_f = g % kBS, nxt_f = (g + kBA) % kBS;
              if (g + kBA < 4 * NT) {
#pragma unroll
                for (int p = 0; p < 2; ++p)
                  bf[nxt_f][p] = *reinterpret_cast<const uint4*>(bimg + bimg_off<BN>(cc, p, (g + kBA) / NT) + boff[(g + kBA) % NT]);
              }
              __builtin_amdgcn_sched_barrier(0);   // (the scheduler would sink the reads to two MFMAs before their use)
#pragma unroll
              for (int i = 0; i < MT; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, cw[i][1]), __builtin_bit_cast(f16x8, bf[cur_f][0]), acc[i][j], 0, 0, 0);
#pragma unroll
              for (int i = 0; i < MT; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, cw[i][0]), __builtin_bit_cast(f16x8, bf[cur_f][1]), acc[i][j], 0, 0, 0);
#pragma unroll
              for (int i = 0; i < MT; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, cw[i][0]), __builtin_bit_cast(f16x8, bf[cur_f][0]), acc[i][j], 0, 0, 0);
            }
          }
        }
      }
    }
    // ---- epilogue: BN affine + ReLU, rows transposed through the (now idle) producer windows into float4 stores ----
    AmaxTracker amax{a.amax_y.p ? (a.lens_y ? a.lens_y[b] : a.frames) : 0};
    const Epilogue<EPI> epi(a.relu, a.act, 0);   // (only add-mode residuals reach this kernel, folded into the weights)
    // 2 x 8 rows x BN columns = 8 KB of the wavefront's 13 KB window (4 of 9); 16 wavefronts: consumers 0..3 in B image 0,
    // which all consumers left before the last chunk's barrier (that chunk is read from image 1), 4..7 in the windows,
    // which the producers left before that same barrier (a dead tile has no other wavefront in LDS at all)
    float* stage = reinterpret_cast<float*>(NW == 16 ? (wave < 4 ? bimg + wave * kStage : wins + (wave - 4) * kStage)
                                                     : wins + wave * kWWave);
    // every pass's BN scale / shift BEFORE the first store: stores count in vmcnt like loads, so a load issued between
    // two passes makes its consumer wait (vmcnt(0)) for every store before it -- eight store round trips in series
    v4f scv[MT][4], shv[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        scv[i][q] = *reinterpret_cast<const v4f*>(a.scale + wm + i * 32 + 8 * q + 4 * kh);
        shv[i][q] = *reinterpret_cast<const v4f*>(a.shift + wm + i * 32 + 8 * q + 4 * kh);
      }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float* buf = stage + ((i * 4 + q) & 1) * (8 * BN);
        const int mq = wm + i * 32 + 8 * q;
        const v4f sc = scv[i][q], sh = shv[i][q];
        wave_fence();
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            buf[(4 * kh + rr) * BN + 32 * j + l31] = fmaf(acc[i][j][4 * q + rr] * out_scale, sc[rr], sh[rr]);
        wave_fence();
        // straight-line pass (no uniform branch per piece: see encoder_pw_split.hip's epilogue): all row pieces requested
        // together, ReLU as a maximum with a uniform floor
        v4f pv[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
          const int f = lane + 64 * k, row = f / (BN / 4), c4 = f % (BN / 4);
          pv[k] = *reinterpret_cast<const v4f*>(buf + row * BN + 4 * c4);
        }
#pragma unroll
        for (int k = 0; k < NT; ++k) {
          const int f = lane + 64 * k, row = f / (BN / 4), c4 = f % (BN / 4);
          const int m = mq + row, t = t0 + 4 * c4;
          const v4f v = epi.apply4(pv[k]);
          *reinterpret_cast<v4f*>(a.y + ((int64_t)b * FC + m) * a.ldy + t) = v;
          amax.track4(v, t);
        }
      }
    }
    if (a.amax_y.p) amax_publish(a.amax_y.p, a.amax_y.stride, b, tile * NPW + wave, amax.ymax, lane);
    return;
  }

  // ============================================= producers ===========================================================
  if (!live) return;
  // 8 wavefronts: wavefront pw produces k-step pw of the chunk (16 channels, both k-halves); 16 wavefronts: k-half pw & 1 of
  // k-step pw >> 1 (8 channels)
  const int pw = wave - NPW;
  const int p = lane / SEG, s = lane % SEG;   // channel pair, segment of FPS frames
  const int ks = NW == 16 ? pw >> 1 : pw;     // k-step of the chunk this wavefront writes
  const int kp = NW == 16 ? (pw & 1) * 4 + p : p;   // channel pair inside that k-step
  unsigned char* win = wins + pw * kWWave;
  // the rows of a chunk as (pair, float4 column) items: item = lane + 64 j
  auto item = [&](int j, int& sp, int& q) { const int idx = lane + 64 * j; sp = idx / G::W4; q = idx - sp * G::W4; };
  v4f st[G::NLD][2];
  auto gload_dw = [&](int c) {
    const float* xb = a.x + ((int64_t)b * FC + c * FCH + pw * (2 * PP)) * a.ldx;
#pragma unroll
    for (int j = 0; j < G::NLD; ++j) {
      int sp, q;
      item(j, sp, q);
      sp = sp < PP ? sp : PP - 1;
      int t = t0 - G::PADL + 4 * q;
      t = t < 0 ? 0 : (t > (int)a.ldx - 4 ? (int)a.ldx - 4 : t);
      // a uniform base per row parity + one 32-bit lane offset per item (at most 15 rows of a pitch that 256 channels of
      // float32 keep far below 2^27): the addresses are loop invariants, and as 64-bit lane pointers they cost four
      // registers an item where the 16-wavefront form has none to spare
      const unsigned off = (unsigned)(2 * sp * (int)a.ldx + t);   // (t >= 0 after the clamp)
      st[j][0] = *reinterpret_cast<const v4f*>(xb + off);
      st[j][1] = *reinterpret_cast<const v4f*>(xb + a.ldx + off);
    }
  };
  // residual chunks: 2 rows x FPS frames per lane, no halo (st[0 .. FPS / 4) hold them)
  auto gload_x2 = [&](int c) {
    const float* xb = a.x2 + ((int64_t)b * FC + (c - FC / FCH) * FCH + pw * (2 * PP)) * a.ldx2 + t0;
    const float* xb1 = xb + a.ldx2;
    const unsigned off = (unsigned)(2 * p * (int)a.ldx2 + FPS * s);
#pragma unroll
    for (int j = 0; j < FPS / 4; ++j) {
      st[j][0] = *reinterpret_cast<const v4f*>(xb + (off + 4 * j));
      st[j][1] = *reinterpret_cast<const v4f*>(xb1 + (off + 4 * j));
    }
  };
  gload_dw(0);
  tap_copy();
  {
    unsigned mx = amax_collect(a.amax_x.p, a.amax_x.stride, a.amax_x.n, b, lane, amv);
    mx = __float_as_uint(__uint_as_float(mx) * a.dw_l1);
    if (DUAL) mx = max(mx, amax_collect(a.amax_x2.p, a.amax_x2.stride, a.amax_x2.n, b, lane, amv2));
    float inv;
    f16_scale(mx, &xs, &inv);
  }
  lds_barrier();   // tap table complete

  const int kh = kp >> 2;
  // address of this lane's 4 bytes in the B image, for frame j of its segment: column n = FPS s + j (bimg_slot: the bits
  // of j sit below FPS, so low4 = j ^ const and the aligned group is the segment's)
  const int wbase = (kh * BN) * 16 + 4 * (kp & 3);
  const int nsw = (FPS * s) & ~15;
  const int sx = (((FPS * s) & 15) ^ (((FPS * s) >> 4) | (kh << TL::KHS))) << 4;
  // converts the FPS (pair, frame) results of this lane and writes them into B image `buf`, k-step ks
  auto emit = [&](int buf, const v2f (&d)[FPS], int nvalid) {
    int sxx = sx;
    // 16 wavefronts: the FPS scales (as register pairs) and FPS addresses below are loop invariants the compiler would
    // hold across the chunk loop -- 24 registers of 128; opaque inputs make it recompute them per chunk (two instructions each)
    if constexpr (NW == 16) asm volatile("" : "+v"(nvalid), "+v"(sxx));
#pragma unroll
    for (int j = 0; j < FPS; ++j) {
      const float sj = j < nvalid ? xs : 0.f;              // MaskedConv1d: the pointwise conv sees zeros past lens_out
      const v2f v = {d[j].x * sj, d[j].y * sj};
      const f16x2 hv = __builtin_convertvector(v, f16x2);
      const v2f r = v - __builtin_convertvector(hv, v2f);   // exact: the residual of a round-to-nearest conversion
      const f16x2 lv = __builtin_convertvector(r, f16x2);
      const int off = wbase + ((nsw << 4) | ((j << 4) ^ sxx));
      *reinterpret_cast<unsigned*>(bimg + bimg_off<BN>(buf, 0, 0) + ks * (2 * BN * 16) + off) = __builtin_bit_cast(unsigned, hv);
      *reinterpret_cast<unsigned*>(bimg + bimg_off<BN>(buf, 1, 0) + ks * (2 * BN * 16) + off) = __builtin_bit_cast(unsigned, lv);
    }
  };

  const unsigned char* rd = win + p * kWPitch + TL::kSegBytes * s;   // this lane's window region
  const int nvalid = len_out - (t0 + FPS * s);
#pragma unroll 1
  for (int c = 0; c < FC / FCH; c += 2) {
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int ch = c + cc;
      // ---- masked rows of chunk ch -> interleaved pairs in the wavefront's LDS window ----
#pragma unroll
      for (int j = 0; j < G::NLD; ++j) {
        int sp, q;
        item(j, sp, q);
        const int t = t0 - G::PADL + 4 * q;
        v4f u = st[j][0], w = st[j][1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool ok = (unsigned)(t + e) < (unsigned)len_in;   // t < 0: conv zero padding; t >= lens: masked_fill
          u[e] = ok ? u[e] : 0.f;
          w[e] = ok ? w[e] : 0.f;
        }
        if (sp < PP) {
          unsigned char* dst = win + sp * kWPitch + (4 * q) * 8 + ((4 * q) / FPS) * 16;   // 16 bytes of pad per FPS frames
          *reinterpret_cast<v4f*>(dst) = v4f{u.x, w.x, u.y, w.y};
          *reinterpret_cast<v4f*>(dst + 16) = v4f{u.z, w.z, u.w, w.w};
        }
      }
      wave_fence();
      // rows of the next chunk (or of the first residual chunk): in flight during this chunk's FMAs
      if (ch + 1 < FC / FCH) gload_dw(ch + 1);
      else if (DUAL) gload_x2(FC / FCH);
      // ---- depthwise: acc[j] = sum_k w[k] * x[OFF + j + k], both channels of the pair per packed FMA ----
      const unsigned char* tp = tapl + ((ch * FCH + pw * (2 * PP)) / 2 + p) * (G::KP * 8);
      v2f xw[2 * G::NR];
      auto load_units = [&](int qa, int qb) {
#pragma unroll
        for (int qq = qa; qq < qb; ++qq) {
          const v4f v = *reinterpret_cast<const v4f*>(rd + qq * 16 + (qq / (FPS / 2)) * 16);   // frames 2 qq, 2 qq + 1
          xw[2 * qq] = v.xy;
          xw[2 * qq + 1] = v.zw;
        }
      };
      v2f acc[FPS];
#pragma unroll
      for (int j = 0; j < FPS; ++j) acc[j] = v2f{0.f, 0.f};
      load_units(0, G::qend(0));
      v2f wn[G::TB];   // taps of the NEXT block: their LDS round trip runs under this block's FMAs
      auto load_taps = [&](int blk) {
#pragma unroll
        for (int k2 = 0; k2 < G::TB / 2; ++k2) {
          if (G::TB * blk + 2 * k2 < G::KP) {
            const v4f v = *reinterpret_cast<const v4f*>(tp + (G::TB * blk + 2 * k2) * 8);
            wn[2 * k2] = v.xy;
            wn[2 * k2 + 1] = v.zw;
          }
        }
      };
      load_taps(0);
#pragma unroll
      for (int blk = 0; blk < G::NB; ++blk) {
        v2f wt[G::TB];
#pragma unroll
        for (int k = 0; k < G::TB; ++k) wt[k] = wn[k];
        if (blk + 1 < G::NB) {
          load_taps(blk + 1);
          load_units(G::qend(blk), G::qend(blk + 1));
        }
#pragma unroll
        for (int k = G::TB * blk; k < G::TB * (blk + 1) && k < K; ++k) {
#pragma unroll
          for (int j = 0; j < FPS; ++j) acc[j] = __builtin_elementwise_fma(wt[k - G::TB * blk], xw[G::OFF + j + k], acc[j]);
          // one tap at a time over all FPS accumulators: left alone, the scheduler turns the loops inside out (one output
          // at a time, its taps as a dependent chain with a wait state between links) to save registers
#pragma unroll
          for (int j = 0; j < FPS; ++j) asm volatile("" : "+v"(acc[j]));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      emit(cc, acc, nvalid);
      lds_barrier();   // hands B image `cc` (chunk ch) to the consumers; they have finished chunk ch - 1
    }
  }
  if constexpr (DUAL) {
    const int nv2 = len2 - (t0 + FPS * s);
#pragma unroll 1
    for (int c = FC / FCH; c < NCH; c += 2) {
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const int ch = c + cc;
        v2f d[FPS];
#pragma unroll
        for (int j = 0; j < FPS / 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) d[4 * j + e] = v2f{st[j][0][e], st[j][1][e]};
        if (ch + 1 < NCH) gload_x2(ch + 1);
        emit(cc, d, nv2);   // the block input is masked with ITS lens (jasper.py:428-436), zeros past it
        lds_barrier();
      }
    }
  }
}

template <int K, bool DUAL, int BN, int NW = 8>
int launch_fused_t(const FusedArgs& a, hipStream_t st, int* amax_n) {
  using G = FGeom<K, BN, NW>;
  const int tiles_t = (int)(a.ldy / BN);
  const int n_blocks = tiles_t * a.batch;
  constexpr int slots = FTile<BN, NW>::NPW;   // maxima slots per tile: one per consumer wavefront
  if (a.amax_y.p) {
    if (tiles_t * slots > a.amax_y.stride) return (int)hipErrorInvalidValue;
    if (amax_n) *amax_n = tiles_t * slots;
  }
  // Hardtanh and SELU take epilogue 1 or 2 (only add-mode residuals reach this kernel); the ReLU kernels stay as they were
  const int epi = epilogue_kind(a.relu, a.act, false);
  auto kern = epi == 2   ? dwpw_fused_kernel<K, DUAL, BN, 2, NW>
              : epi == 1 ? dwpw_fused_kernel<K, DUAL, BN, 1, NW>
                         : dwpw_fused_kernel<K, DUAL, BN, 0, NW>;
  static std::atomic<uint64_t> lds_opted[3];   // per device and epilogue (dyn_lds_opt_in)
  const hipError_t attr = dyn_lds_opt_in(reinterpret_cast<const void*>(kern), (int)G::LDS, lds_opted[epi]);
  if (attr != hipSuccess) return (int)attr;
  VASR_LAUNCH(kern, dim3(n_blocks), dim3(NW * 64), G::LDS, st, a, tiles_t, n_blocks);
  return 0;
}

template <int K, bool DUAL>
int launch_fused_128(const FusedArgs& a, int waves, hipStream_t st, int* amax_n) {
  return waves == 16 ? launch_fused_t<K, DUAL, 128, 16>(a, st, amax_n) : launch_fused_t<K, DUAL, 128, 8>(a, st, amax_n);
}

}  // namespace

// Wavefronts per workgroup of the fused kernel for a sub-block (kernel, folded residual) on tiles of tile_cols frames:
// forced (VASR_FUSED_WAVES, devtools build) where the form exists -- the 128-frame tile -- else the measured default
// (profiles/fused16_bench.json).  The 64-frame tile has the 8-wavefront form only.
int fused_waves_choice(int kernel, bool dual, int tile_cols, int forced) {
  if (tile_cols == 64) return 8;
  if (forced == 8 || forced == 16) return forced;
  (void)kernel; (void)dual;
  return 16;
}

bool fused_dwpw_supported(int channels, int cout, int kernel, int stride, int dilation) {
  return channels == FC && cout == FC && stride == 1 && dilation == 1 && (kernel == 33 || kernel == 39);
}
int fused_dwpw_taps_per_pair(int kernel) { return (kernel + 2) & ~1; }

// host: depthwise weights [C][K] -> [C / 2][KP][2] (channel pairs interleaved, zero padded); returns max_c sum_k |w|
float pack_fused_taps(const float* w, int channels, int kernel, float* out) {
  const int kp = fused_dwpw_taps_per_pair(kernel);
  float l1 = 0.f;
  for (int c = 0; c < channels; ++c) {
    double s = 0;
    for (int k = 0; k < kernel; ++k) s += std::fabs((double)w[(size_t)c * kernel + k]);
    l1 = (float)s > l1 ? (float)s : l1;
  }
  for (int pr = 0; pr < channels / 2; ++pr)
    for (int k = 0; k < kp; ++k)
      for (int h = 0; h < 2; ++h)
        out[((size_t)pr * kp + k) * 2 + h] = k < kernel ? w[(size_t)(2 * pr + h) * kernel + k] : 0.f;
  // one ulp up: the bound must not fall below the true sum through the float rounding of this very sum
  return __builtin_nextafterf(l1, 3.0e38f);
}

int launch_fused_dwpw(const FusedLaunch& f, hipStream_t st, int* amax_n) {
  FusedArgs a{};
  a.x = f.x; a.ldx = f.ldx; a.lens_in = f.lens_in; a.lens_out = f.lens_out; a.taps = f.taps; a.dw_l1 = f.dw_l1;
  a.amax_x = f.amax_x; a.wt = reinterpret_cast<const uint4*>(f.wt); a.w_inv_scale = f.w_inv_scale; a.scale = f.scale;
  a.shift = f.shift; a.y = f.y; a.ldy = f.ldy; a.frames = f.frames; a.relu = f.relu; a.act = f.act; a.amax_y = f.amax_y;
  a.lens_y = f.lens_y; a.x2 = f.x2; a.ldx2 = f.ldx2; a.lens2 = f.lens2; a.amax_x2 = f.amax_x2; a.batch = f.batch;
  const bool dual = f.x2 != nullptr;
  if (f.tile_cols == 64) {
    if (f.kernel == 33) return dual ? launch_fused_t<33, true, 64>(a, st, amax_n) : launch_fused_t<33, false, 64>(a, st, amax_n);
    if (f.kernel == 39) return dual ? launch_fused_t<39, true, 64>(a, st, amax_n) : launch_fused_t<39, false, 64>(a, st, amax_n);
    return -1;
  }
  const int waves = fused_waves_choice(f.kernel, dual, 128, f.waves);
  if (f.kernel == 33) return dual ? launch_fused_128<33, true>(a, waves, st, amax_n) : launch_fused_128<33, false>(a, waves, st, amax_n);
  if (f.kernel == 39) return dual ? launch_fused_128<39, true>(a, waves, st, amax_n) : launch_fused_128<39, false>(a, waves, st, amax_n);
  return -1;
}

}  // namespace vasr
