// SpecAugment / SpecCutout for gfx950: rectangles of a [B][feat][ld] float32 feature tensor set to +0.0f (reference
// nemo/collections/asr/parts/spectr_augment.py: `x.masked_fill(mask, 0)`).  The host draws the rectangles (viet-asr_amd/asr.py
// consumes Python's generator as the reference does) and uploads them resolved, as a CSR list per batch row; this file is the
// stores.  include/vasr.h (vasr_spec_mask_f32) has the contract, DESIGN.md section 7i the two forms:
//
//   in place     one workgroup per (batch row, kSpecRows feature rows).  It walks the row's rectangles and stores zeros over
//                the part of each that lies in its feature rows; the tensor is never read, a row without rectangles costs two
//                dword loads per workgroup.  32 lanes share one feature row and store 16 bytes each where the address is
//                16-byte aligned and the four cells lie inside the rectangle, single dwords at its ragged ends.
//   out of place one workgroup per (batch row, kSpecRows feature rows, kSpecTile frames): every thread owns 4 frames of each of
//                the 8 feature rows, builds their 32 mask bits from the rectangle list (staged through LDS kSpecChunk at a time),
//                then copies.  Where both pitches and both bases are multiples of 16 bytes the 4 frames are consecutive: eight
//                16-byte loads issued before the first of eight 16-byte stores.  Otherwise (a contiguous port tensor of 1 001
//                frames) they lie kSpecBlock apart and travel as dwords, contiguous across the wavefront.
//
// Cells travel as 32-bit integers: a kept cell keeps its bit pattern (NaN payloads, -0.0), a masked one becomes 0x00000000.
// Every rectangle is clipped to [0, feat) x [0, frames) before it is used, so no store leaves the tensor whatever the device
// arrays hold; columns frames .. ld are never written.  Plain vector stores only, no atomics: overlapping rectangles store the
// same value.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vasr_internal.h"

namespace vasr {

namespace {

struct Rect { int f0, f1, t0, t1; };

// rectangle i of the list, clipped to the tensor; an empty one comes back with f0 >= f1 or t0 >= t1
__device__ inline Rect clipped_rect(const int32_t* __restrict__ rects, int64_t i, int feat, int frames) {
  const int32_t* r = rects + 4 * i;
  Rect c;
  c.f0 = max(r[0], 0); c.f1 = min(r[1], feat);
  c.t0 = max(r[2], 0); c.t1 = min(r[3], frames);
  return c;
}

// the list of batch row b: [*begin, *begin + return value); a non-increasing pair or a negative begin is empty
__device__ inline int row_rects(const int32_t* __restrict__ row_begin, int b, int64_t* begin) {
  const int lo = row_begin[b], hi = row_begin[b + 1];
  *begin = lo;
  return lo >= 0 && hi > lo ? hi - lo : 0;
}

__global__ __launch_bounds__(kSpecBlock) void spec_mask_inplace_kernel(float* __restrict__ x, int64_t ld, int feat, int frames,
                                                                       int f_tiles, const int32_t* __restrict__ rects,
                                                                       const int32_t* __restrict__ row_begin) {
  const int b = blockIdx.x / f_tiles, f_lo = (blockIdx.x % f_tiles) * kSpecRows;
  int64_t begin;
  const int n = row_rects(row_begin, b, &begin);
  if (n == 0) return;
  const int f = f_lo + (int)threadIdx.x / 32, lane = threadIdx.x % 32;   // kSpecBlock / 32 == kSpecRows
  if (f >= feat) return;
  uint32_t* row = reinterpret_cast<uint32_t*>(x) + ((int64_t)b * feat + f) * ld;
  // dword address of the row's first cell: 16-byte units are counted in absolute addresses, so that a pitch or a base that is
  // no multiple of 4 cells only moves where the ragged ends are
  const uint64_t a_row = reinterpret_cast<uintptr_t>(row) >> 2;
  for (int i = 0; i < n; ++i) {
    const Rect r = clipped_rect(rects, begin + i, feat, frames);   // uniform over the wavefront: scalar loads
    if (f < r.f0 || f >= r.f1 || r.t0 >= r.t1) continue;
    const uint64_t a0 = a_row + (uint64_t)r.t0, a1 = a_row + (uint64_t)r.t1;
    for (uint64_t u = (a0 >> 2) + lane; u < ((a1 + 3) >> 2); u += 32) {
      const uint64_t c0 = u << 2;
      if (c0 >= a0 && c0 + 4 <= a1) {
        *reinterpret_cast<uint4*>(row + (c0 - a_row)) = make_uint4(0u, 0u, 0u, 0u);
      } else {
        for (int j = 0; j < 4; ++j)
          if (c0 + j >= a0 && c0 + j < a1) row[c0 + j - a_row] = 0u;
      }
    }
  }
}

__global__ __launch_bounds__(kSpecBlock) void spec_mask_copy_kernel(const float* __restrict__ in, int64_t ld_in,
                                                                    float* __restrict__ out, int64_t ld_out, int feat, int frames,
                                                                    int f_tiles, int t_tiles, const int32_t* __restrict__ rects,
                                                                    const int32_t* __restrict__ row_begin) {
  __shared__ Rect s_rect[kSpecChunk];
  const int t_tile = blockIdx.x % t_tiles, f_tile = (blockIdx.x / t_tiles) % f_tiles, b = blockIdx.x / (t_tiles * f_tiles);
  const int f_lo = f_tile * kSpecRows;
  // Where both pitches and both bases are multiples of 16 bytes every row of the tile is, and a thread owns 4 consecutive frames
  // (one 16-byte access per row); otherwise it owns 4 frames kSpecBlock apart, so that a wavefront's dword accesses are
  // contiguous.  The choice is uniform over the launch.  (frames < 2^31 - 2 kSpecTile: no index below overflows)
  const bool aligned = (((ld_in | ld_out) & 3) == 0) &&
                       (((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0);
  const int t = t_tile * kSpecTile + (aligned ? 4 * (int)threadIdx.x : (int)threadIdx.x);   // this thread's first frame
  const int step = aligned ? 1 : kSpecBlock;                                                // ... and the distance to its next
  int64_t begin;
  const int n = row_rects(row_begin, b, &begin);
  uint32_t mask = 0;   // bit 4 r + j: cell (f_lo + r, t + j step) is masked
  for (int base = 0; base < n; base += kSpecChunk) {
    const int m = min(n - base, kSpecChunk);
    if (base) __syncthreads();
    if ((int)threadIdx.x < m) s_rect[threadIdx.x] = clipped_rect(rects, begin + base + threadIdx.x, feat, frames);
    __syncthreads();
    for (int i = 0; i < m; ++i) {
      const Rect r = s_rect[i];
      const int r0 = max(r.f0 - f_lo, 0), r1 = min(r.f1 - f_lo, kSpecRows);
      uint32_t cols = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) cols |= (t + j * step >= r.t0 && t + j * step < r.t1) ? 1u << j : 0u;
      if (r0 >= r1 || cols == 0) continue;
      for (int r_ = r0; r_ < r1; ++r_) mask |= cols << (4 * r_);
    }
  }
  if (t >= frames) return;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(in) + (int64_t)b * feat * ld_in + t;
  uint32_t* dst = reinterpret_cast<uint32_t*>(out) + (int64_t)b * feat * ld_out + t;
  if (aligned && t + 4 <= frames) {
    // all eight loads are issued before the first store; a row past the last one re-reads the last (and is not stored)
    uint4 v[kSpecRows];
#pragma unroll
    for (int r = 0; r < kSpecRows; ++r)
      v[r] = *reinterpret_cast<const uint4*>(src + (int64_t)min(f_lo + r, feat - 1) * ld_in);
#pragma unroll
    for (int r = 0; r < kSpecRows; ++r) {
      const uint32_t m = mask >> (4 * r);
      uint4 y = v[r];
      y.x = (m & 1u) ? 0u : y.x; y.y = (m & 2u) ? 0u : y.y; y.z = (m & 4u) ? 0u : y.z; y.w = (m & 8u) ? 0u : y.w;
      if (f_lo + r < feat) *reinterpret_cast<uint4*>(dst + (int64_t)(f_lo + r) * ld_out) = y;
    }
    return;
  }
  // dwords: the whole tile where it is not aligned, the row's last thread where frames is no multiple of 4
  for (int r = 0; r < kSpecRows && f_lo + r < feat; ++r) {
    const uint32_t* s = src + (int64_t)(f_lo + r) * ld_in;
    uint32_t* d = dst + (int64_t)(f_lo + r) * ld_out;
    uint32_t y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = t + j * step < frames ? s[j * step] : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t + j * step < frames) d[j * step] = ((mask >> (4 * r + j)) & 1u) ? 0u : y[j];
  }
}

}  // namespace

void launch_spec_mask(const float* in, int64_t ld_in, float* out, int64_t ld_out, int batch, int feat, int frames,
                      const int32_t* rects, const int32_t* row_begin, hipStream_t st) {
  const int f_tiles = (int)(((int64_t)feat + kSpecRows - 1) / kSpecRows);
  if (in == out) {
    hipLaunchKernelGGL(spec_mask_inplace_kernel, dim3((unsigned)(batch * f_tiles)), dim3(kSpecBlock), 0, st, out, ld_out, feat,
                       frames, f_tiles, rects, row_begin);
    return;
  }
  const int t_tiles = (frames + kSpecTile - 1) / kSpecTile;
  hipLaunchKernelGGL(spec_mask_copy_kernel, dim3((unsigned)(batch * f_tiles * t_tiles)), dim3(kSpecBlock), 0, st, in, ld_in, out,
                     ld_out, feat, frames, f_tiles, t_tiles, rects, row_begin);
}

}  // namespace vasr
