// The vector epilogue of the implicit-GEMM 3x3 conv kernels: shared by the
// 128-tile kernel (conv.hip) and the 256x256 kernel (conv_v4.hip).
#pragma once
#include "common.h"

// ---- vector epilogue, shared by both conv kernels --------------------------
// Kernel argument `flags`: what the host checked for this launch.
#define CONV_F_VEC 1        // Y + column offset 16-B aligned, cols and ldY % 8
#define CONV_F_BIAS_BF16 2  // bias points at bf16, not fp32

// The bias is read as stored: bf16 -> fp32 is exact, so no per-call copy.
__device__ __forceinline__ float conv_bias_at(const void *bias, int flags,
                                              int co) {
  return (flags & CONV_F_BIAS_BF16)
             ? bf2f(((const __hip_bfloat16 *)bias)[co])
             : ((const float *)bias)[co];
}

// Bytes of wave-private LDS one 64-row strip of NJ column fragments takes:
// bf16 rows of NJ*16 columns, padded by 16 B so the four lane quarters of a
// fragment write (rows 4 apart) land 16 banks apart.
template <int NJ>
constexpr int conv_epi_stride = NJ * 32 + 16;
template <int NJ>
constexpr int conv_epi_bytes = 64 * conv_epi_stride<NJ>;

// One wave's 64-row x (NJ*16)-column strip of a FULL tile (every row < M,
// every column < cols: the caller's block-uniform test), acc in the MFMA
// layout: row = i*16 + (lane/16)*4 + r, column = j*16 + lane%16.
//  1. in that layout: v = ((acc + bias) + cb) + res in fp32, one f2bf, the
//     GroupNorm partials over the rounded values in the element-wise path's
//     order; residual (and multi-image channel-bias) loads of a fragment
//     row are issued together, offsets are 32-bit from wave-uniform bases;
//  2. the bf16 strip goes through the wave's private LDS region `wl`
//     (wave-local ordering only: s_waitcnt lgkmcnt, no barrier);
//  3. each lane stores 16 B = 8 consecutive channels of one row, so a wave
//     writes whole NJ*32-byte row segments.
// CB_ONE: the whole tile lies in one image, cbv[] holds its channel bias;
// otherwise row `row` of the strip belongs to image (rem0 + row) / HoWo
// past the one `cbw` points at. FOLD: row = source pixel mrow + row, stored
// at output pixel (2i+fa, 2j+fb); `yw` is then Y + the wave's column base.
// TIGHT (the v4 kernel, 128 accumulator VGPRs): the loads run exactly one
// fragment row ahead of their use, pinned by sched_barrier, because hoisting
// all four rows' loads would spill; the multi-image channel bias then loads
// in place. Otherwise the compiler is free to hoist every load.
template <bool HAS_RES, bool HAS_CB, bool CB_ONE, bool FOLD, int NJ,
          bool TIGHT>
__device__ __forceinline__ void conv_epi_strip(
    const f32x4 (&acc)[4][NJ], const float (&bv)[NJ], const float (&cbv)[NJ],
    const __hip_bfloat16 *__restrict__ cbw, unsigned rem0, unsigned HoWo,
    const __hip_bfloat16 *__restrict__ resw, __hip_bfloat16 *__restrict__ yw,
    long mrow, int W, int Wo, int fa, int fb, unsigned ldY, char *wl,
    int lane, float (&gs)[NJ], float (&gq)[NJ]) {
  constexpr int STRIDE = conv_epi_stride<NJ>;
  constexpr bool LOADS = HAS_RES || (HAS_CB && !CB_ONE);
  constexpr bool AHEAD = !(TIGHT && HAS_CB && !CB_ONE);
  const unsigned l16 = lane % 16, r4 = (lane / 16) * 4;
  float rv[2][NJ][4], cv[2][NJ][4];
  // per-lane BYTE offsets of the fragment's four rows, shared by every i:
  // the 16-row step goes onto the wave-uniform base and the column onto the
  // instruction's immediate, so a load is base + 32-bit offset + constant
  unsigned voff[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) voff[r] = ((r4 + r) * ldY + l16) * 2;
  // residual and channel bias of fragment row i into slot b
  auto fetch = [&](int i, int b) {
    const char *ri = (const char *)resw + (size_t)(i * 16) * ldY * 2;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      unsigned coff = l16 * 2;
      if constexpr (HAS_CB && !CB_ONE)
        coff += ((rem0 + i * 16 + r4 + r) / HoWo) * ldY * 2;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if constexpr (HAS_RES)
          rv[b][j][r] =
              (float)*(const __hip_bfloat16 *)((ri + voff[r]) + j * 32);
        if constexpr (HAS_CB)
          cv[b][j][r] = CB_ONE ? cbv[j]
                               : (float)*(const __hip_bfloat16 *)(
                                     ((const char *)cbw + coff) + j * 32);
      }
    }
  };
  if constexpr (AHEAD) fetch(0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (AHEAD) {
      if (i + 1 < 4) fetch(i + 1, (i + 1) & 1);
    } else {
      fetch(i, i & 1);
    }
    if constexpr (TIGHT && LOADS) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[i][j][r] + bv[j];
        if constexpr (HAS_CB) v += cv[i & 1][j][r];
        if constexpr (HAS_RES) v += rv[i & 1][j][r];
        const __hip_bfloat16 vb = f2bf(v);
        *(__hip_bfloat16 *)(wl + (i * 16 + r4 + r) * STRIDE +
                            (j * 16 + l16) * 2) = vb;
        // stats over the STORED values; taken always (three VALU ops an
        // element, no branch), used only when the caller collects them
        const float vr = bf2f(vb);
        gs[j] += vr;
        gq[j] += vr * vr;
      }
    }
    if constexpr (TIGHT && LOADS) __builtin_amdgcn_sched_barrier(0);
  }
  // the strip is in LDS: only this wave wrote it, only this wave reads it.
  // The strip is written as bf16 elements and read back as uint4, by other
  // lanes than wrote it: what orders the two for the compiler is this asm's
  // "memory" clobber (no LDS access may move across it), and for the
  // hardware the wave's in-order LDS queue, drained here
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  constexpr int CH = NJ * 2;    // 16-B chunks per row
  constexpr int RP = 64 / CH;   // rows per pass; CH passes cover 64 rows
  const unsigned prow = lane / CH, pch = lane % CH;
  uint4 ov[CH];
#pragma unroll
  for (int p = 0; p < CH; ++p)
    ov[p] = *(const uint4 *)(wl + (p * RP + prow) * STRIDE + pch * 16);
  const unsigned soff = (prow * ldY + pch * 8) * 2;  // bytes
#pragma unroll
  for (int p = 0; p < CH; ++p) {
    const unsigned row = p * RP + prow;
    if constexpr (FOLD) {
      // source pixel (n, i, j) -> output row (n, 2i+a, 2j+b); with
      // q = n*H + i, n*Ho + 2i is 2q (host: source pixels fit an int)
      const unsigned m = (unsigned)mrow + row;
      const unsigned q = m / (unsigned)W;
      const unsigned jw = m - q * (unsigned)W;
      const long orow = (long)(2 * q + fa) * Wo + 2 * jw + fb;
      *(uint4 *)(yw + orow * (long)ldY + pch * 8) = ov[p];
    } else {
      *(uint4 *)(((char *)yw + (size_t)(p * RP) * ldY * 2) + soff) = ov[p];
    }
  }
  // the next strip's bf16 writes must not pass these uint4 reads: again
  // the "memory" clobber is what holds the compiler to it
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}


