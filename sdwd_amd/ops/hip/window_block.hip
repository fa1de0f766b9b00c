// The window-attention half of a Swin-Conv block (SCUNet) in one kernel on
// gfx950, for branch widths C = 32 and 64 (1 or 2 heads of 32 channels):
//
//   n1  = LN(x; g1, b1)                        -> bf16
//   qkv = n1 Wqkv^T + bqkv                     -> q, k, v bf16
//   s   = scale <q, k> + rel[h, di + 7, dj + 7]   fp32, shifted windows masked
//   o   = softmax(s) v                         -> P bf16 once, o bf16
//   y   = x + o Wp^T + bp                      fp32 sum, one bf16 rounding
//   n2  = LN(y_fp32; g2, b2)                   one bf16 rounding
//
// x, y, n2 are [B, H, W, C] views with unit channel stride; windows are 8 x 8
// and the addressing is attention_swin.hip's: window (wy, wx), local token
// (i, j) is grid token ((8 wy + i + shift) mod H, (8 wx + j + shift) mod W),
// and both outputs are written at that token. Nothing is rolled, partitioned
// or reversed, and no qkv, attention or proj tensor exists in memory: the
// kernel reads x and writes y and n2.
//
//  * work split: a wave owns whole windows (64 tokens = two 32-row MFMA
//    tiles) and walks windows g, g + G, ... as swin_attn_bf16_kernel does. A
//    block is four such waves; they share only the staged weights.
//  * weights: Wqkv, Wp (ops.window_attn_block_prepare: every MFMA fragment a
//    contiguous 1 KB block, lane l's 16 bytes at 16 l), the norm vectors, the
//    biases and rel (log2 units, rows padded to 16) are staged into LDS once
//    per block, one barrier; after it there is no barrier and no LDS write.
//    A fragment read is one conflict-free ds_read_b128 a lane, and every
//    weight fragment is read once per window and used for both token tiles.
//  * operand chain: every intermediate is born in the register layout its
//    consumer reads, so no activation goes through LDS at all. All GEMMs are
//    v_mfma_f32_32x32x16_bf16; "swapped" means the weight is the A operand:
//      - x is loaded as 16-byte pieces: lane (lq, half) holds channels
//        16c + 8 half .. +8 of token lq of each tile: after LN1 that IS the B
//        fragment of a swapped GEMM (and the A fragment of an unswapped one).
//      - Q^T, K^T = mfma(W_frag, n1_frag): a lane holds channels crow(r, half)
//        of its token, and p_relayout turns the tile into the two 16-deep
//        fragments QK^T reads (the layout swin_attn_bf16_kernel loads).
//      - V = mfma(n1_frag, Wv_frag), NOT swapped: a lane holds tokens
//        crow(r, half) of channel lq, and p_relayout gives the transposed V
//        fragments of PV (what the swin kernel gets from ds_read_b64_tr_b16).
//      - S^T = mfma(K_frag, Q_frag), softmax over the lane's 32 scores and
//        lane ^ 32, O^T = mfma(V_frag, P_frag), 1/l a lane constant: the swin
//        kernel's. p_relayout of O^T is the B fragment of the proj GEMM.
//      - Y^T = mfma(Wp_frag, o_frag), after the last head, into accumulators
//        that START as x + bp in fp32 (x waits as the bf16 it was loaded as,
//        which is exact; the accumulators are not live under the attention).
//  * residual: x's fp32 copy moves from the fragment layout to the
//    accumulator layout with one v_permlane32_swap per two values (the swap
//    p_relayout uses, on whole fp32 registers). C = 32 keeps x in registers;
//    C = 64 reads the rows again, from cache (holding them made it spill).
//  * rel is read by offset: the score of query (ip, jp) against key (iq, jq)
//    adds rel[h][ip - iq + 7][jp - jq + 7]; in the accumulator layout that is
//    a lane base plus a compile-time offset, one ds_read_b32 each, all lanes
//    of a read on distinct banks or the same word.
//  * mask: shift > 0 only, last window row / column only: a wave-uniform
//    branch, qs != sub for rows and a lane constant for columns, adding -inf
//    (p = 0 exactly; a query always keeps its own key, so the max is finite).
//  * LN1 statistics: the lane's C/2 values plus one exchange with lane ^ 32,
//    two-pass. LN2: the same over the fp32 accumulators (swin_mlp's epilogue).
//  * stores: p_relayout of an accumulator tile is channels 32n + 8 half .. +8
//    and 32n + 16 + 8 half .. +8 of the lane's token: two 16-byte stores.
//  * compiled without packed fp32 VALU ops (WIDE_KERNEL_ATTR); no atomics,
//    every output element is written once by one lane.

#include "common.h"

#include <algorithm>
#include <tuple>

struct WinBlockArgs {
  long xb, xy, xx;  // x strides (elements): batch, grid row, grid column
  long yb, yy, yx;  // y
  long nb, ny, nx;  // n2
  int H, W;         // token grid
  int nwy, nwx;     // windows per grid column / row
  int nwin;         // B * nwy * nwx
  int shift;        // 0 or 4
  float scale;
  float eps;
};

constexpr int WB_REL_ROW = 16;             // LDS row of rel (15 used)
constexpr int WB_REL_HEAD = 15 * WB_REL_ROW;

// LayerNorm statistics of a token whose values two lanes (l, l ^ 32) share
__device__ __forceinline__ void wb_stats(float s, float &mean, int lane,
                                         float inv_c) {
  s += wide_shfl(s, lane ^ 32);
  mean = s * inv_c;
}

template <int C>
WIDE_KERNEL_ATTR __launch_bounds__(256, 2) __global__
void window_block_attn_bf16_kernel(const __hip_bfloat16 *__restrict__ x,
                                   __hip_bfloat16 *__restrict__ y,
                                   __hip_bfloat16 *__restrict__ n2,
                                   const float *__restrict__ g1,
                                   const float *__restrict__ b1,
                                   const __hip_bfloat16 *__restrict__ wqkv_p,
                                   const float *__restrict__ bqkv,
                                   const float *__restrict__ rel,
                                   const __hip_bfloat16 *__restrict__ wp_p,
                                   const float *__restrict__ bp,
                                   const float *__restrict__ g2,
                                   const float *__restrict__ b2,
                                   WinBlockArgs a) {
  constexpr float LOG2E = 1.4426950408889634f;
  constexpr int HEADS = C / 32;
  constexpr int KS = C / 16;  // k steps over the width
  constexpr int NT = C / 32;  // 32-column tiles of the width
  constexpr int WQ = 3 * C * C, WP = C * C;
  constexpr int FRAG = 64 * 8;  // elements of one staged fragment
  // fp32 region: g1 | b1 | bqkv (3C) | bp | g2 | b2 | rel
  constexpr int O_B1 = C, O_BQ = 2 * C, O_BP = 5 * C, O_G2 = 6 * C,
                O_B2 = 7 * C, O_REL = 8 * C;
  __shared__ __align__(16) __bf16 wl[WQ + WP];
  __shared__ __align__(16) float fls[O_REL + HEADS * WB_REL_HEAD];

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid % WAVE;
  const int lq = lane % 32;    // the lane's token of a tile / weight row
  const int half = lane / 32;  // half-wave id

  // ---- stage: straight copies, the prepared layout is the LDS layout ----
  for (int p = tid; p < WQ / 8; p += 256)
    *(bf16x8 *)(wl + 8 * p) = *(const bf16x8 *)(wqkv_p + 8 * p);
  for (int p = tid; p < WP / 8; p += 256)
    *(bf16x8 *)(wl + WQ + 8 * p) = *(const bf16x8 *)(wp_p + 8 * p);
  for (int i = tid; i < C; i += 256) {
    fls[i] = g1[i];
    fls[O_B1 + i] = b1[i];
    fls[O_BP + i] = bp[i];
    fls[O_G2 + i] = g2[i];
    fls[O_B2 + i] = b2[i];
  }
  for (int i = tid; i < 3 * C; i += 256) fls[O_BQ + i] = bqkv[i];
  for (int i = tid; i < HEADS * WB_REL_HEAD; i += 256) {
    const int h = i / WB_REL_HEAD, r = (i % WB_REL_HEAD) / WB_REL_ROW,
              c = i % WB_REL_ROW;
    fls[O_REL + i] = c < 15 ? rel[(h * 15 + r) * 15 + c] * LOG2E : 0.0f;
  }
  wide_barrier();

  const float l2scale = a.scale * LOG2E;
  const float ninf = -__builtin_inff();
  const float inv_c = 1.0f / (float)C;

  for (int w = blockIdx.x * 4 + wid; w < a.nwin; w += gridDim.x * 4) {
    const int wx = w % a.nwx;
    const int wt = w / a.nwx;
    const int wy = wt % a.nwy;
    const int bb = wt / a.nwy;
    const int y0 = 8 * wy + a.shift, x0 = 8 * wx + a.shift;

    // The staged data never changes after the barrier, so the compiler would
    // hoist every LDS read out of the walk and hold weights, biases and rel
    // in registers (376 at C = 32, spills at C = 64). An offset it cannot
    // see through keeps the reads where they are used.
    int opaque = 0;
    asm volatile("" : "+v"(opaque));
    const float *fl = fls + opaque;
    const __bf16 *wfrag = wl + lane * 8 + opaque;  // + FRAG * (tile * KS + c)
    const __bf16 *pfrag = wfrag + WQ;
    // rel word of (qs, sub, g, e): relb[(4 (qs - sub) - g) * 16 - e]
    const float *relb = fl + O_REL + ((lq >> 3) + 7) * WB_REL_ROW + (lq & 7) -
                        4 * half + 7;

    // this lane's token of each 32-token tile: local (4 t + lq / 8, lq % 8)
    int xq = x0 + (lq & 7);
    xq = (xq >= a.W) ? xq - a.W : xq;
    long xo[2], yo[2], no[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      int yy = y0 + 4 * t + (lq >> 3);
      yy = (yy >= a.H) ? yy - a.H : yy;
      xo[t] = bb * a.xb + yy * a.xy + xq * a.xx + 8 * half;
      yo[t] = bb * a.yb + yy * a.yy + xq * a.yx + 8 * half;
      no[t] = bb * a.nb + yy * a.ny + xq * a.nx + 8 * half;
    }

    bf16x8 xr[2][KS];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int c = 0; c < KS; ++c)
        xr[t][c] = *(const bf16x8 *)(x + xo[t] + 16 * c);

    // ---- LN1 -> n1 fragments ----
    bf16x8 nf[2][KS];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float xf[KS][8];
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < KS; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          xf[c][j] = (float)xr[t][c][j];
          s += xf[c][j];
        }
      float mean;
      wb_stats(s, mean, lane, inv_c);
      float q = 0.f;
#pragma unroll
      for (int c = 0; c < KS; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = xf[c][j] - mean;
          q += d * d;
        }
      q += wide_shfl(q, lane ^ 32);
      const float rstd = __builtin_amdgcn_rsqf(q * inv_c + a.eps);
#pragma unroll
      for (int c = 0; c < KS; ++c) {
        const int k0 = 16 * c + 8 * half;
        const f32x4 ga = *(const f32x4 *)(fl + k0);
        const f32x4 gb = *(const f32x4 *)(fl + k0 + 4);
        const f32x4 ba = *(const f32x4 *)(fl + O_B1 + k0);
        const f32x4 bb4 = *(const f32x4 *)(fl + O_B1 + k0 + 4);
        unsigned pk[4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          pk[j] = pack_bf16(
              (xf[c][2 * j] - mean) * rstd * ga[2 * j] + ba[2 * j],
              (xf[c][2 * j + 1] - mean) * rstd * ga[2 * j + 1] + ba[2 * j + 1]);
          pk[2 + j] = pack_bf16(
              (xf[c][4 + 2 * j] - mean) * rstd * gb[2 * j] + bb4[2 * j],
              (xf[c][5 + 2 * j] - mean) * rstd * gb[2 * j + 1] +
                  bb4[2 * j + 1]);
        }
        nf[t][c] = *(bf16x8 *)pk;
      }
    }

    bf16x8 of[2][KS];  // [tile][16-channel step]: the proj GEMM's operand

    // the wrap straddles only the last window row / column
    const bool lastrow = a.shift > 0 && wy == a.nwy - 1;
    const bool lastcol = a.shift > 0 && wx == a.nwx - 1;
    const float coladd =
        (lastcol && (((lane & 4) != 0) != (half == 1))) ? ninf : 0.0f;

#pragma unroll
    for (int h = 0; h < HEADS; ++h) {
      // ---- q, k (swapped) and v (not swapped) of this head ----
      bf16x8 qk[2][2][2];  // [q | k][tile][16-channel step]
#pragma unroll
      for (int t3 = 0; t3 < 2; ++t3) {
        const int tile = t3 * HEADS + h;
        f32x16 pr[2];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 b4 =
              *(const f32x4 *)(fl + O_BQ + 32 * tile + 8 * g + 4 * half);
#pragma unroll
          for (int e = 0; e < 4; ++e) pr[0][4 * g + e] = pr[1][4 * g + e] = b4[e];
        }
#pragma unroll
        for (int c = 0; c < KS; ++c) {
          const bf16x8 wf = *(const bf16x8 *)(wfrag + FRAG * (tile * KS + c));
#pragma unroll
          for (int t = 0; t < 2; ++t)
            pr[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, nf[t][c], pr[t],
                                                            0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
          p_relayout(pr[t], qk[t3][t][0], qk[t3][t][1]);
      }
      bf16x8 vf[4];  // V fragments of keys kc*16 .. +16, all 32 channels
      {
        const int tile = 2 * HEADS + h;
        const float vb = fl[O_BQ + 32 * tile + lq];
        f32x16 pr[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) pr[0][r] = pr[1][r] = vb;
#pragma unroll
        for (int c = 0; c < KS; ++c) {
          const bf16x8 wf = *(const bf16x8 *)(wfrag + FRAG * (tile * KS + c));
#pragma unroll
          for (int t = 0; t < 2; ++t)
            pr[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(nf[t][c], wf, pr[t],
                                                            0, 0, 0);
        }
        p_relayout(pr[0], vf[0], vf[1]);
        p_relayout(pr[1], vf[2], vf[3]);
      }

      // ---- attention, the two 32-query halves one after the other ----
      const float *relh = relb + h * WB_REL_HEAD;
#pragma unroll
      for (int qs = 0; qs < 2; ++qs) {
        f32x16 s[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          s[sub] = (f32x16){};
#pragma unroll
          for (int c = 0; c < 2; ++c)
            s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                qk[1][sub][c], qk[0][qs][c], s[sub], 0, 0, 0);
        }
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              s[sub][4 * g + e] =
                  s[sub][4 * g + e] * l2scale +
                  relh[(4 * (qs - sub) - g) * WB_REL_ROW - e];
        if (lastrow || lastcol) {
#pragma unroll
          for (int sub = 0; sub < 2; ++sub) {
            const float add = (lastrow && sub != qs) ? ninf : coladd;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[sub][r] += add;
          }
        }
        float m = s[0][0];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r) m = fmaxf(m, s[sub][r]);
        m = fmaxf(m, wide_shfl(m, lane ^ 32));
        float l = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            s[sub][r] = __builtin_amdgcn_exp2f(s[sub][r] - m);
            l += s[sub][r];
          }
        l += wide_shfl(l, lane ^ 32);

        bf16x8 pa[4];
        p_relayout(s[0], pa[0], pa[1]);
        p_relayout(s[1], pa[2], pa[3]);
        f32x16 o = (f32x16){};
#pragma unroll
        for (int kc = 0; kc < 4; ++kc)
          o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[kc], pa[kc], o, 0, 0,
                                                      0);
        const float inv = 1.0f / l;  // l >= 1: the row's max contributes 1
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= inv;
        p_relayout(o, of[qs][2 * h], of[qs][2 * h + 1]);
        // one query half, and one head, at a time: interleaving them costs
        // more registers than the overlap is worth (C = 64 spilled)
        __builtin_amdgcn_sched_barrier(0);
      }

    }

    // ---- proj into accumulators that start as x + bp in fp32 ----
    f32x16 acc[2][NT];
    if constexpr (C == 64) {
      // 32 registers that would otherwise wait under the whole attention
      // (with them the instantiation spilled): the rows are read again, from
      // cache, 8 KB a window
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < KS; ++c)
          xr[t][c] = *(const volatile bf16x8 *)(x + xo[t] + 16 * c);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      // fragment layout (channel 16c + 8 half + j) -> accumulator layout
      // (register 4g + e is channel 32n + 8g + 4 half + e): values j = e and
      // j = 4 + e of fragment c = 2n + cc swap into g = 2cc and g = 2cc + 1
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
          const f32x4 p0 =
              *(const f32x4 *)(fl + O_BP + 32 * n + 16 * cc + 4 * half);
          const f32x4 p1 =
              *(const f32x4 *)(fl + O_BP + 32 * n + 16 * cc + 8 + 4 * half);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            auto r = __builtin_amdgcn_permlane32_swap(
                __builtin_bit_cast(unsigned, (float)xr[t][2 * n + cc][e]),
                __builtin_bit_cast(unsigned, (float)xr[t][2 * n + cc][4 + e]),
                false, false);
            acc[t][n][8 * cc + e] =
                __builtin_bit_cast(float, (unsigned)r[0]) + p0[e];
            acc[t][n][8 * cc + 4 + e] =
                __builtin_bit_cast(float, (unsigned)r[1]) + p1[e];
          }
        }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int c = 0; c < KS; ++c) {
        const bf16x8 wf = *(const bf16x8 *)(pfrag + FRAG * (n * KS + c));
#pragma unroll
        for (int t = 0; t < 2; ++t)
          acc[t][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              wf, of[t][c], acc[t][n], 0, 0, 0);
      }

    // ---- y and LN2(y) from the fp32 sum ----
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        bf16x8 o0, o1;
        p_relayout(acc[t][n], o0, o1);
        *(bf16x8 *)(y + yo[t] + 32 * n) = o0;
        *(bf16x8 *)(y + yo[t] + 32 * n + 16) = o1;
      }
      float s = 0.f;
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) s += acc[t][n][r];
      float mean;
      wb_stats(s, mean, lane, inv_c);
      float q = 0.f;
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float d = acc[t][n][r] - mean;
          q += d * d;
        }
      q += wide_shfl(q, lane ^ 32);
      const float rstd = __builtin_amdgcn_rsqf(q * inv_c + a.eps);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        f32x16 v;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int col = 32 * n + 8 * g + 4 * half;
          const f32x4 gm = *(const f32x4 *)(fl + O_G2 + col);
          const f32x4 bt = *(const f32x4 *)(fl + O_B2 + col);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[4 * g + e] = (acc[t][n][4 * g + e] - mean) * rstd * gm[e] + bt[e];
        }
        bf16x8 o0, o1;
        p_relayout(v, o0, o1);
        *(bf16x8 *)(n2 + no[t] + 32 * n) = o0;
        *(bf16x8 *)(n2 + no[t] + 32 * n + 16) = o1;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host-side dispatch (torch API lives in ext.hip which includes this file)
// ---------------------------------------------------------------------------
bool window_block_attn_supported_width(long c) { return c == 32 || c == 64; }

// {windows a wave walks, blocks}. A block is four waves and stages the
// weights once; up to WB_WAVES resident waves (256 CUs x 8) every wave takes
// one window, past that the walk grows and the staging is amortised over it.
constexpr long WB_WAVES = 2048;
std::tuple<long, long> window_block_attn_plan(long nwin, long c) {
  TORCH_CHECK(nwin >= 1, "window_block_attn: empty problem");
  TORCH_CHECK(window_block_attn_supported_width(c),
              "window_block_attn: width ", c, " is not 32 or 64");
  const long walk = (nwin + WB_WAVES - 1) / WB_WAVES;
  const long waves = (nwin + walk - 1) / walk;
  return {walk, (waves + 3) / 4};
}

#ifdef __HIP_PLATFORM_AMD__
// x, y, n2 [B, H, W, C] views; the caller checked everything an address is
// formed from
template <int C>
static void window_block_launch(const torch::Tensor &x, torch::Tensor &y,
                                torch::Tensor &n2, const torch::Tensor &g1,
                                const torch::Tensor &b1,
                                const torch::Tensor &wqkv_p,
                                const torch::Tensor &bqkv,
                                const torch::Tensor &rel,
                                const torch::Tensor &wp_p,
                                const torch::Tensor &bp,
                                const torch::Tensor &g2,
                                const torch::Tensor &b2, double scale,
                                long shift, double eps) {
  const long B = x.size(0), H = x.size(1), W = x.size(2);
  WinBlockArgs a;
  a.xb = x.stride(0), a.xy = x.stride(1), a.xx = x.stride(2);
  a.yb = y.stride(0), a.yy = y.stride(1), a.yx = y.stride(2);
  a.nb = n2.stride(0), a.ny = n2.stride(1), a.nx = n2.stride(2);
  a.H = (int)H;
  a.W = (int)W;
  a.nwy = (int)(H / 8);
  a.nwx = (int)(W / 8);
  a.nwin = (int)(B * (H / 8) * (W / 8));
  a.shift = (int)shift;
  a.scale = (float)scale;
  a.eps = (float)eps;
  const auto [walk, blocks] = window_block_attn_plan(a.nwin, C);
  (void)walk;
  hipLaunchKernelGGL(window_block_attn_bf16_kernel<C>, dim3((unsigned)blocks),
                     dim3(256), 0, cur_stream(),
                     (const __hip_bfloat16 *)x.data_ptr(),
                     (__hip_bfloat16 *)y.data_ptr(),
                     (__hip_bfloat16 *)n2.data_ptr(),
                     (const float *)g1.data_ptr(), (const float *)b1.data_ptr(),
                     (const __hip_bfloat16 *)wqkv_p.data_ptr(),
                     (const float *)bqkv.data_ptr(),
                     (const float *)rel.data_ptr(),
                     (const __hip_bfloat16 *)wp_p.data_ptr(),
                     (const float *)bp.data_ptr(), (const float *)g2.data_ptr(),
                     (const float *)b2.data_ptr(), a);
}
#endif
