// Flash-style fused attention forward for gfx950 (MFMA 32x32x16 bf16).
//
// Three kernels built from one set of pieces.
//
// Shared by all three (the helpers below, each written once):
//  * workgroup = 4 waves; each wave owns QS 32-row q-subtiles, the WG shares
//    K/V tiles of KVB = 64 keys staged in LDS (AttnGeom<DPAD>).
//  * swapped QK^T: S^T = mfma(K_frag, Q_frag) so each lane holds the scores
//    of ONE q-row (lane%32) across 16 of 32 keys (crow() names the row of
//    an accumulator register) — softmax is register-local plus one
//    __shfl_xor(32) to combine the half-wave pair. Q fragments are read once
//    (load_q_frags).
//  * P (bf16-packed) is redistributed to the PV A-fragment layout with
//    v_permlane32_swap pairs (guide T12, p_relayout), then PV accumulates
//    fp32 via MFMA.
//  * per-row factors (the online-softmax rescale, 1/l, w/l) live in the lane
//    that owns the row and reach accumulator register r by
//    __shfl(f, crow(r, half)).
//  * STRIDED access: Q/K/V/O are addressed with (batch, head, row) strides,
//    so both [B,H,S,D] and [B,S,H,D] layouts run with NO transpose or pad
//    copies; the head dim D only needs D % 8 == 0 (8-element groups beyond
//    D are masked in-kernel, DPAD = next multiple of 16).
//
// The kernels:
//  * flash_fwd_bf16_kernel ("v2"): K row-major and V transposed in LDS
//    (v2_stage), online softmax with per-tile rescale; the previous tile's
//    PV completes before the rescale decision (textbook order). The whole
//    per-tile compute is v2_tile_step.
//  * flash_blend_bf16_kernel: a context loop around v2's tile loop — the
//    same v2_stage and v2_tile_step, with its own QS and the context's key
//    count as the key bound.
//  * flash_fwd_bf16_v3: the same geometry with double-buffered row-major
//    tiles, hardware-transpose V reads, async staging and defer-max; it
//    shares the helpers, not the tile step. Its WIN flag is the windowed
//    addressing mode (attention inside the windows of a token grid).
//
// These kernels sit at the 256-VGPR edge, and how far a piece is shared is
// set by what keeps their register allocation (table and method in
// docs/kernels.md): a helper is optimised on its own before it is inlined,
// so one that owns an unrolled r loop hands the kernel 16 hoisted broadcast
// addresses or d-guards instead of a loop. That is why load_q_frags and
// store_row take one q-subtile / one register and the kernels keep those
// loops, why the per-row rescale loop is spelled out in v2_tile_step and
// in v3, and why v3 keeps its own epilogue.
//
// UNet shapes: D 40(->48), 80, 160; SDXL 64; VAE (D=512) takes the composed
// fallback path in ext.hip.
#include "common.h"

#include <type_traits>
#include <utility>

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  union {
    __hip_bfloat162 h2;
    unsigned u;
  } cvt;
  cvt.h2 = __hip_bfloat162(__float2bfloat16(lo), __float2bfloat16(hi));
  return cvt.u;
}

struct AttnStrides {
  long qb, qh, qr;  // batch, head, row strides (elements)
  long kb, kh, kr;
  long vb, vh, vr;
  long ob, oh, or_;
};

// Windowed self-attention (v3's WIN mode): the S = gh*gw tokens of a batch
// row are a gh x gw grid cut into nh x nw windows of th x tw tokens, and
// attention runs inside each window. In-window row r of window (i, j) is
// grid token ((i*th + r/tw) * gw + j*tw + r%tw), addressed with the row
// strides of AttnStrides: no rearranged copies of q, k, v or the output.
struct AttnWindow {
  int nh, nw;  // windows per grid column / row
  int th, tw;  // window size (tokens)
  int gw;      // grid width: tokens per grid row
};
// v3's strides argument: AttnStrides alone, plus the window when WIN. The
// WIN = false kernels keep the argument block (and the code) they had.
template <bool WIN>
struct AttnArgs : AttnStrides {};
template <>
struct AttnArgs<true> : AttnStrides {
  AttnWindow win;
};

// tile geometry of every kernel here, as functions of the padded head dim
template <int DPAD>
struct AttnGeom {
  static constexpr int KVB = 64;  // two 32-key S^T sub-tiles per staging phase
  static constexpr int PADK = 8;  // bf16 per-row pad: breaks ds_read_b128 conflicts
  static constexpr int NC = DPAD / 16;              // QK^T k-chunks
  static constexpr int DV = (DPAD + 31) / 32 * 32;  // PV d extent (32-col O tiles)
  static constexpr int ND = DV / 32;                // PV d-chunks (O accum tiles)
};

// 32-row q-subtiles per wave (a block is 4 waves: 128 * QS q rows). The
// kernels, the plan functions and the launchers' checks all read these.
constexpr int v2_qs(int) { return 2; }
constexpr int v3_qs(int dpad) { return dpad <= 96 ? 2 : 1; }
constexpr int blend_qs(int dpad) { return dpad <= 32 ? 2 : 1; }
constexpr int blend_min_blocks(int dpad) { return dpad <= 96 ? 2 : 1; }

// C layout of the 32x32 MFMA: the row that accumulator register r holds in
// half-wave `half` (the column is lane % 32)
__device__ __forceinline__ int crow(int r, int half) {
  return (r & 3) + 8 * (r >> 2) + 4 * half;
}

// Q fragments of one 32-row q-subtile, read once; qq is this lane's q row.
// B-frag of mfma(K,Q): lane holds Q[q=lq][d = c*16 + 8*half + i]. Rows past
// Sq re-read the last row (never stored); 8-groups beyond D are zero. FOLD
// (v3) multiplies by `fold` and rounds back to bf16 in the same pass.
template <bool FOLD, int NC>
__device__ __forceinline__ void load_q_frags(bf16x8 (&qf)[NC],
                                             const __hip_bfloat16 *Qb,
                                             long qr, long qq, long Sq, int D,
                                             int half, float fold = 1.0f) {
  const long qrow = (qq < Sq) ? qq : (Sq - 1);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d0 = c * 16 + 8 * half;
    bf16x8 qv = (bf16x8){};
    if (d0 + 8 <= D) {
      qv = *(const bf16x8 *)(Qb + qrow * qr + d0);
      if constexpr (FOLD) {
#pragma unroll
        for (int i = 0; i < 8; ++i) qv[i] = (__bf16)((float)qv[i] * fold);
      }
    }
    qf[c] = qv;
  }
}

// one S^T[32k, 32q] score sub-tile -> the two PV A-fragments (16 keys each)
__device__ __forceinline__ void p_relayout(const f32x16 &s, bf16x8 &pa0,
                                           bf16x8 &pa1) {
  unsigned pk[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) pk[t] = pack_bf16(s[2 * t], s[2 * t + 1]);
  auto r0 = __builtin_amdgcn_permlane32_swap(pk[0], pk[2], false, false);
  auto r1 = __builtin_amdgcn_permlane32_swap(pk[1], pk[3], false, false);
  unsigned frag[4] = {r0[0], r1[0], r0[1], r1[1]};
  pa0 = *(bf16x8 *)frag;
  auto r2 = __builtin_amdgcn_permlane32_swap(pk[4], pk[6], false, false);
  auto r3 = __builtin_amdgcn_permlane32_swap(pk[5], pk[7], false, false);
  unsigned frag1[4] = {r2[0], r3[0], r2[1], r3[1]};
  pa1 = *(bf16x8 *)frag1;
}

// epilogue (v2, blend) of register r of the q-subtile whose first row is
// qbase: o (times the row's f when SCALED) rounded to bf16, column-per-lane
// scatter (widen later, T21)
template <bool SCALED, int ND>
__device__ __forceinline__ void store_row(const f32x16 (&o)[ND], float f,
                                          int r, __hip_bfloat16 *Ob, long orow,
                                          long qbase, long Sq, int D, int lq,
                                          int half) {
  const int qrow = crow(r, half);
  float a = 1.0f;
  if constexpr (SCALED) a = __shfl(f, qrow, WAVE);
  const long qq = qbase + qrow;
  if (qq >= Sq) return;
#pragma unroll
  for (int d = 0; d < ND; ++d)
    if (d * 32 + lq < D)
      Ob[qq * orow + d * 32 + lq] = f2bf(SCALED ? o[d][r] * a : o[d][r]);
}

// ---------------------------------------------------------------------------
// v2 pieces: LDS tiles (K row-major padded, V transposed for contiguous
// B-fragment reads), the cooperative stage and the per-tile compute. The
// callers own the kv loop and its two block-uniform barriers per tile.
// ---------------------------------------------------------------------------
template <int DPAD>
using V2KTile = __bf16[AttnGeom<DPAD>::KVB][DPAD + AttnGeom<DPAD>::PADK];
template <int DPAD>
using V2VTile =
    __bf16[AttnGeom<DPAD>::DV][AttnGeom<DPAD>::KVB + AttnGeom<DPAD>::PADK];

// zero vt's pad rows once (D..DV); they are never re-staged
template <int DPAD>
__device__ __forceinline__ void v2_zero_vt_pad(V2VTile<DPAD> &vt, int D) {
  using G = AttnGeom<DPAD>;
  for (int idx = threadIdx.x + (D / 8) * 8 * (G::KVB + G::PADK);
       idx < G::DV * (G::KVB + G::PADK); idx += 256)
    ((__bf16 *)vt)[idx] = (__bf16)0.0f;
}

// cooperative K/V stage of keys [kv, kv + KVB): 256 threads, 8 bf16 each per
// step; keys at or past len and 8-groups beyond D are staged as zero
template <int DPAD>
__device__ __forceinline__ void v2_stage(V2KTile<DPAD> &kt, V2VTile<DPAD> &vt,
                                         const __hip_bfloat16 *Kb,
                                         const __hip_bfloat16 *Vb, long kr,
                                         long vr, long kv, long len, int D) {
  for (int idx = threadIdx.x; idx < AttnGeom<DPAD>::KVB * (DPAD / 8);
       idx += 256) {
    const int r = idx / (DPAD / 8);     // key row in tile
    const int c8 = idx % (DPAD / 8);    // 8-elem column group
    bf16x8 kvec = (bf16x8){};
    bf16x8 vvec = (bf16x8){};
    if (kv + r < len && c8 * 8 + 8 <= D) {
      kvec = *(const bf16x8 *)(Kb + (kv + r) * kr + c8 * 8);
      vvec = *(const bf16x8 *)(Vb + (kv + r) * vr + c8 * 8);
    }
    *(bf16x8 *)&kt[r][c8 * 8] = kvec;
#pragma unroll
    for (int j = 0; j < 8; ++j) vt[c8 * 8 + j][r] = vvec[j];
  }
}

// the staged tile against every q-subtile of the wave: two S^T[32k, 32q]
// k-sub-tiles, merged softmax, O rescale, PV. Keys at or past len are masked.
template <int DPAD, int QS>
__device__ __forceinline__ void v2_tile_step(
    const V2KTile<DPAD> &kt, const V2VTile<DPAD> &vt,
    const bf16x8 (&qf)[QS][AttnGeom<DPAD>::NC],
    f32x16 (&o)[QS][AttnGeom<DPAD>::ND], float (&m)[QS], float (&l)[QS],
    long kv, long len, float l2scale, int lq, int half) {
  using G = AttnGeom<DPAD>;
#pragma unroll
  for (int qs = 0; qs < QS; ++qs) {
    f32x16 stile[2] = {(f32x16){}, (f32x16){}};
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int c = 0; c < G::NC; ++c) {
        bf16x8 kf = *(const bf16x8 *)&kt[sub * 32 + lq][c * 16 + 8 * half];
        stile[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            kf, qf[qs][c], stile[sub], 0, 0, 0);
      }

    // softmax in base-2, in the accumulator registers: the fp32 scores
    // take scale*log2(e) once, after the MFMA (Q is not pre-scaled), so the
    // hot exponentials are bare v_exp2 with no per-element multiply
    float pmax = -1e30f;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = sub * 32 + crow(r, half);
        const float sv = (kv + kk < len) ? stile[sub][r] * l2scale : -1e30f;
        stile[sub][r] = sv;
        pmax = fmaxf(pmax, sv);
      }
    pmax = fmaxf(pmax, __shfl_xor(pmax, 32, WAVE));
    const float mnew = fmaxf(m[qs], pmax);
    const float alpha = __builtin_amdgcn_exp2f(m[qs] - mnew);
    float rowsum = 0.f;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        stile[sub][r] = __builtin_amdgcn_exp2f(stile[sub][r] - mnew);
        rowsum += stile[sub][r];
      }
    rowsum += __shfl_xor(rowsum, 32, WAVE);
    l[qs] = l[qs] * alpha + rowsum;
    m[qs] = mnew;

    // (not a helper shared with v3's deferred rescale: wrapping even the
    // broadcast moved v2<80> from 88 to 132 and v2<160> from 736 to 856
    // B/lane of scratch)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float a = __shfl(alpha, crow(r, half), WAVE);
#pragma unroll
      for (int d = 0; d < G::ND; ++d) o[qs][d][r] *= a;
    }

#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      bf16x8 pa0, pa1;
      p_relayout(stile[sub], pa0, pa1);
#pragma unroll
      for (int d = 0; d < G::ND; ++d) {
        bf16x8 v0 = *(const bf16x8 *)&vt[d * 32 + lq][sub * 32 + 8 * half];
        o[qs][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa0, v0, o[qs][d],
                                                           0, 0, 0);
        bf16x8 v1 =
            *(const bf16x8 *)&vt[d * 32 + lq][sub * 32 + 16 + 8 * half];
        o[qs][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa1, v1, o[qs][d],
                                                           0, 0, 0);
      }
    }
  }
}

template <int DPAD>
__launch_bounds__(256, 2) __global__ void flash_fwd_bf16_kernel(
    const __hip_bfloat16 *__restrict__ Q, const __hip_bfloat16 *__restrict__ K,
    const __hip_bfloat16 *__restrict__ V, __hip_bfloat16 *__restrict__ O,
    int H, long Sq, long Sk, int D, float scale, AttnStrides st) {
  using G = AttnGeom<DPAD>;
  constexpr int QS = v2_qs(DPAD);

  __shared__ __align__(16) V2KTile<DPAD> kt;
  __shared__ __align__(16) V2VTile<DPAD> vt;

  // (an XCD-grouping remap — one head's q-blocks pinned to one XCD for
  // K/V L2 reuse — measured -13% on the S=4096 shape: the concentrated
  // staging traffic beats the reuse. Plain mapping kept.)
  const int bh = blockIdx.y;
  const int qblk = blockIdx.x;
  const int bb = bh / H, hh = bh % H;
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int lq = lane % 32;   // q-row (softmax) / d-col (PV C) index
  const int half = lane / 32; // half-wave id
  const long q0 = (long)qblk * (QS * 128) + wid * (QS * 32);

  const __hip_bfloat16 *Qb = Q + bb * st.qb + hh * st.qh;
  const __hip_bfloat16 *Kb = K + bb * st.kb + hh * st.kh;
  const __hip_bfloat16 *Vb = V + bb * st.vb + hh * st.vh;
  __hip_bfloat16 *Ob = O + bb * st.ob + hh * st.oh;

  bf16x8 qf[QS][G::NC];
#pragma unroll
  for (int qs = 0; qs < QS; ++qs)
    load_q_frags<false>(qf[qs], Qb, st.qr, q0 + qs * 32 + lq, Sq, D, half);

  f32x16 o[QS][G::ND];
#pragma unroll
  for (int qs = 0; qs < QS; ++qs)
#pragma unroll
    for (int d = 0; d < G::ND; ++d) o[qs][d] = (f32x16){};
  float m[QS], l[QS];
#pragma unroll
  for (int qs = 0; qs < QS; ++qs) { m[qs] = -1e30f; l[qs] = 0.f; }

  v2_zero_vt_pad<DPAD>(vt, D);
  const float l2scale = scale * 1.4426950408889634f;

  for (long kv = 0; kv < Sk; kv += G::KVB) {
    __syncthreads();  // previous tile's LDS reads complete
    v2_stage<DPAD>(kt, vt, Kb, Vb, st.kr, st.vr, kv, Sk, D);
    __syncthreads();
    v2_tile_step<DPAD, QS>(kt, vt, qf, o, m, l, kv, Sk, l2scale, lq, half);
  }

  // epilogue: O /= l, store
#pragma unroll
  for (int qs = 0; qs < QS; ++qs) {
    const float linv = 1.0f / fmaxf(l[qs], 1e-30f);
#pragma unroll
    for (int r = 0; r < 16; ++r)
      store_row<true>(o[qs], linv, r, Ob, st.or_, q0 + qs * 32, Sq, D, lq,
                      half);
  }
}

// ---------------------------------------------------------------------------
// v3: same wave/tile geometry as v2 (4 waves x 64 q-rows, KVB=64 staged in
// LDS, swapped QK^T, in-register softmax, permlane P->A relayout) with the
// guide's attention-ladder levers applied:
//  * async-STAGE split (T14): next tile's K/V issued to registers BEFORE the
//    compute phase; only the LDS-write latency sits at the tile seam.
//  * scale folded into Q in log2 units: the hot loop's scores are already
//    scale*log2(e)*(q.k) so softmax is bare v_exp2 with no per-score mul.
//  * full-tile fast path: the (kv+kk<Sk) mask VALU only runs on the ragged
//    last tile; staged loads clamp rows/cols instead of branching per lane.
//  * defer-max (T13): the O/l rescale (16 shfl + 32 mul per q-subtile) is
//    skipped while the running max grows < 2^THR; P is bounded by 2^THR
//    which fp32 accumulation absorbs (THR=8 -> P<=256).
//  * s_setprio(1) brackets around the MFMA clusters (T5).
// ---------------------------------------------------------------------------
//
// WIN is the windowed addressing mode, a compile-time flag like the conv
// kernels' WRAP and add+LN's GATHER: blockIdx.y walks (batch, window, head),
// the launch passes Sq = Sk = th*tw, and every row index is an
// in-window row mapped to its grid token (AttnWindow). The tile loop stays
// division-free: each staged piece carries its x within the window row next
// to its pointer and advances by (64 / tw, 64 % tw) with one conditional
// carry; when tw divides 64 the carry never fires and the advance is the
// uniform delta again. Only the Q load, the clamped re-derivation on the
// ragged last tile and the epilogue divide (once per row). The arithmetic
// and the tile order are v3's, so a windowed call is bit-equal to v3 on
// materialised window copies.
template <int DPAD, int QS = v3_qs(DPAD), bool WIN = false>
__launch_bounds__(256, 2) __global__ void flash_fwd_bf16_v3(
    const __hip_bfloat16 *__restrict__ Q, const __hip_bfloat16 *__restrict__ K,
    const __hip_bfloat16 *__restrict__ V, __hip_bfloat16 *__restrict__ O,
    int H, long Sq, long Sk, int D, float scale, AttnArgs<WIN> st) {
  using G = AttnGeom<DPAD>;
  constexpr int KVB = G::KVB, PADK = G::PADK, NC = G::NC, DV = G::DV,
                ND = G::ND;
  // tr-read conflict pad: the residual ~6% SQ_LDS_BANK_CONFLICT is
  // tr-instruction-intrinsic (a +16 stride variant measured identical;
  // guide T10: addr swizzles don't move tr_read conflict classes)
  constexpr int PADV = (DV == 128) ? 24 : 8;
  constexpr int RSV = DV + PADV;              // vt2 row stride (elements)
  constexpr int NG = KVB * (DPAD / 8);        // bf16x8 pieces per operand
  constexpr int NST = 2 * NG / 256;           // pieces/thread (exact: 16*DPAD%256==0)
  constexpr float THR = 8.0f;                 // defer-max threshold (log2)
  // async register staging costs NST*8 VGPRs; at DPAD>=80 that spills,
  // so big head dims stage synchronously instead
  constexpr bool ASYNC = (DPAD <= 64);

  // BOTH K and V are staged row-major with pure vectorized writes: the PV
  // B-fragments come from ds_read_b64_tr_b16 hardware transpose reads
  // (mapping decoded by tools/tr16_probe.py: with addr(l) =
  // &vt2[k0 + ((l&15)>>2)][d0 + 4*(l&3)], lane l receives V[k0+j][d0+(l&15)]
  // for j=0..3). This removes the 8-scalar-LDS-write V transpose AND makes
  // the staging exactly NST pieces for EVERY thread (wave-balanced barriers;
  // the old 1.5-piece split parked half the waves at each barrier - the
  // round-1 PMC showed 52.6% SQ_WAIT_ANY at D=48).
  // double-buffered tiles: tile i+1 is written into buf i^1 while buf i
  // is computed, so ONE barrier per tile suffices (write(i) only needs
  // compute(i-2) complete, which the barrier of iteration i-1 guarantees)
  __shared__ __align__(16) __bf16 kt[2][KVB][DPAD + PADK];
  __shared__ __align__(16) __bf16 vt2[2][KVB][RSV];

  // WIN: blockIdx.y is (batch, window, head), head fastest
  const int bh = blockIdx.y;
  const int qblk = blockIdx.x;
  int bb = bh / H;
  const int hh = bh % H;
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int lq = lane % 32;
  const int half = lane / 32;
  const long q0 = (long)qblk * (QS * 128) + wid * (QS * 32);

  long w0 = 0;  // WIN: the window's first grid token
  if constexpr (WIN) {
    const int nwin = st.win.nh * st.win.nw;
    const int wi = bb % nwin;
    bb /= nwin;
    w0 = (long)(wi / st.win.nw) * st.win.th * st.win.gw +
         (long)(wi % st.win.nw) * st.win.tw;
  }
  const __hip_bfloat16 *Qb = Q + bb * st.qb + hh * st.qh;
  const __hip_bfloat16 *Kb = K + bb * st.kb + hh * st.kh;
  const __hip_bfloat16 *Vb = V + bb * st.vb + hh * st.vh;
  __hip_bfloat16 *Ob = O + bb * st.ob + hh * st.oh;
  if constexpr (WIN) {
    Qb += w0 * st.qr;
    Kb += w0 * st.kr;
    Vb += w0 * st.vr;
    Ob += w0 * st.or_;
  }
  // in-window row (already clamped below th*tw) -> grid token offset from
  // the window's first token; the identity without windows
  const auto grid_row = [&](long r) -> long {
    if constexpr (WIN) {
      const int y = (int)r / st.win.tw;
      return (long)y * st.win.gw + ((int)r - y * st.win.tw);
    } else {
      return r;
    }
  };

  // staged-piece coordinates: pieces [0,NG) are K rows, [NG,2NG) V rows;
  // NG is a multiple of 64 so the K/V split is wave-uniform and every
  // piece costs the same (one b128 write). Coordinates are recomputed on
  // the rare clamped paths instead of held live (VGPR budget).
  const auto piece = [&](int s, int &r, int &c, bool &v) {
    const int pc = threadIdx.x + s * 256;
    const int q = (pc < NG) ? pc : pc - NG;
    v = pc >= NG;
    r = q / (DPAD / 8);
    c = q % (DPAD / 8);
  };
  int eoff[NST];
#pragma unroll
  for (int s = 0; s < NST; ++s) {
    int r, c; bool v; piece(s, r, c, v);
    eoff[s] = v ? (r * RSV + c * 8) : (r * (DPAD + PADK) + c * 8);
  }
  // clamp the d-group so the ragged head dim never reads past a row
  const int dmax = D / 8 - 1;  // last full 8-group (D%8==0 guaranteed)

  // Q fragments with scale*log2(e) folded in (one extra bf16 rounding)
  const float l2scale = scale * 1.4426950408889634f;
  bf16x8 qf[QS][NC];
#pragma unroll
  for (int qs = 0; qs < QS; ++qs) {
    if constexpr (WIN) {
      // clamp in the window, then map: the helper's own clamp is a no-op
      const long qq = q0 + qs * 32 + lq;
      const long g = grid_row((qq < Sq) ? qq : (Sq - 1));
      load_q_frags<true>(qf[qs], Qb, st.qr, g, g + 1, D, half, l2scale);
    } else {
      load_q_frags<true>(qf[qs], Qb, st.qr, q0 + qs * 32 + lq, Sq, D, half,
                         l2scale);
    }
  }

  // per-lane tr-read base LDS byte address (probe-decoded mapping): the
  // per-read row/col deltas are added as small unsigned offsets
  const unsigned vbase =
      (unsigned)(unsigned long long)(const char *)&vt2[0][0][0] +
      ((((lane & 15) >> 2) + 8 * half) * RSV + 4 * (lane & 3) +
       ((lane >> 4) & 1) * 16) *
          2;

  f32x16 o[QS][ND];
#pragma unroll
  for (int qs = 0; qs < QS; ++qs)
#pragma unroll
    for (int d = 0; d < ND; ++d) o[qs][d] = (f32x16){};
  float m[QS], l[QS];
#pragma unroll
  for (int qs = 0; qs < QS; ++qs) { m[qs] = -1e30f; l[qs] = 0.f; }

  // per-thread running piece pointers: tile 0 clamped; full-tile advances
  // are one uniform-delta 64-bit add instead of strided re-derivation
  const __hip_bfloat16 *pp[NST];
  int px[WIN ? NST : 1];  // WIN: the piece's x within its window row
#pragma unroll
  for (int s = 0; s < NST; ++s) {
    int sr, sc; bool v; piece(s, sr, sc, v);
    const long r = (sr < Sk) ? sr : (Sk - 1);
    const int cg = (sc <= dmax) ? sc : dmax;
    const long g = grid_row(r);
    pp[s] = (v ? Vb + g * st.vr : Kb + g * st.kr) + cg * 8;
    if constexpr (WIN) px[s] = (int)r % st.win.tw;
  }
  // 64 rows on: (64 / tw) grid rows down and 64 % tw to the right, one more
  // grid row down and tw back when x passes the window's right edge
  int dx = 0;
  long rstep = KVB, rcarry = 0;
  if constexpr (WIN) {
    dx = KVB % st.win.tw;
    rstep = (long)(KVB / st.win.tw) * st.win.gw + dx;
    rcarry = st.win.gw - st.win.tw;
  }
  const long kdelta = rstep * st.kr, vdelta = rstep * st.vr;
  const long kcarry = rcarry * st.kr, vcarry = rcarry * st.vr;

  // prologue: issue tile 0's loads (clamped; OOB keys masked at score time)
  bf16x8 stg[ASYNC ? NST : 1];
  if constexpr (ASYNC) {
#pragma unroll
    for (int s = 0; s < NST; ++s) stg[s] = *(const bf16x8 *)pp[s];
  }

  int cur = 0;
  for (long kv = 0; kv < Sk; kv += KVB, cur ^= 1) {
    if constexpr (ASYNC) {
#pragma unroll
      for (int s = 0; s < NST; ++s) {
        const bool v = threadIdx.x + s * 256 >= NG;
        *(bf16x8 *)((v ? &vt2[cur][0][0] : &kt[cur][0][0]) + eoff[s]) =
            stg[s];
      }
    } else {
      // synchronous cooperative stage (VGPR-tight big head dims)
#pragma unroll
      for (int s = 0; s < NST; ++s) {
        const bool v = threadIdx.x + s * 256 >= NG;
        *(bf16x8 *)((v ? &vt2[cur][0][0] : &kt[cur][0][0]) + eoff[s]) =
            *(const bf16x8 *)pp[s];
      }
    }
    // piece pointers -> the next tile: a uniform advance while it is full,
    // the clamped re-derivation when it is the ragged last one
    if (kv + 2 * KVB <= Sk) {
#pragma unroll
      for (int s = 0; s < NST; ++s) {
        const bool v = threadIdx.x + s * 256 >= NG;
        pp[s] += v ? vdelta : kdelta;
        if constexpr (WIN) {
          px[s] += dx;
          if (px[s] >= st.win.tw) {
            px[s] -= st.win.tw;
            pp[s] += v ? vcarry : kcarry;
          }
        }
      }
    } else if (kv + KVB < Sk) {
      // (the next tile is the last: px is not read again)
#pragma unroll
      for (int s = 0; s < NST; ++s) {
        int sr, sc; bool v; piece(s, sr, sc, v);
        const long rr = kv + KVB + sr;
        const long r = grid_row((rr < Sk) ? rr : (Sk - 1));
        const int cg = (sc <= dmax) ? sc : dmax;
        pp[s] = (v ? Vb + r * st.vr : Kb + r * st.kr) + cg * 8;
      }
    }
    __syncthreads();
    // async-STAGE: issue the NEXT tile's loads now; they complete under
    // this tile's compute (the compiler places the vmcnt at first reuse)
    if constexpr (ASYNC) {
      if (kv + KVB < Sk) {
#pragma unroll
        for (int s = 0; s < NST; ++s) stg[s] = *(const bf16x8 *)pp[s];
      }
    }

    const bool fulltile = (kv + KVB <= Sk);
#pragma unroll
    for (int qs = 0; qs < QS; ++qs) {
      f32x16 stile[2] = {(f32x16){}, (f32x16){}};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          bf16x8 kf =
              *(const bf16x8 *)&kt[cur][sub * 32 + lq][c * 16 + 8 * half];
          stile[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              kf, qf[qs][c], stile[sub], 0, 0, 0);
        }
      __builtin_amdgcn_s_setprio(0);

      // softmax IN the accumulator registers (no p[] copy: VGPR budget)
      float pmax = -1e30f;
      if (fulltile) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            pmax = fmaxf(pmax, stile[sub][r]);
      } else {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kk = sub * 32 + crow(r, half);
            if (kv + kk >= Sk) stile[sub][r] = -1e30f;
            pmax = fmaxf(pmax, stile[sub][r]);
          }
      }
      pmax = fmaxf(pmax, __shfl_xor(pmax, 32, WAVE));

      // defer-max: rescale only when some row's max grew past THR
      if (!__all(pmax <= m[qs] + THR)) {
        const float mnew = fmaxf(m[qs], pmax);
        const float alpha = __builtin_amdgcn_exp2f(m[qs] - mnew);
        l[qs] *= alpha;
        m[qs] = mnew;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float a = __shfl(alpha, crow(r, half), WAVE);
#pragma unroll
          for (int d = 0; d < ND; ++d) o[qs][d][r] *= a;
        }
      }
      float rowsum = 0.f;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          stile[sub][r] = __builtin_amdgcn_exp2f(stile[sub][r] - m[qs]);
          rowsum += stile[sub][r];
        }
      rowsum += __shfl_xor(rowsum, 32, WAVE);
      l[qs] += rowsum;

#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        bf16x8 pa[2];
        p_relayout(stile[sub], pa[0], pa[1]);
        // PV with tr-read V fragments: per 16-key chunk, 2 transpose
        // reads per d-tile deliver V[k..k+7][dcol] straight from the
        // row-major tile (guide T10; mapping from tools/tr16_probe.py)
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
#pragma unroll
          for (int db = 0; db < ND; db += 2) {  // <=2 d-tiles per wait:
            constexpr int DB = 2;               // bounds tr live ranges
            unsigned long long tv[DB][2];
#pragma unroll
            for (int dd = 0; dd < DB; ++dd) {
              const int d = db + dd;
              if (d >= ND) break;
              const unsigned a0 =
                  vbase + (unsigned)(cur * (KVB * RSV * 2)) +
                  (unsigned)(((sub * 32 + kc * 16) * RSV + d * 32) * 2);
              asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
                           "ds_read_b64_tr_b16 %1, %3"
                           : "=&v"(tv[dd][0]), "=&v"(tv[dd][1])
                           : "v"(a0), "v"(a0 + (unsigned)(8 * RSV)));
            }
            // the wait NAMES the tr destinations (guide §5.7 form ii):
            // the consuming MFMAs then depend on it through registers, so
            // no sched_barrier wall is needed and independent work (the
            // other q-subtile's chain) may schedule into the LDS shadow
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(tv[0][0]), "+v"(tv[0][1]), "+v"(tv[1][0]),
                           "+v"(tv[1][1])
                         :
                         : "memory");
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int dd = 0; dd < DB; ++dd) {
              const int d = db + dd;
              if (d >= ND) break;
              union {
                unsigned long long u[2];
                bf16x8 v;
              } cv;
              cv.u[0] = tv[dd][0];
              cv.u[1] = tv[dd][1];
              o[qs][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                  pa[kc], cv.v, o[qs][d], 0, 0, 0);
            }
            __builtin_amdgcn_s_setprio(0);
          }
        }
      }
    }
  }

  // epilogue: store_row's sequence, spelled out. Through the helper the
  // d-guards leave the r loop and DPAD 80 and 96 spill 20 and 4 B/lane more
#pragma unroll
  for (int qs = 0; qs < QS; ++qs) {
    const float linv = 1.0f / fmaxf(l[qs], 1e-30f);
    // WIN: lane lq maps its own (clamped) row once; the grid token reaches
    // register r the way 1/l does
    int gmine = 0;
    if constexpr (WIN) {
      const long qm = q0 + qs * 32 + lq;
      gmine = (int)grid_row((qm < Sq) ? qm : (Sq - 1));
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float inv = __shfl(linv, crow(r, half), WAVE);
      long qq = q0 + qs * 32 + crow(r, half);
      int g = 0;
      if constexpr (WIN) g = __shfl(gmine, crow(r, half), WAVE);
      if (qq >= Sq) continue;
      if constexpr (WIN) qq = g;
#pragma unroll
      for (int d = 0; d < ND; ++d)
        if (d * 32 + lq < D)
          Ob[qq * st.or_ + d * 32 + lq] = f2bf(o[qs][d][r] * inv);
    }
  }
}

// ---------------------------------------------------------------------------
// multi-context blend: out[b,s,h,:] = sum_c W[b,c,s] * attn(q[b,s,h], K_c, V_c)
// with K_c/V_c = batch row kv_index[b*C + c] of K/V, kv_len[row] keys long.
// The v2 pieces (v2_stage, v2_tile_step: fp32 score scaling after the MFMA)
// with a context loop around the tile loop: Q fragments are read once; every
// context restarts m/l/o, walks its own tiles, and folds o * (w / l) into
// a second fp32 accumulator; the output is rounded to bf16 once, after the
// last context. The row and its length depend on (b, c) only, so every
// wave of the block walks every context and every tile and the barriers
// stay block-uniform. No zero-weight shortcut: every context is computed.
// Registers: o and acc are 2 * QS * ND * 16 fp32 next to NC * QS * 4 of Q
// fragments and 32 of scores. Two blocks per CU leave 256 registers a lane:
// QS=2 fits only at DPAD 32, QS=1 (128 q rows per block) up to DPAD 96.
// Beyond that they do not (at DPAD 192 o, acc, Q and the scores alone are
// 272), so DPAD >= 112 runs one block per CU with AGPRs. No instantiation uses
// scratch (checked with -Rpass-analysis=kernel-resource-usage; table in
// docs/kernels.md).
// ---------------------------------------------------------------------------
template <int DPAD, int QS = blend_qs(DPAD)>
__launch_bounds__(256, blend_min_blocks(DPAD)) __global__
void flash_blend_bf16_kernel(
    const __hip_bfloat16 *__restrict__ Q, const __hip_bfloat16 *__restrict__ K,
    const __hip_bfloat16 *__restrict__ V, __hip_bfloat16 *__restrict__ O,
    int H, long Sq, long Sk, int D, float scale, AttnStrides st, int C,
    int Bk, const int *__restrict__ kv_index, const int *__restrict__ kv_len,
    const float *__restrict__ W, long wb, long wc) {
  using G = AttnGeom<DPAD>;

  __shared__ __align__(16) V2KTile<DPAD> kt;
  __shared__ __align__(16) V2VTile<DPAD> vt;

  const int bh = blockIdx.y;
  const int qblk = blockIdx.x;
  const int bb = bh / H, hh = bh % H;
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int lq = lane % 32;
  const int half = lane / 32;
  const long q0 = (long)qblk * (QS * 128) + wid * (QS * 32);

  const __hip_bfloat16 *Qb = Q + bb * st.qb + hh * st.qh;
  __hip_bfloat16 *Ob = O + bb * st.ob + hh * st.oh;

  bf16x8 qf[QS][G::NC];
#pragma unroll
  for (int qs = 0; qs < QS; ++qs)
    load_q_frags<false>(qf[qs], Qb, st.qr, q0 + qs * 32 + lq, Sq, D, half);

  f32x16 acc[QS][G::ND];
#pragma unroll
  for (int qs = 0; qs < QS; ++qs)
#pragma unroll
    for (int d = 0; d < G::ND; ++d) acc[qs][d] = (f32x16){};

  v2_zero_vt_pad<DPAD>(vt, D);
  const float l2scale = scale * 1.4426950408889634f;

  for (int cx = 0; cx < C; ++cx) {
    // block-uniform: the K/V row of (b, context) and its key count. The
    // wrapper validates host tables; the clamps keep a bad device table
    // inside the K/V allocation
    int row = kv_index[bb * C + cx];
    row = row < 0 ? 0 : (row >= Bk ? Bk - 1 : row);
    long len = kv_len ? (long)kv_len[row] : Sk;
    len = len < 0 ? 0 : (len > Sk ? Sk : len);
    const __hip_bfloat16 *Kb = K + row * st.kb + hh * st.kh;
    const __hip_bfloat16 *Vb = V + row * st.vb + hh * st.vh;

    f32x16 o[QS][G::ND];
#pragma unroll
    for (int qs = 0; qs < QS; ++qs)
#pragma unroll
      for (int d = 0; d < G::ND; ++d) o[qs][d] = (f32x16){};
    float m[QS], l[QS];
#pragma unroll
    for (int qs = 0; qs < QS; ++qs) { m[qs] = -1e30f; l[qs] = 0.f; }

    for (long kv = 0; kv < len; kv += G::KVB) {
      __syncthreads();  // previous tile's (or context's) LDS reads complete
      v2_stage<DPAD>(kt, vt, Kb, Vb, st.kr, st.vr, kv, len, D);
      __syncthreads();
      v2_tile_step<DPAD, QS>(kt, vt, qf, o, m, l, kv, len, l2scale, lq, half);
    }

    // fold this context in: acc += o * (w / l). Lane lq holds its own
    // row's l and loads its own row's weight; the per-row lane broadcast
    // is row_factor's
#pragma unroll
    for (int qs = 0; qs < QS; ++qs) {
      const long qq = q0 + qs * 32 + lq;
      const float wv = (qq < Sq) ? W[bb * wb + cx * wc + qq] : 0.f;
      const float wl = wv / fmaxf(l[qs], 1e-30f);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float f = __shfl(wl, crow(r, half), WAVE);
#pragma unroll
        for (int d = 0; d < G::ND; ++d) acc[qs][d][r] += o[qs][d][r] * f;
      }
    }
  }

  // one bf16 rounding of the blended row
#pragma unroll
  for (int qs = 0; qs < QS; ++qs)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      store_row<false>(acc[qs], 1.0f, r, Ob, st.or_, q0 + qs * 32, Sq, D, lq,
                       half);
}

// ---------------------------------------------------------------------------
// host-side dispatch (torch API lives in ext.hip which includes this file)
// ---------------------------------------------------------------------------
bool flash_supported(long d_head) {
  return d_head > 16 && d_head <= 192 && (d_head % 8) == 0;
}

#ifdef __HIP_PLATFORM_AMD__
static inline long round16(long d) { return (d + 15) / 16 * 16; }

// Calls f(std::integral_constant<int, DP>) for the instantiated padded head
// dim DP equal to dpad; any other dpad is an error.
template <class F, int... DP>
static void dispatch_dpad_in(long dpad, const char *who, F &&f,
                             std::integer_sequence<int, DP...>) {
  const bool found =
      ((dpad == DP ? (f(std::integral_constant<int, DP>{}), true) : false) ||
       ...);
  TORCH_CHECK(found, who, ": unsupported padded head dim ", dpad);
}
template <class F>
static void dispatch_dpad(long dpad, const char *who, F &&f) {
  dispatch_dpad_in(dpad, who, f,
                   std::integer_sequence<int, 32, 48, 64, 80, 96, 112, 128,
                                         144, 160, 176, 192>{});
}

// q/k/v/out: "bhsd" ([B,H,S,D]) or "bshd" ([B,S,H,D]) views
static AttnStrides attn_strides(const torch::Tensor &q, const torch::Tensor &k,
                                const torch::Tensor &v,
                                const torch::Tensor &out, bool bshd) {
  const int h = bshd ? 2 : 1, r = bshd ? 1 : 2;
  AttnStrides st;
  st.qb = q.stride(0); st.qh = q.stride(h); st.qr = q.stride(r);
  st.kb = k.stride(0); st.kh = k.stride(h); st.kr = k.stride(r);
  st.vb = v.stride(0); st.vh = v.stride(h); st.vr = v.stride(r);
  st.ob = out.stride(0); st.oh = out.stride(h); st.or_ = out.stride(r);
  return st;
}

// Which kernel serves an attention call: {"v2" | "v3" | "composed", padded
// head dim, q rows per workgroup}. "composed" is the GEMM + row_softmax_
// path of attention_fwd (head dims the flash kernels do not take); its
// other two fields are 0. force: 0 = measured policy, 2 = v2, 3 = v3 (A/B
// tooling and tests); a forced flash kernel on an unsupported head dim is
// an error, never a silent composition. The launcher below follows this
// and nothing else decides.
std::tuple<std::string, long, long> attention_plan(long d_head, long sk,
                                                   long force) {
  TORCH_CHECK(force == 0 || force == 2 || force == 3,
              "attention: force must be 0 (auto), 2 (v2) or 3 (v3)");
  if (!flash_supported(d_head)) {
    TORCH_CHECK(force == 0, "attention: head dim ", d_head,
                " has no flash kernel; variant v", force,
                " cannot be forced");
    return {"composed", 0, 0};
  }
  const long dpad = round16(d_head);
  // measured dispatch: v3 wins every self-attention shape (at D>64 its
  // prologue/epilogue spills are off the hot loop: +24% at D=80, +7% at
  // D=160); the short-Sk cross shapes (Sk=77) stay on v2
  const bool v2 = force == 2 || (force == 0 && dpad > 64 && sk < 256);
  if (v2) return {"v2", dpad, 128 * v2_qs((int)dpad)};
  return {"v3", dpad, 128 * v3_qs((int)dpad)};
}

// qkv layout: "bhsd" (q.size = [B,H,S,D]) or "bshd" ([B,S,H,D]); tensors
// need unit stride in D and 16-byte-aligned row starts, NOT full contiguity.
static torch::Tensor flash_attention_raw(torch::Tensor q, torch::Tensor k,
                                         torch::Tensor v, double scale,
                                         bool bshd, long force) {
  const long B = q.size(0);
  const long H = bshd ? q.size(2) : q.size(1);
  const long Sq = bshd ? q.size(1) : q.size(2);
  const long Sk = bshd ? k.size(1) : k.size(2);
  const long D = q.size(3);
  TORCH_CHECK(q.stride(3) == 1 && k.stride(3) == 1 && v.stride(3) == 1,
              "flash: D must be unit-stride");
  auto out = bshd ? torch::empty({B, Sq, H, D}, q.options())
                  : torch::empty({B, H, Sq, D}, q.options());
  const AttnStrides st = attn_strides(q, k, v, out, bshd);
  const dim3 block(256);
  auto stream = cur_stream();
  // the plan decides v2 vs v3 and the block's q-row extent; nothing else
  const auto [kernel, dpad, qrows] = attention_plan(D, Sk, force);
  TORCH_CHECK(dpad == round16(D),
              "flash: plan/launch padded head dim mismatch");
  const bool run_v2 = kernel == "v2";
  const long rows = qrows;  // (a structured binding cannot be captured)
  const dim3 grid((unsigned)((Sq + rows - 1) / rows), (unsigned)(B * H));

  dispatch_dpad(dpad, "flash", [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    TORCH_CHECK(rows == 128 * (run_v2 ? v2_qs(DP) : v3_qs(DP)),
                "flash: plan rows do not match the instantiation");
    const auto launch = [&](auto kernel, auto args) {
      hipLaunchKernelGGL(kernel, grid, block, 0, stream,
                         (const __hip_bfloat16 *)q.data_ptr(),
                         (const __hip_bfloat16 *)k.data_ptr(),
                         (const __hip_bfloat16 *)v.data_ptr(),
                         (__hip_bfloat16 *)out.data_ptr(), (int)H, Sq, Sk,
                         (int)D, (float)scale, args);
    };
    if (run_v2) launch(flash_fwd_bf16_kernel<DP>, st);
    else launch(flash_fwd_bf16_v3<DP>, AttnArgs<false>{st});
  });
  return out;
}

// The windowed kernel's geometry: {padded head dim, q rows per workgroup}.
// Windowed calls always run v3 (WIN = true), whatever the window's token
// count; a head dim without a flash kernel is an error. The launcher below
// follows this and nothing else decides.
std::tuple<long, long> attention_window_plan(long d_head) {
  TORCH_CHECK(flash_supported(d_head), "attention_window: head dim ", d_head,
              " has no flash kernel");
  const long dpad = round16(d_head);
  return {dpad, 128 * v3_qs((int)dpad)};
}

// q/k/v [B, gh*gw, H, D] (unit stride in D, 16-byte-aligned rows; the caller
// checked shapes, alignment and that th | gh, tw | gw): attention inside each
// th x tw window of the gh x gw token grid, output in the original order.
static torch::Tensor flash_window_raw(torch::Tensor q, torch::Tensor k,
                                      torch::Tensor v, double scale, long gh,
                                      long gw, long th, long tw) {
  const long B = q.size(0), S = q.size(1), H = q.size(2), D = q.size(3);
  auto out = torch::empty({B, S, H, D}, q.options());
  AttnArgs<true> args{attn_strides(q, k, v, out, /*bshd=*/true),
                      AttnWindow{(int)(gh / th), (int)(gw / tw), (int)th,
                                 (int)tw, (int)gw}};
  const auto [dpad, qrows] = attention_window_plan(D);
  const long rows = qrows;  // (a structured binding cannot be captured)
  const long wtok = th * tw, nblk_y = B * (gh / th) * (gw / tw) * H;
  TORCH_CHECK(nblk_y <= 65535, "attention_window: batch * windows * heads = ",
              nblk_y, " exceeds the grid's y extent (65535)");
  const dim3 grid((unsigned)((wtok + rows - 1) / rows), (unsigned)nblk_y);
  const dim3 block(256);
  auto stream = cur_stream();

  dispatch_dpad(dpad, "flash_window", [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    TORCH_CHECK(rows == 128 * v3_qs(DP),
                "flash_window: plan rows do not match the instantiation");
    hipLaunchKernelGGL((flash_fwd_bf16_v3<DP, v3_qs(DP), true>), grid, block,
                       0, stream, (const __hip_bfloat16 *)q.data_ptr(),
                       (const __hip_bfloat16 *)k.data_ptr(),
                       (const __hip_bfloat16 *)v.data_ptr(),
                       (__hip_bfloat16 *)out.data_ptr(), (int)H, wtok, wtok,
                       (int)D, (float)scale, args);
  });
  return out;
}

// The multi-context blend kernel's geometry: {padded head dim, q rows per
// workgroup}. One kernel family serves every supported head dim; a head
// dim without a flash kernel is an error (the blend is never composed).
// The launcher below follows this and nothing else decides.
std::tuple<long, long> attention_blend_plan(long d_head) {
  TORCH_CHECK(flash_supported(d_head), "attention_blend: head dim ", d_head,
              " has no flash kernel");
  const long dpad = round16(d_head);
  return {dpad, 128 * blend_qs((int)dpad)};
}

// q [B,Sq,H,D], k/v [Bk,Sk,H,D] (unit stride in D, 16-byte-aligned rows),
// w fp32 [B or 1, C, Sq] unit-stride in s, kv_index int32 [B*C] and kv_len
// int32 [Bk] (or undefined) on the device.
static torch::Tensor flash_blend_raw(torch::Tensor q, torch::Tensor k,
                                     torch::Tensor v, torch::Tensor w,
                                     torch::Tensor kv_index,
                                     c10::optional<torch::Tensor> kv_len,
                                     double scale) {
  const long B = q.size(0), Sq = q.size(1), H = q.size(2), D = q.size(3);
  const long Bk = k.size(0), Sk = k.size(1);
  const long C = w.size(1);
  auto out = torch::empty({B, Sq, H, D}, q.options());
  const AttnStrides st = attn_strides(q, k, v, out, /*bshd=*/true);
  const long wb = w.size(0) == 1 ? 0 : w.stride(0), wc = w.stride(1);
  const auto [dpad, qrows] = attention_blend_plan(D);
  const long rows = qrows;  // (a structured binding cannot be captured)
  const dim3 grid((unsigned)((Sq + rows - 1) / rows), (unsigned)(B * H));
  const dim3 block(256);
  auto stream = cur_stream();
  const int *len_ptr =
      kv_len.has_value() ? kv_len->data_ptr<int>() : (const int *)nullptr;

  dispatch_dpad(dpad, "flash_blend", [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    TORCH_CHECK(rows == 128 * blend_qs(DP),
                "flash_blend: plan rows do not match the instantiation");
    hipLaunchKernelGGL(flash_blend_bf16_kernel<DP>, grid, block, 0, stream,
                       (const __hip_bfloat16 *)q.data_ptr(),
                       (const __hip_bfloat16 *)k.data_ptr(),
                       (const __hip_bfloat16 *)v.data_ptr(),
                       (__hip_bfloat16 *)out.data_ptr(), (int)H, Sq, Sk,
                       (int)D, (float)scale, st, (int)C, (int)Bk,
                       kv_index.data_ptr<int>(), len_ptr,
                       w.data_ptr<float>(), wb, wc);
  });
  return out;
}

#endif
