// HAT attention on gfx950: 16 x 16 query windows against a KW x KW key patch
// with a relative-position bias. KW = 16 is the (shifted-)window
// self-attention of a HAB, KW = 24 the overlapping cross-attention of an OCAB
// (the 24 x 24 patch centred on the window, zero keys outside the grid). The
// fragment helpers, tr_v_frag, wide_shfl, wide_barrier and the kernel
// attribute are common.h's, shared with the other attention kernels.
//
// The problem per (window, head) is 256 queries x 256 / 576 keys x 32
// channels. Neither the scores of a query nor the gathered bias
// ([256, KW^2] fp32 a head, 256 / 576 KB) fit anywhere near the registers
// attention_swin.hip keeps them in, so the split is a different one:
//
//  * work split: one block of four waves per (window, head); blockIdx.x is
//    the window of B * H/16 * W/16, blockIdx.y the head. Wave g owns query
//    rows 4g .. 4g+3 of the window, 64 queries, as two 32-query halves qs
//    (rows 4g + 2qs, 4g + 2qs + 1). Lane l holds query lq = l % 32 of each
//    half: local (4g + 2qs + lq / 16, lq % 16). No launch walk: a 256 x 256
//    token grid is 1536 blocks at 6 heads, six to a CU.
//  * addressing: qkv is the [B, H, W, 3, heads, 32] view of the QKV GEMM's
//    output, read at its strides. Window (wy, wx), local query (i, j) is grid
//    token ((16 wy + i + shift) mod H, (16 wx + j + shift) mod W) and its
//    output row is written at that token of a contiguous [B, H, W, heads*32]
//    tensor. Key (ky, kx) of the patch is grid token (16 wy + shift - PAD +
//    ky, ...), PAD = (KW - 16) / 2: wrapped at KW 16, out of the grid at
//    KW 24 (shift is 0 there). No roll, partition, unfold, score, mask or
//    reverse tensor exists.
//  * LDS, one object: K tile | V tile | bias offsets. K and V rows are 32
//    bf16 at a row stride of 40 (80 B, 5 16-byte slots: the 16-byte fragment
//    reads of 32 consecutive rows spread over all banks), row = ky * KW + kx
//    of the phase. The block stages them once and the four waves share them.
//    Static LDS ends at 64 KB and the whole 24 x 24 patch would be 92 KB (one
//    block a CU), so KW 24 runs two phases of 12 key rows (46,080 B of K and
//    V + 6,084 B of bias), with a barrier pair between them; KW 16 is one
//    phase of 16 rows (40,960 + 3,844 B). Either fits three blocks a CU;
//    the registers (166 / 231 VGPRs, no scratch) allow three and two, and
//    the other blocks' tiles cover a block's staging. Out-of-grid
//    keys are staged as zero rows: their score is the bias alone, they add
//    exp(bias) to the denominator and nothing to the numerator.
//  * bias: bias_off [heads, R, R] fp32, R = KW + 15, entry
//    [ky - qy + 15][kx - qx + 15], is staged into LDS in log2 units for the
//    block's lifetime. A key tile is four whole key rows (64 keys at KW 16,
//    96 = three 32-key MFMA blocks at KW 24), so accumulator register r of
//    block sub is key n = 32 sub + (r & 3) + 8 (r >> 2) + 4 half of the tile,
//    (n / KW, n % KW) with n / KW the same in both half-waves: a lookup is one
//    ds_read_b32 at a compile-time offset from a lane pointer that advances
//    4 R a tile.
//  * QK^T: swapped, S^T = mfma(K_frag, Q_frag), 32x32x16 bf16, K fragments
//    16-byte LDS reads, Q fragments 16-byte global loads held for the whole
//    block. s = acc * (scale log2 e) + bias in fp32.
//  * shift mask (KW 16, shift 8): only windows of the last window row /
//    column straddle the wrap. The row region changes between local rows 7
//    and 8: a property of (wave, tile), so a whole tile is masked or not.
//    The column region changes between columns 7 and 8: bit 3 of lq for the
//    query and bit 2 of r for the key, so two lane constants cover it.
//  * softmax: online over the tiles. Max over the lane's 32 / 48 scores and
//    one exchange with lane ^ 32; the row sum stays a per-lane partial of the
//    unrounded fp32 P (both half-waves rescale it by the same factor) and is
//    exchanged once at the end. P is rounded to bf16 once, as the PV operand.
//  * PV: swapped as well, O^T = mfma(V_frag, P_frag) with V fragments by
//    ds_read_b64_tr_b16: a lane holds the channels of ITS query, so 1/l is a
//    lane constant and p_relayout turns the tile into two 16-byte stores.
//  * no atomics; every output element is written once by one lane.

#include "common.h"

struct HatArgs {
  long sb, sy, sx, s3, sh;  // qkv strides (elements): batch, row, col, q/k/v, head
  int H, W;                 // token grid
  int nwy, nwx;             // windows per grid column / row
  int heads;
  int shift;                // 0 or 8 (0 at KW 24)
  float scale;
};

constexpr int HAT_RS = 40;  // K / V tile row stride (bf16): 80 B

template <int KW>
WIDE_KERNEL_ATTR __launch_bounds__(256, 2) __global__
void hat_attn_bf16_kernel(const __hip_bfloat16 *__restrict__ qkv,
                          const float *__restrict__ bias_off,
                          __hip_bfloat16 *__restrict__ out, HatArgs a) {
  constexpr float LOG2E = 1.4426950408889634f;
  constexpr int R = KW + 15;              // bias offsets per axis
  constexpr int PR = KW == 24 ? 12 : 16;  // key rows of a phase
  constexpr int NPH = KW / PR;            // phases
  constexpr int PKEYS = PR * KW;          // keys of a phase: 256 / 288
  constexpr int TK = 4 * KW;              // keys of a tile: 64 / 96
  constexpr int NSUB = TK / 32;           // 32-key MFMA blocks of a tile
  constexpr int NT = PR / 4;              // tiles of a phase
  constexpr int PAD = (KW - 16) / 2;      // patch overhang per side
  constexpr int NPIECE = PKEYS * 4;       // 16-byte pieces of a K (V) phase
  constexpr int NIT = (NPIECE + 255) / 256;
  __shared__ __align__(16) __bf16 smem[2 * PKEYS * HAT_RS + 2 * R * R];
  __bf16 *kt = smem;
  __bf16 *vt = smem + PKEYS * HAT_RS;
  float *bo = (float *)(smem + 2 * PKEYS * HAT_RS);

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid % WAVE;
  const int lq = lane % 32;    // query (scores, O^T column) / key (K fragment)
  const int half = lane / 32;  // half-wave id
  const int head = blockIdx.y;
  const int wx = blockIdx.x % a.nwx;
  const int wt = blockIdx.x / a.nwx;
  const int wy = wt % a.nwy;
  const int bb = wt / a.nwy;
  const __hip_bfloat16 *base = qkv + bb * a.sb + head * a.sh;

  for (int i = tid; i < R * R; i += 256)
    bo[i] = bias_off[(long)head * (R * R) + i] * LOG2E;

  // the lane's query of each half, its Q fragments and its output row
  const int qx = lq & 15;
  const int qy0 = 4 * wid + (lq >> 4);  // of half 0; half 1 is two rows down
  long otok[2];
  bf16x8 qf[2][2];
  {
    int xq = 16 * wx + a.shift + qx;
    xq = (xq >= a.W) ? xq - a.W : xq;
#pragma unroll
    for (int qs = 0; qs < 2; ++qs) {
      int y = 16 * wy + a.shift + qy0 + 2 * qs;
      y = (y >= a.H) ? y - a.H : y;
      const __hip_bfloat16 *qp = base + y * a.sy + xq * a.sx + 8 * half;
      qf[qs][0] = *(const bf16x8 *)qp;
      qf[qs][1] = *(const bf16x8 *)(qp + 16);
      otok[qs] = (((long)bb * a.H + y) * a.W + xq) * ((long)a.heads * 32) +
                 head * 32 + 8 * half;
    }
  }
  // bias of key (ky, kx) for the query of half qs: bq[(ky - 2 qs) * R + kx]
  const float *bq = bo + (15 - qy0) * R + 15 - qx + 4 * half;
  const __bf16 *klane = kt + lq * HAT_RS + 8 * half;
  const __bf16 *vlane = vt + (((lane & 15) >> 2) + 8 * half) * HAT_RS +
                        4 * (lane & 3) + ((lane >> 4) & 1) * 16;

  const float l2scale = a.scale * LOG2E;
  const float neg = -100.0f * LOG2E;
  const bool lastrow = KW == 16 && a.shift > 0 && wy == a.nwy - 1;
  const bool lastcol = KW == 16 && a.shift > 0 && wx == a.nwx - 1;
  // keys of columns 0..7 (8..15) lie across the wrap from queries of 8..15
  // (0..7)
  const float cadd[2] = {(lastcol && qx >= 8) ? neg : 0.0f,
                         (lastcol && qx < 8) ? neg : 0.0f};

  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
  f32x16 o[2] = {(f32x16){}, (f32x16){}};

#pragma unroll 1
  for (int ph = 0; ph < NPH; ++ph) {
    if (ph > 0) wide_barrier();  // every wave is done with the last phase
    {
      bf16x8 kp[NIT], vp[NIT];
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int p = it * 256 + tid;
        const int row = p >> 2;
        int y = 16 * wy + a.shift - PAD + ph * PR + row / KW;
        int x = 16 * wx + a.shift - PAD + row % KW;
        bool ok = NPIECE % 256 == 0 || p < NPIECE;
        if (KW == 16) {
          y = (y >= a.H) ? y - a.H : y;
          x = (x >= a.W) ? x - a.W : x;
        } else {
          ok = ok && y >= 0 && y < a.H && x >= 0 && x < a.W;
        }
        kp[it] = (bf16x8){};
        vp[it] = (bf16x8){};
        if (ok) {
          const __hip_bfloat16 *src = base + y * a.sy + x * a.sx + (p & 3) * 8;
          kp[it] = *(const bf16x8 *)(src + a.s3);
          vp[it] = *(const bf16x8 *)(src + 2 * a.s3);
        }
      }
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int p = it * 256 + tid;
        if (NPIECE % 256 == 0 || p < NPIECE) {
          const int at = (p >> 2) * HAT_RS + (p & 3) * 8;
          *(bf16x8 *)(kt + at) = kp[it];
          *(bf16x8 *)(vt + at) = vp[it];
        }
      }
    }
    wide_barrier();

#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
      const int ky0 = ph * PR + 4 * t;  // first key row of the tile
      bf16x8 kf[NSUB][2];
#pragma unroll
      for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
        for (int c = 0; c < 2; ++c)
          kf[sub][c] = *(const bf16x8 *)(klane + (t * TK + sub * 32) * HAT_RS +
                                         c * 16);
      bf16x8 vf[2 * NSUB];
#pragma unroll
      for (int kc = 0; kc < 2 * NSUB; ++kc)
        vf[kc] = tr_v_frag<HAT_RS>(vlane + (t * TK + kc * 16) * HAT_RS);
      const float *bt = bq + ky0 * R;
      const bool rowmask = lastrow && ((wid >= 2) != (ky0 >= 8));

#pragma unroll
      for (int qs = 0; qs < 2; ++qs) {
        f32x16 s[NSUB];
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
          s[sub] = (f32x16){};
#pragma unroll
          for (int c = 0; c < 2; ++c)
            s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                kf[sub][c], qf[qs][c], s[sub], 0, 0, 0);
        }
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int n = sub * 32 + (r & 3) + 8 * (r >> 2);  // + 4 half
            s[sub][r] = s[sub][r] * l2scale +
                        bt[(n / KW - 2 * qs) * R + n % KW];
          }
        if (KW == 16 && (lastrow || lastcol)) {
#pragma unroll
          for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r)
              s[sub][r] += rowmask ? neg : cadd[(r >> 2) & 1];
        }
        float mt = s[0][0];
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[sub][r]);
        mt = fmaxf(mt, wide_shfl(mt, lane ^ 32));
        const float mn = fmaxf(m[qs], mt);
        const float alpha = __builtin_amdgcn_exp2f(m[qs] - mn);
        m[qs] = mn;
        float lt = 0.f;
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            s[sub][r] = __builtin_amdgcn_exp2f(s[sub][r] - mn);
            lt += s[sub][r];
          }
        l[qs] = l[qs] * alpha + lt;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[qs][r] *= alpha;

        // O^T[channel][query] += sum over 16-key chunks of mfma(V, P)
        bf16x8 pa[2 * NSUB];
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
          p_relayout(s[sub], pa[2 * sub], pa[2 * sub + 1]);
#pragma unroll
        for (int kc = 0; kc < 2 * NSUB; ++kc)
          o[qs] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[kc], pa[kc],
                                                          o[qs], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int qs = 0; qs < 2; ++qs) {
    const float lsum = l[qs] + wide_shfl(l[qs], lane ^ 32);
    const float inv = 1.0f / lsum;  // lsum >= 1: the row's max contributes 1
#pragma unroll
    for (int r = 0; r < 16; ++r) o[qs][r] *= inv;
    bf16x8 o0, o1;  // channels 8*half..+8 and 16 + 8*half..+8 of the query
    p_relayout(o[qs], o0, o1);
    *(bf16x8 *)(out + otok[qs]) = o0;
    *(bf16x8 *)(out + otok[qs] + 16) = o1;
  }
}

// ---------------------------------------------------------------------------
// host-side dispatch (torch API lives in ext.hip which includes this file)
// ---------------------------------------------------------------------------
#ifdef __HIP_PLATFORM_AMD__
// qkv [B, H, W, 3, heads, 32] view, bias_off [heads, kw + 15, kw + 15]
// contiguous fp32 (the caller checked everything an address is formed from)
static torch::Tensor hat_attn_raw(torch::Tensor qkv, torch::Tensor bias_off,
                                  double scale, long shift, long kw) {
  const long B = qkv.size(0), H = qkv.size(1), W = qkv.size(2),
             heads = qkv.size(4);
  auto out = torch::empty({B, H, W, heads * 32}, qkv.options());
  HatArgs a;
  a.sb = qkv.stride(0);
  a.sy = qkv.stride(1);
  a.sx = qkv.stride(2);
  a.s3 = qkv.stride(3);
  a.sh = qkv.stride(4);
  a.H = (int)H;
  a.W = (int)W;
  a.nwy = (int)(H / 16);
  a.nwx = (int)(W / 16);
  a.heads = (int)heads;
  a.shift = (int)shift;
  a.scale = (float)scale;
  const dim3 grid((unsigned)(B * a.nwy * a.nwx), (unsigned)heads);
  auto kern = kw == 16 ? hat_attn_bf16_kernel<16> : hat_attn_bf16_kernel<24>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, cur_stream(),
                     (const __hip_bfloat16 *)qkv.data_ptr(),
                     (const float *)bias_off.data_ptr(),
                     (__hip_bfloat16 *)out.data_ptr(), a);
  return out;
}
#endif
