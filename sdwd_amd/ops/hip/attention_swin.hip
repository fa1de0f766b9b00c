// Shifted-window attention with a relative-position bias (SwinIR) on gfx950.
// The fragment helpers (crow, p_relayout), the transpose-read operand types,
// wide_shfl and the kernel attribute are common.h's, shared with attention.hip
// and attention_wide.hip.
//
// The problem per (window, head) is 64 queries x 64 keys x 32 channels: 12 KB
// of q, k and v in, 4 KB out, 16 MFMAs. It is bandwidth-bound, so the kernel
// moves qkv in and the output out and nothing else:
//
//  * addressing: qkv is the [B, H, W, 3, heads, 32] view of the QKV GEMM's
//    output and is read at its strides. Window (wy, wx), local token (i, j)
//    is grid token ((8 wy + i + shift) mod H, (8 wx + j + shift) mod W); the
//    output row is written at that token of a contiguous [B, H, W, heads*32]
//    tensor. No roll, partition, reverse or mask tensor exists.
//  * work split: a wave owns whole (window, head) problems. A block is four
//    independent waves of one head (blockIdx.y); wave g of the head takes
//    windows g, g + G, g + 2G, ... of the B * H/8 * W/8 windows. There is no
//    block barrier and no LDS shared between waves.
//  * bias residency: the head's [64, 64] fp32 bias (16 KB, more than the
//    qkv of one problem) is read once per wave into 64 registers a lane, in
//    the layout of the score accumulators and already in log2 units, and
//    stays there for the wave's whole window walk. The launcher picks G so a
//    wave walks several windows once the GPU is full (attention_swin_plan).
//  * QK^T: swapped, S^T = mfma(K_frag, Q_frag), 32x32x16 bf16. A lane holds
//    the scores of query qs*32 + lane%32 against keys sub*32 + crow(r, half).
//    K and Q fragments are 16-byte global loads, each piece read by exactly
//    one lane. The two 32-query halves run one after the other (32 score
//    registers live, not 64).
//  * scores: s = acc * (scale log2 e) + bias, in fp32. With shift > 0 only
//    the windows of the last window row / column straddle the wrap: there a
//    token's row region changes between i = 3 and i = 4, and its column region
//    between j = 3 and j = 4. In the accumulator layout that is qs != sub for
//    rows (a compile-time property of the tile) and ((lane & 4) != 0) !=
//    (half == 1) for columns (a constant of the lane), so the mask is one
//    wave-uniform branch and one add; other windows skip it.
//  * softmax: one pass, all 64 keys present: max and sum over the lane's 32
//    scores plus one exchange with lane ^ 32. The sum is of the unrounded fp32
//    P; P is rounded to bf16 once, as the PV operand (p_relayout).
//  * PV: V goes through a per-wave LDS tile (64 rows x 32, row stride 40
//    bf16 = 5 16-byte slots) and comes back as transposed fragments by
//    ds_read_b64_tr_b16, read once per window for both query halves. The
//    product is taken swapped as well, O^T = mfma(V_frag, P_frag): a lane then
//    holds output channels crow(r, half) of ITS query, so 1/l is a lane
//    constant (no broadcast) and p_relayout's two half-wave swaps turn the
//    tile into two 16-byte pieces a lane: channels 8*half..+8 and
//    16 + 8*half..+8 of the query's 64-byte head row.
//  * LDS ordering: a wave's DS operations execute in order, and the tile is
//    private to the wave, so the V store -> transpose read -> next window's
//    store sequence needs no barrier.
//  * no atomics; every output element is written once by one lane.

#include "common.h"

#include <algorithm>
#include <tuple>

struct SwinArgs {
  long sb, sy, sx, s3, sh;  // qkv strides (elements): batch, row, col, q/k/v, head
  int H, W;                 // token grid
  int nwy, nwx;             // windows per grid column / row
  int nwin;                 // B * nwy * nwx
  int heads;
  int shift;                // 0 or 4
  float scale;
};

constexpr int SWIN_RS = 40;  // V tile row stride (bf16): 80 B, 5 16-byte slots

WIDE_KERNEL_ATTR __launch_bounds__(256, 2) __global__
void swin_attn_bf16_kernel(const __hip_bfloat16 *__restrict__ qkv,
                           const float *__restrict__ bias,
                           __hip_bfloat16 *__restrict__ out, SwinArgs a) {
  constexpr float LOG2E = 1.4426950408889634f;
  __shared__ __align__(16) __bf16 vt[4][64][SWIN_RS];

  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int lq = lane % 32;    // query (scores, O^T column) / key (K fragment)
  const int half = lane / 32;  // half-wave id
  const int head = blockIdx.y;

  // the head's bias in the accumulator layout, log2 units: bs[qs][sub][r] is
  // bias[qs*32 + lq][sub*32 + crow(r, half)]; registers 4g..4g+3 are four
  // consecutive keys, one 16-byte load
  float bs[2][2][16];
  {
    const float *bh = bias + (long)head * 4096 + lq * 64 + 4 * half;
#pragma unroll
    for (int qs = 0; qs < 2; ++qs)
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 b4 =
              *(const f32x4 *)(bh + qs * 2048 + sub * 32 + 8 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) bs[qs][sub][4 * g + e] = b4[e] * LOG2E;
        }
  }
  const float l2scale = a.scale * LOG2E;
  const float neg = -100.0f * LOG2E;

  __bf16 *vw = &vt[wid][0][0];
  // staging piece it of a lane: tile row it*16 + lane/4, channels (lane%4)*8
  __bf16 *vst = vw + (lane >> 2) * SWIN_RS + (lane & 3) * 8;
  const __bf16 *vlane = vw + (((lane & 15) >> 2) + 8 * half) * SWIN_RS +
                        4 * (lane & 3) + ((lane >> 4) & 1) * 16;
  const long orow = (long)a.heads * 32;

  for (int w = blockIdx.x * 4 + wid; w < a.nwin; w += gridDim.x * 4) {
    const int wx = w % a.nwx;
    const int wt = w / a.nwx;
    const int wy = wt % a.nwy;
    const int bb = wt / a.nwy;
    const int y0 = 8 * wy + a.shift, x0 = 8 * wx + a.shift;
    const __hip_bfloat16 *base = qkv + bb * a.sb + head * a.sh;

    // this lane's token of each 32-token half: local (4*t + lq/8, lq%8). It
    // is the key row of K fragment t, the query of half t and its output row
    int xq = x0 + (lq & 7);
    xq = (xq >= a.W) ? xq - a.W : xq;
    long tok[2], otok[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      int y = y0 + 4 * t + (lq >> 3);
      y = (y >= a.H) ? y - a.H : y;
      tok[t] = y * a.sy + xq * a.sx + 8 * half;
      otok[t] = (((long)bb * a.H + y) * a.W + xq) * orow + head * 32 + 8 * half;
    }

    // V: 4 pieces a lane into the wave's tile
    {
      int xv = x0 + ((lane >> 2) & 7);
      xv = (xv >= a.W) ? xv - a.W : xv;
      const __hip_bfloat16 *vb = base + 2 * a.s3 + xv * a.sx + (lane & 3) * 8;
      bf16x8 vp[4];
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        int y = y0 + 2 * it + (lane >> 5);
        y = (y >= a.H) ? y - a.H : y;
        vp[it] = *(const bf16x8 *)(vb + y * a.sy);
      }
#pragma unroll
      for (int it = 0; it < 4; ++it)
        *(bf16x8 *)(vst + it * 16 * SWIN_RS) = vp[it];
    }
    // K fragments: lane holds K[sub*32 + lq][c*16 + 8*half ..+8]
    bf16x8 kf[2][2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int c = 0; c < 2; ++c)
        kf[sub][c] = *(const bf16x8 *)(base + a.s3 + tok[sub] + c * 16);
    bf16x8 qf[2][2];
#pragma unroll
    for (int qs = 0; qs < 2; ++qs)
#pragma unroll
      for (int c = 0; c < 2; ++c)
        qf[qs][c] = *(const bf16x8 *)(base + tok[qs] + c * 16);

    __builtin_amdgcn_wave_barrier();
    bf16x8 vf[4];  // V fragments of keys kc*16 .. +16, all 32 channels
#pragma unroll
    for (int kc = 0; kc < 4; ++kc)
      vf[kc] = tr_v_frag<SWIN_RS>(vlane + kc * 16 * SWIN_RS);
    __builtin_amdgcn_wave_barrier();

    // the wrap straddles only the last window row / column
    const bool lastrow = a.shift > 0 && wy == a.nwy - 1;
    const bool lastcol = a.shift > 0 && wx == a.nwx - 1;
    const float coladd =
        (lastcol && (((lane & 4) != 0) != (half == 1))) ? neg : 0.0f;

#pragma unroll
    for (int qs = 0; qs < 2; ++qs) {
      f32x16 s[2];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        s[sub] = (f32x16){};
#pragma unroll
        for (int c = 0; c < 2; ++c)
          s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              kf[sub][c], qf[qs][c], s[sub], 0, 0, 0);
      }
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          s[sub][r] = s[sub][r] * l2scale + bs[qs][sub][r];
      if (lastrow || lastcol) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          const float add = (lastrow && sub != qs) ? neg : coladd;
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

      // O^T[channel][query] = sum over 16-key chunks of mfma(V_frag, P_frag)
      bf16x8 pa[4];
      p_relayout(s[0], pa[0], pa[1]);
      p_relayout(s[1], pa[2], pa[3]);
      f32x16 o = (f32x16){};
#pragma unroll
      for (int kc = 0; kc < 4; ++kc)
        o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[kc], pa[kc], o, 0, 0, 0);

      const float inv = 1.0f / l;  // l >= 1: the row's max contributes 1
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] *= inv;
      bf16x8 o0, o1;  // channels 8*half..+8 and 16 + 8*half..+8 of the query
      p_relayout(o, o0, o1);
      *(bf16x8 *)(out + otok[qs]) = o0;
      *(bf16x8 *)(out + otok[qs] + 16) = o1;
    }
  }
}

// ---------------------------------------------------------------------------
// host-side dispatch (torch API lives in ext.hip which includes this file)
// ---------------------------------------------------------------------------

// {windows a wave walks, blocks per head}. A block is four waves of one head.
// Up to SWIN_WAVES resident waves (256 CUs x 8) every wave takes one window;
// past that the walk grows, and the head's bias is read once per walk.
constexpr long SWIN_WAVES = 2048;
std::tuple<long, long> attention_swin_plan(long nwin, long heads) {
  TORCH_CHECK(nwin >= 1 && heads >= 1, "attention_swin: empty problem");
  const long per_head = std::max<long>(1, SWIN_WAVES / heads);
  const long walk = (nwin + per_head - 1) / per_head;
  const long waves = (nwin + walk - 1) / walk;
  return {walk, (waves + 3) / 4};
}

#ifdef __HIP_PLATFORM_AMD__
// qkv [B, H, W, 3, heads, 32] view, bias [heads, 64, 64] contiguous fp32 (the
// caller checked everything an address is formed from)
static torch::Tensor swin_attn_raw(torch::Tensor qkv, torch::Tensor bias,
                                   double scale, long shift) {
  const long B = qkv.size(0), H = qkv.size(1), W = qkv.size(2),
             heads = qkv.size(4);
  auto out = torch::empty({B, H, W, heads * 32}, qkv.options());
  SwinArgs a;
  a.sb = qkv.stride(0);
  a.sy = qkv.stride(1);
  a.sx = qkv.stride(2);
  a.s3 = qkv.stride(3);
  a.sh = qkv.stride(4);
  a.H = (int)H;
  a.W = (int)W;
  a.nwy = (int)(H / 8);
  a.nwx = (int)(W / 8);
  a.nwin = (int)(B * (H / 8) * (W / 8));
  a.heads = (int)heads;
  a.shift = (int)shift;
  a.scale = (float)scale;
  const auto [walk, blocks] = attention_swin_plan(a.nwin, heads);
  (void)walk;
  hipLaunchKernelGGL(swin_attn_bf16_kernel,
                     dim3((unsigned)blocks, (unsigned)heads), dim3(256), 0,
                     cur_stream(), (const __hip_bfloat16 *)qkv.data_ptr(),
                     (const float *)bias.data_ptr(),
                     (__hip_bfloat16 *)out.data_ptr(), a);
  return out;
}
#endif
