// SwinIR's MLP half of a Swin block in one kernel on gfx950:
//
//   h   = gelu(x W1^T + b1)        fp32 accumulate, bf16 ONCE as GEMM 2's operand
//   s   = h W2^T + b2 + res        fp32
//   sum = bf16(s)
//   ln  = bf16(LN(s) * gamma + beta)   from the fp32 s, only when LN
//
// x, res, sum, ln are [R, C] bf16 token rows, C % 4 == 0, C <= CPAD in
// {192, 256}. The hidden activation exists in neither LDS nor memory; the
// kernel reads x and res and writes sum and ln, nothing else leaves the chip.
//
//  * work split: a block is four waves and owns 128 token rows; a wave owns
//    32 rows and all C output columns, and never talks to the other waves
//    except through the shared weight tiles.
//  * x: the wave's 32 x CPAD fragment (B operand of GEMM 1: lane holds
//    x[row lane%32][16c + 8*half .. +8], c < CPAD/16) is loaded once with
//    8-byte loads (rows are only 8-byte aligned at C = 180) and stays in
//    CPAD/4 registers. Columns >= C and rows >= R load as zero.
//  * hidden chunks of 32. GEMM 1 is taken swapped, H^T[32 hidden, 32 rows] =
//    mfma(W1_frag, x_frag) on v_mfma_f32_32x32x16_bf16, CPAD/16 MFMAs: a
//    lane holds hidden units crow(r, half) of ITS row. b1 and gelu_f go on
//    the 16 accumulators, and p_relayout (common.h, the exchange the
//    attention kernels use for P) turns them into the two 16-deep operand
//    fragments of GEMM 2.
//  * GEMM 2 is swapped as well: Out^T[32 columns, 32 rows] += mfma(W2_frag,
//    H_frag) into CPAD/32 f32x16 accumulators. A lane therefore holds columns
//    32n + crow(r, half) of its own row: the residual and b2 are the
//    accumulators' initial value (8-byte loads, in flight under the first
//    chunk), the LayerNorm statistics are a sum over the lane's registers plus
//    ONE exchange with lane ^ 32, and 1/sigma is a lane constant.
//  * weights: w1p [Hp, CPAD] and w2p [Hp/32, CPAD, 32] (chunk j of W2 as
//    [column][hidden], so both chunks are one contiguous 32*CPAD block) are
//    zero-padded once by the caller. A chunk of each is staged through LDS for
//    the four waves and double-buffered through registers: chunk j+1's global
//    loads are issued before chunk j's MFMAs and written to the other buffer
//    after them, one barrier a chunk. LDS = 2 buffers x 2 matrices x 32*CPAD
//    bf16 = 48 KB (192) / 64 KB (256) in ONE object.
//  * bank conflicts: SWIZZLE, not padding (padding would put CPAD 256 over
//    64 KB). 64 banks x 4 B, a b128 read is served 16 lanes at a time, and a
//    fragment's 16 lanes read 16 consecutive rows at one 16-byte slot. W1
//    rows are CPAD/8 slots: slot ^= row & 15 (256: rows start 0 mod 16 slots)
//    or slot ^= (row >> 1) & 7 (192: rows alternate 0 / 8 mod 16), both a
//    bijection of 16 consecutive rows onto the 16 slot positions. W2 rows are
//    4 slots: slot ^= ((row >> 2) ^ (row >> 1)) & 3, distinct for the four
//    rows that share row % 4. The XOR stays inside an aligned group of slots
//    of the same row, so staging writes the same bytes elsewhere in the row.
//  * epilogue: the sum and the normalised row leave as 16-byte stores when
//    C % 8 == 0 (p_relayout again: columns 32n + 8*half ..+8 and 32n + 16 +
//    8*half ..+8) and as 8-byte stores straight from the accumulator quads
//    otherwise (C = 180). Variance is two-pass over the registers; the
//    CPAD - C zero columns' (0 - mean)^2 is taken back out in closed form.
//  * masking: rows >= R are computed on zeros and never stored; columns >= C
//    are never loaded or stored (their accumulators are exactly zero: zero
//    weight columns, no residual, no bias). Padded hidden units have zero W1
//    rows and zero b1, so gelu(0) = 0 meets zero W2 entries.
//  * compiled without packed fp32 VALU ops (WIDE_KERNEL_ATTR), hence the
//    spelled-out barrier and wide_shfl; no atomics, every output element is
//    written once by one lane.

#include "common.h"

constexpr int MLP_ROWS = 128;  // token rows a block
constexpr int MLP_HC = 32;     // hidden units a chunk

__device__ __forceinline__ void mlp_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int CPAD>
__device__ __forceinline__ int mlp_w1_swz(int row) {
  return CPAD == 256 ? (row & 15) : ((row >> 1) & 7);
}
__device__ __forceinline__ int mlp_w2_swz(int row) {
  return ((row >> 2) ^ (row >> 1)) & 3;
}

// one [32 columns, 32 rows] accumulator tile of a lane's row -> memory at
// columns 32n ..: 16-byte pieces when wide, accumulator quads otherwise
__device__ __forceinline__ void mlp_store_tile(__hip_bfloat16 *row, int n,
                                               int half, int C, bool wide,
                                               const f32x16 &v) {
  if (wide) {
    bf16x8 o0, o1;
    p_relayout(v, o0, o1);
    const int col = 32 * n + 8 * half;
    if (col < C) *(bf16x8 *)(row + col) = o0;
    if (col + 16 < C) *(bf16x8 *)(row + col + 16) = o1;
  } else {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int col = 32 * n + 8 * g + 4 * half;
      uint2 o;
      o.x = pack_bf16(v[4 * g], v[4 * g + 1]);
      o.y = pack_bf16(v[4 * g + 2], v[4 * g + 3]);
      if (col < C) *(uint2 *)(row + col) = o;
    }
  }
}

template <int CPAD, bool LN>
WIDE_KERNEL_ATTR __launch_bounds__(256) __global__
void swin_mlp_bf16_kernel(const __hip_bfloat16 *__restrict__ x,
                          const __hip_bfloat16 *__restrict__ res,
                          const __hip_bfloat16 *__restrict__ w1p,
                          const float *__restrict__ b1p,
                          const __hip_bfloat16 *__restrict__ w2p,
                          const float *__restrict__ b2,
                          const float *__restrict__ gamma,
                          const float *__restrict__ beta,
                          __hip_bfloat16 *__restrict__ out_sum,
                          __hip_bfloat16 *__restrict__ out_ln, long R, int C,
                          int nchunk, float eps) {
  constexpr int KS = CPAD / 16;        // k steps of GEMM 1
  constexpr int NT = CPAD / 32;        // column tiles of GEMM 2
  constexpr int SPR = CPAD / 8;        // 16-byte slots of a W1 row
  constexpr int NP = CPAD / 64;        // staged pieces a thread and matrix
  constexpr int WBUF = MLP_HC * CPAD;  // elements of one matrix chunk
  // [buffer][W1 | W2]. Exactly 65,536 B at CPAD 256, the ceiling of static
  // LDS: one more __shared__ byte in this kernel no longer compiles
  __shared__ __align__(16) __bf16 wt[2][2][WBUF];

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid % WAVE;
  const int lq = lane % 32;    // the lane's token row / the weight row it reads
  const int half = lane / 32;  // half-wave id
  const long tok = (long)blockIdx.x * MLP_ROWS + wid * 32 + lq;
  const bool valid = tok < R;
  const bool wide = (C & 7) == 0;
  const long roff = valid ? tok * C : 0;  // never dereferenced when !valid

  // staging: piece p = tid + 256 i of a chunk is its bytes 16p .. 16p + 15
  int dst1[NP], dst2[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int p = tid + 256 * i;
    const int r1 = p / SPR, s1 = p % SPR;
    dst1[i] = (r1 * SPR + (s1 ^ mlp_w1_swz<CPAD>(r1))) * 8;
    const int r2 = p >> 2, s2 = p & 3;
    dst2[i] = WBUF + (r2 * 4 + (s2 ^ mlp_w2_swz(r2))) * 8;
  }
  bf16x8 st1[NP], st2[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    st1[i] = *(const bf16x8 *)(w1p + (tid + 256 * i) * 8);
    st2[i] = *(const bf16x8 *)(w2p + (tid + 256 * i) * 8);
  }

  // the wave's x fragment
  bf16x8 xf[KS];
  {
    const __hip_bfloat16 *xr = x + roff;
#pragma unroll
    for (int c = 0; c < KS; ++c) {
      const int k0 = 16 * c + 8 * half;
      bf16x4 lo = (bf16x4){}, hi = (bf16x4){};
      if (valid && k0 < C) lo = *(const bf16x4 *)(xr + k0);
      if (valid && k0 + 4 < C) hi = *(const bf16x4 *)(xr + k0 + 4);
      xf[c] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
  }

  // Out^T accumulators start as b2 + res: acc[n][4g + e] is column
  // 32n + 8g + 4*half + e of the lane's row
  f32x16 acc[NT];
  {
    const __hip_bfloat16 *rr = res + roff;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = 32 * n + 8 * g + 4 * half;
        f32x4 v = (f32x4){};
        if (col < C) {
          v = *(const f32x4 *)(b2 + col);
          if (valid) {
            const bf16x4 r4 = *(const bf16x4 *)(rr + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += (float)r4[e];
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[n][4 * g + e] = v[e];
      }
  }

#pragma unroll
  for (int i = 0; i < NP; ++i) {
    *(bf16x8 *)(&wt[0][0][0] + dst1[i]) = st1[i];
    *(bf16x8 *)(&wt[0][0][0] + dst2[i]) = st2[i];
  }
  mlp_barrier();

  // fragment reads: W1 row lq at slot 2c + half, W2 row 32n + lq at slot
  // 2kc + half (its swizzle depends on row % 16 only: a lane constant)
  const int w1row = lq * SPR * 8;
  const int sw1 = mlp_w1_swz<CPAD>(lq);
  const int sw2 = mlp_w2_swz(lq);
  const int w2o0 = WBUF + (lq * 4 + (half ^ sw2)) * 8;
  const int w2o1 = WBUF + (lq * 4 + ((2 + half) ^ sw2)) * 8;

  for (int j = 0; j < nchunk; ++j) {
    const __bf16 *ws = &wt[j & 1][0][0];
    const bool more = j + 1 < nchunk;
    if (more) {
      const long o = (long)(j + 1) * WBUF;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        st1[i] = *(const bf16x8 *)(w1p + o + (tid + 256 * i) * 8);
        st2[i] = *(const bf16x8 *)(w2p + o + (tid + 256 * i) * 8);
      }
    }
    f32x4 bb[4];  // b1 of hidden units j*32 + 8g + 4*half .. +4
#pragma unroll
    for (int g = 0; g < 4; ++g)
      bb[g] = *(const f32x4 *)(b1p + j * MLP_HC + 8 * g + 4 * half);

    f32x16 ht = (f32x16){};
#pragma unroll
    for (int c = 0; c < KS; ++c) {
      const bf16x8 a =
          *(const bf16x8 *)(ws + w1row + ((2 * c + half) ^ sw1) * 8);
      ht = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xf[c], ht, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) ht[r] = gelu_f(ht[r] + bb[r >> 2][r & 3]);
    bf16x8 h0, h1;  // hidden units 0..15 and 16..31 of the chunk
    p_relayout(ht, h0, h1);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const bf16x8 a0 = *(const bf16x8 *)(ws + n * 32 * 32 + w2o0);
      const bf16x8 a1 = *(const bf16x8 *)(ws + n * 32 * 32 + w2o1);
      acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, h0, acc[n], 0, 0, 0);
      acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, h1, acc[n], 0, 0, 0);
    }
    if (more) {
      __bf16 *wn = &wt[(j + 1) & 1][0][0];
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        *(bf16x8 *)(wn + dst1[i]) = st1[i];
        *(bf16x8 *)(wn + dst2[i]) = st2[i];
      }
    }
    mlp_barrier();
  }

  if (!valid) return;
  __hip_bfloat16 *srow = out_sum + roff;
#pragma unroll
  for (int n = 0; n < NT; ++n) mlp_store_tile(srow, n, half, C, wide, acc[n]);

  if constexpr (LN) {
    float s = 0.f;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) s += acc[n][r];
    s += wide_shfl(s, lane ^ 32);
    const float inv_c = 1.0f / (float)C;
    const float mean = s * inv_c;
    float q = 0.f;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float d = acc[n][r] - mean;
        q += d * d;
      }
    q += wide_shfl(q, lane ^ 32);
    const float var = (q - (float)(CPAD - C) * mean * mean) * inv_c;
    const float rstd = __builtin_amdgcn_rsqf(fmaxf(var, 0.0f) + eps);
    __hip_bfloat16 *lrow = out_ln + roff;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      f32x16 y;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = 32 * n + 8 * g + 4 * half;
        f32x4 gm = (f32x4){}, bt = (f32x4){};
        if (col < C) {
          gm = *(const f32x4 *)(gamma + col);
          bt = *(const f32x4 *)(beta + col);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
          y[4 * g + e] = (acc[n][4 * g + e] - mean) * rstd * gm[e] + bt[e];
      }
      mlp_store_tile(lrow, n, half, C, wide, y);
    }
  }
}

// ---------------------------------------------------------------------------
// host-side dispatch (torch API lives in ext.hip which includes this file)
// ---------------------------------------------------------------------------
#ifdef __HIP_PLATFORM_AMD__
// x, res [R, C] contiguous bf16; the caller checked everything an address is
// formed from. gamma == nullptr: no LayerNorm output
template <int CPAD>
static void swin_mlp_launch(const torch::Tensor &x, const torch::Tensor &res,
                            const torch::Tensor &w1p, const torch::Tensor &b1p,
                            const torch::Tensor &w2p, const torch::Tensor &b2,
                            const float *gamma, const float *beta,
                            torch::Tensor &sum, void *ln, double eps) {
  const long R = x.size(0);
  const int C = (int)x.size(1);
  auto kern = gamma ? swin_mlp_bf16_kernel<CPAD, true>
                    : swin_mlp_bf16_kernel<CPAD, false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((R + MLP_ROWS - 1) / MLP_ROWS)),
                     dim3(256), 0, cur_stream(),
                     (const __hip_bfloat16 *)x.data_ptr(),
                     (const __hip_bfloat16 *)res.data_ptr(),
                     (const __hip_bfloat16 *)w1p.data_ptr(),
                     (const float *)b1p.data_ptr(),
                     (const __hip_bfloat16 *)w2p.data_ptr(),
                     (const float *)b2.data_ptr(), gamma, beta,
                     (__hip_bfloat16 *)sum.data_ptr(), (__hip_bfloat16 *)ln, R,
                     C, (int)(w1p.size(0) / MLP_HC), (float)eps);
}
#endif
