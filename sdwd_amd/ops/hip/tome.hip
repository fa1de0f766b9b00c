// Token merging (ToMe) for the level-0 self-attention, gfx950.
//
// The 2x2 partition splits the N = h*w tokens of a block input x [B,N,C]
// into Nd dst tokens (even row, even column) and Ns src tokens (the rest);
// src_tok / dst_tok list their token positions in ascending order. The
// kernels here are the float side of the feature; the integer plan (which
// src tokens merge, the CSR of every dst's members) is torch integer ops on
// the results of the match (ops/__init__.py, tome_plan).
//
//  * tome_rnorm_bf16_kernel: 1/|x_t| = rsqrt(max(sum x^2, 2^-80)) for every
//    token, one wave per row, fp32. The match reads the dst entries (a
//    pre-pass instead of a reduction inside the staging loop: the staging
//    threads of one dst row do not sit in one wave, and the table is 4 B per
//    token against the row's 2*C).
//  * tome_match_bf16_kernel<C>: for every src row the maximum cosine score
//    over the dst rows of its batch row, and the lowest dst index attaining
//    it. It is attention.hip's swapped QK^T with a running (max, argmax) in
//    place of the softmax: a workgroup of 4 waves, each wave owns one 32-row
//    src sub-tile whose fragments are read once through src_tok
//    (load_q_frags' layout), dst tiles of 64 rows are gathered through
//    dst_tok into padded LDS rows, S^T = mfma(dst_frag, src_frag) leaves a
//    lane with the scores of ONE src row for 16 of 32 dst rows. The score
//    takes 1/|b_j| in fp32 after the MFMA; 1/|a_i|, positive and constant
//    along the row, multiplies the final max only. Scores never reach
//    memory.
//    Ties: a lane walks its dst rows in ascending order and replaces on a
//    strict >, so it keeps the lowest index; the half-wave join prefers the
//    lower index on equality.
//  * tome_merge_bf16_kernel: one output row per wave. Unmerged src rows are
//    copies; a dst row is its own row plus its members in CSR order, summed
//    in fp32, divided by float(1 + count), rounded to bf16 once. No atomics.
//  * tome_unmerge_bf16_kernel: row gather through slot, 16 B per lane.
//
// Every table entry is clamped to its legal range inside the kernels, so a
// bad table reads a wrong row of the same tensor, never outside it.
#include "common.h"

static constexpr int TOME_DB = 64;   // dst rows per staged tile
static constexpr int TOME_PADK = 8;  // bf16 per-row pad (row = odd count of 16 B slots)

__device__ __forceinline__ int tome_clamp(int v, int hi /*exclusive*/) {
  return v < 0 ? 0 : (v >= hi ? hi - 1 : v);
}

__global__ __launch_bounds__(256) void tome_rnorm_bf16_kernel(
    const __hip_bfloat16 *__restrict__ x, float *__restrict__ rn, long R,
    int C) {
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const long row = (long)blockIdx.x * 4 + wid;
  if (row >= R) return;
  const bf16x8 *xb = (const bf16x8 *)(x + row * C);
  float ss = 0.f;
  for (int i = lane; i < C / 8; i += WAVE) {
    const bf16x8 v = xb[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += (float)v[j] * (float)v[j];
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) ss += __shfl_xor(ss, off, WAVE);
  if (lane == 0) rn[row] = rsqrtf(fmaxf(ss, 0x1p-80f));
}

template <int C>
__launch_bounds__(256, 2) __global__ void tome_match_bf16_kernel(
    const __hip_bfloat16 *__restrict__ x, const float *__restrict__ rn,
    const int *__restrict__ src_tok, const int *__restrict__ dst_tok,
    float *__restrict__ node_max, int *__restrict__ node_idx, int N, int Ns,
    int Nd) {
  static_assert(C % 16 == 0, "tome_match: C must be a multiple of 16");
  constexpr int NC = C / 16;  // k-chunks
  constexpr int ROW = C + TOME_PADK;

  __shared__ __align__(16) __bf16 dt[TOME_DB][ROW];
  __shared__ float drn[TOME_DB];

  const int bb = blockIdx.y;
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int lq = lane % 32;
  const int half = lane / 32;
  const int i = blockIdx.x * 128 + wid * 32 + lq;  // this lane's src row

  const __hip_bfloat16 *xb = x + (long)bb * N * C;
  const float *rnb = rn + (long)bb * N;

  // src fragments, read once: lane holds a[i][c*16 + 8*half + 0..7]. A row
  // past Ns re-reads the last one and is never stored.
  const int stok = tome_clamp(src_tok[i < Ns ? i : Ns - 1], N);
  bf16x8 sf[NC];
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    sf[c] = *(const bf16x8 *)(xb + (long)stok * C + c * 16 + 8 * half);
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += (float)sf[c][j] * (float)sf[c][j];
  }
  ss += __shfl_xor(ss, 32, WAVE);
  const float arn = rsqrtf(fmaxf(ss, 0x1p-80f));

  float best = -INFINITY;
  int bidx = 0;

  for (int d0 = 0; d0 < Nd; d0 += TOME_DB) {
    __syncthreads();  // previous tile's LDS reads complete
    // rows past Nd are staged as the last dst row and masked below
    for (int idx = threadIdx.x; idx < TOME_DB * (C / 8); idx += 256) {
      const int r = idx / (C / 8);
      const int c8 = idx % (C / 8);
      const int j = d0 + r < Nd ? d0 + r : Nd - 1;
      const int tok = tome_clamp(dst_tok[j], N);
      *(bf16x8 *)&dt[r][c8 * 8] =
          *(const bf16x8 *)(xb + (long)tok * C + c8 * 8);
    }
    if (threadIdx.x < TOME_DB) {
      const int j = d0 + threadIdx.x < Nd ? d0 + threadIdx.x : Nd - 1;
      drn[threadIdx.x] = rnb[tome_clamp(dst_tok[j], N)];
    }
    __syncthreads();

#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      f32x16 acc = (f32x16){};
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const bf16x8 df =
            *(const bf16x8 *)&dt[sub * 32 + lq][c * 16 + 8 * half];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, sf[c], acc, 0, 0, 0);
      }
      // crow(r, half) ascends with r: ascending j inside the lane
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jl = sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const int j = d0 + jl;
        const float s = j < Nd ? acc[r] * drn[jl] : -INFINITY;
        if (s > best) {
          best = s;
          bidx = j;
        }
      }
    }
  }

  // join the half-wave pair: both halves hold the same src row
  const float obest = __shfl_xor(best, 32, WAVE);
  const int oidx = __shfl_xor(bidx, 32, WAVE);
  if (obest > best || (obest == best && oidx < bidx)) {
    best = obest;
    bidx = oidx;
  }
  if (half == 0 && i < Ns) {
    node_max[(long)bb * Ns + i] = best * arn;
    node_idx[(long)bb * Ns + i] = bidx;
  }
}

// out [B, N - r, C]. Rows [0, Nu) copy x[b, unm_tok[b, row]]; row Nu + j is
// (x[dst_tok[j]] + sum of x[members[seg_start[j] .. seg_start[j+1])]) /
// (1 + count). Nu = Ns - r.
__global__ __launch_bounds__(256) void tome_merge_bf16_kernel(
    const __hip_bfloat16 *__restrict__ x, const int *__restrict__ dst_tok,
    const int *__restrict__ unm_tok, const int *__restrict__ seg_start,
    const int *__restrict__ members, __hip_bfloat16 *__restrict__ out, int B,
    int N, int Nu, int Nd, int r, int C) {
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int M = Nu + Nd;
  const long grow = (long)blockIdx.x * 4 + wid;
  if (grow >= (long)B * M) return;
  const int bb = (int)(grow / M);
  const int row = (int)(grow % M);
  const __hip_bfloat16 *xb = x + (long)bb * N * C;
  bf16x8 *ob = (bf16x8 *)(out + grow * C);
  const int nv = C / 8;

  if (row < Nu) {
    const int tok = tome_clamp(unm_tok[(long)bb * Nu + row], N);
    const bf16x8 *sb = (const bf16x8 *)(xb + (long)tok * C);
    for (int i = lane; i < nv; i += WAVE) ob[i] = sb[i];
    return;
  }
  const int j = row - Nu;
  const int dtok = tome_clamp(dst_tok[j], N);
  int m0 = seg_start[(long)bb * (Nd + 1) + j];
  int m1 = seg_start[(long)bb * (Nd + 1) + j + 1];
  m0 = m0 < 0 ? 0 : (m0 > r ? r : m0);
  m1 = m1 < m0 ? m0 : (m1 > r ? r : m1);
  const float cnt = (float)(1 + m1 - m0);
  const int *mb = members + (long)bb * r;
  for (int i = lane; i < nv; i += WAVE) {
    const bf16x8 v = ((const bf16x8 *)(xb + (long)dtok * C))[i];
    float a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = (float)v[k];
    for (int m = m0; m < m1; ++m) {
      const int tok = tome_clamp(mb[m], N);
      const bf16x8 u = ((const bf16x8 *)(xb + (long)tok * C))[i];
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] += (float)u[k];
    }
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = (__bf16)(a[k] / cnt);
    ob[i] = o;
  }
}

// out[b, t] = y[b, slot[b, t]]; y [B, M, C], out [B, N, C]; nv = C / 8
// 16 B vectors per row, one per lane.
__global__ __launch_bounds__(256) void tome_unmerge_bf16_kernel(
    const __hip_bfloat16 *__restrict__ y, const int *__restrict__ slot,
    __hip_bfloat16 *__restrict__ out, long rows /*B*N*/, int N, int M,
    int nv) {
  const long total = rows * nv;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (long)gridDim.x * 256) {
    const long row = idx / nv;
    const int i = (int)(idx % nv);
    const long bb = row / N;
    const int s = tome_clamp(slot[row], M);
    ((bf16x8 *)out)[idx] = ((const bf16x8 *)y)[(bb * M + s) * nv + i];
  }
}
