// The elementwise tail of a HAT hybrid attention block, and the residual +
// LayerNorm of any transformer block whose width is a multiple of 4 but not
// of 8 (embed 180, 60):
//
//   gate[b, :] = scale * sigmoid(W2 relu(W1 mean_hw(c[b]) + b1) + b2)
//   s          = (x + a) + gate[b] * c           (s = x + a without GATED)
//   out_sum    = bf16(s),  out_ln = bf16(LN(s) * w + b)
//
// All tensors are bf16 rows [R, C], R = B * HW, C % 4 == 0, 4 <= C <= 256, so
// a row is a whole number of 8-byte pieces (360 B at C = 180: 8- but not
// 16-byte aligned) and V = C / 4 <= 64 pieces long. Math is fp32. Nothing
// here uses an atomic: every sum has one fixed order, so the same inputs give
// the same bits on every call.
//
// Three launches, six passes over a tensor (c for the mean; x, a, c in and
// sum, ln out):
//   channel_pool_bf16_kernel  partial column sums per POOL_ROWS-row chunk
//   channel_gate_kernel       chunk sums -> mean -> the two tiny products
//   hab_tail_bf16_kernel      the row kernel
#include "common.h"

#define POOL_ROWS 256   // rows of one batch element a pool block owns
#define GATE_THREADS 1024
#define GATE_MAX_S 32
#define TAIL_ITERS 4    // row pairs a wave walks

// ---------------------------------------------------------------------------
// c [B, HW, C] -> partial [B, P, C] fp32, P = ceil(HW / POOL_ROWS).
// grid = (P, B), block = 256 laid out as RP = 256 / V row lanes times V piece
// columns (225 of 256 threads at C = 180, 252 at 144): a thread owns four
// channels and the rows ro, ro + RP, ... of the chunk, so consecutive
// threads read consecutive 8-byte pieces across row ends and every wave's
// loads are one contiguous span. Four rows are in flight per thread. The row
// lanes are folded through LDS in index order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void channel_pool_bf16_kernel(
    const __hip_bfloat16 *__restrict__ c, float *__restrict__ partial, int C,
    int HW, int P) {
  __shared__ float red[256 * 4];  // [ro][C]
  const int V = C / 4, RP = 256 / V;
  const int tid = threadIdx.x;
  const int ro = tid / V, vc = tid % V;
  const int r0 = blockIdx.x * POOL_ROWS;
  const int r1 = min(HW, r0 + POOL_ROWS);
  if (ro < RP) {
    const bf16x4 *base =
        (const bf16x4 *)(c + ((long)blockIdx.y * HW) * C) + vc;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int r = r0 + ro;
    for (; r + 3 * RP < r1; r += 4 * RP) {
      bf16x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = base[(long)(r + u * RP) * V];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += (float)v[u][j];
    }
    for (; r < r1; r += RP) {
      const bf16x4 v = base[(long)r * V];
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += (float)v[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[ro * C + vc * 4 + j] = s[j];
  }
  __syncthreads();
  if (tid < C) {
    float acc = 0.f;
    for (int q = 0; q < RP; ++q) acc += red[q * C + tid];
    partial[((long)blockIdx.y * P + blockIdx.x) * C + tid] = acc;
  }
}

// ---------------------------------------------------------------------------
// partial [B, P, C] -> gate [B, C] fp32. grid = B, block = 1024.
// The P chunk sums (1024 of them at a 512 x 512 grid) are the long part:
// thread (pg, vc) of 16 x 64 adds chunks pg, pg + 16, ... of four channels in
// that order, eight 16-byte loads in flight, then the 16 groups are added in
// index order. hidden: one wave per squeeze unit, a fixed butterfly. The
// sigmoid uses expf: B * C calls in all.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(GATE_THREADS) void channel_gate_kernel(
    const float *__restrict__ partial, const float *__restrict__ w1,
    const float *__restrict__ b1, const float *__restrict__ w2,
    const float *__restrict__ b2, float *__restrict__ gate, int C, int S,
    int P, float inv_hw, float scale) {
  __shared__ float red[16 * 256];
  __shared__ float mean[256];
  __shared__ float hidden[GATE_MAX_S];
  const int tid = threadIdx.x;
  const int V = C / 4;
  const int pg = tid / WAVE, vc = tid % WAVE;
  const float *pb = partial + (long)blockIdx.x * P * C;
  if (vc < V) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int p = pg;
    for (; p + 7 * 16 < P; p += 8 * 16) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = ((const f32x4 *)(pb + (long)(p + u * 16) * C))[vc];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; p < P; p += 16) acc += ((const f32x4 *)(pb + (long)p * C))[vc];
#pragma unroll
    for (int j = 0; j < 4; ++j) red[pg * C + vc * 4 + j] = acc[j];
  }
  __syncthreads();
  if (tid < C) {
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc += red[q * C + tid];
    mean[tid] = acc * inv_hw;
  }
  __syncthreads();
  for (int s = pg; s < S; s += GATE_THREADS / WAVE) {
    float acc = 0.f;
    for (int ch = vc; ch < C; ch += WAVE) acc += w1[s * C + ch] * mean[ch];
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1)
      acc += __shfl_xor(acc, off, WAVE);
    if (vc == 0) hidden[s] = fmaxf(acc + b1[s], 0.f);
  }
  __syncthreads();
  if (tid < C) {
    float acc = b2[tid];
    for (int s = 0; s < S; ++s) acc += w2[tid * S + s] * hidden[s];
    gate[(long)blockIdx.x * C + tid] = scale / (1.f + expf(-acc));
  }
}

// ---------------------------------------------------------------------------
// The row kernel. A row is V <= 64 pieces of 8 bytes, one piece a lane, in a
// group of G lanes (G = 16, 32 or 64, the least that holds V): a wave holds
// RPW = 64 / G rows side by side and walks TAIL_ITERS pairs of such row sets,
// both sets of a pair loaded before either is used. At C = 180 that is two
// rows, 45 of 64 lanes, and 2 x 3 x 360 B of loads in flight per wave; at
// the six waves a SIMD the gated form's 78 VGPRs allow that is 52 KB per CU
// (eight waves and 46 KB un-gated), above the ~40 KB that HBM latency times
// a CU's share of the bandwidth asks for. 16-byte pieces would need a lane
// that straddles two rows at C = 180 and buy nothing at that depth.
// The statistics are a butterfly inside the group (every lane ends with the
// sums), taken from the unrounded fp32 s that stays in registers until the
// normalise step: add_layer_norm_bf16_kernel's convention.
// The norm's w and b pieces are loaded once per wave. GATED: a lane tracks
// the batch element of each of its two rows without a division in the loop
// and reloads its gate piece only when that changes, so a block may span any
// number of batch elements (HW below the block's rows included).
// grid = ceil(R / (4 * TAIL_ITERS * 2 * RPW)), block = 256.
// ---------------------------------------------------------------------------
template <bool GATED>
__global__ __launch_bounds__(256) void hab_tail_bf16_kernel(
    const __hip_bfloat16 *__restrict__ x, const __hip_bfloat16 *__restrict__ a,
    const __hip_bfloat16 *__restrict__ c, const float *__restrict__ gate,
    const float *__restrict__ w, const float *__restrict__ b,
    __hip_bfloat16 *__restrict__ out_sum, __hip_bfloat16 *__restrict__ out_ln,
    int R, int C, int HW, int G, float eps) {
  const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int V = C / 4, RPW = WAVE / G;
  const int sub = lane / G, pc = lane % G;
  const bool col = pc < V;
  const float inv_c = 1.f / (float)C;
  // 64-bit only here: R < 2^31 by dispatch, the product may pass it
  const long wave0 = ((long)blockIdx.x * 4 + wid) * (TAIL_ITERS * 2 * RPW);
  if (wave0 >= R) return;  // the whole wave leaves: no shuffle is left short

  f32x4 wv = {0.f, 0.f, 0.f, 0.f}, bv = wv;
  if (col) {
    wv = ((const f32x4 *)w)[pc];
    bv = ((const f32x4 *)b)[pc];
  }
  // rows row[k] = wave0 + sub + k * RPW, k = 0, 1; then += 2 * RPW a step
  int bat[2], rem[2], have[2] = {-1, -1};
  f32x4 gv[2] = {wv, wv};
  if constexpr (GATED) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned r = (unsigned)(wave0 + sub + k * RPW);
      bat[k] = (int)(r / (unsigned)HW);
      rem[k] = (int)(r % (unsigned)HW);
    }
  }

  for (int it = 0; it < TAIL_ITERS; ++it) {
    const long base = wave0 + (long)it * 2 * RPW + sub;
    if (base - sub >= R) break;  // wave-uniform
    bf16x4 vx[2], va[2], vc[2];
    bool on[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const long row = base + k * RPW;
      on[k] = col && row < R;
      if (on[k]) {
        const long off = row * V + pc;
        vx[k] = ((const bf16x4 *)x)[off];
        va[k] = ((const bf16x4 *)a)[off];
        if constexpr (GATED) vc[k] = ((const bf16x4 *)c)[off];
      }
    }
    float s[2][4], sum[2] = {0.f, 0.f}, sq[2] = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if constexpr (GATED) {
        if (on[k] && have[k] != bat[k]) {
          gv[k] = ((const f32x4 *)(gate + (long)bat[k] * C))[pc];
          have[k] = bat[k];
        }
      }
      if (on[k]) {
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float f = (float)vx[k][j] + (float)va[k][j];
          if constexpr (GATED) f += gv[k][j] * (float)vc[k][j];
          s[k][j] = f;
          sum[k] += f;
          sq[k] += f * f;
          o[j] = (__bf16)f;
        }
        ((bf16x4 *)out_sum)[(base + k * RPW) * V + pc] = o;
      }
    }
    for (int off = G / 2; off > 0; off >>= 1) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        sum[k] += __shfl_xor(sum[k], off, WAVE);
        sq[k] += __shfl_xor(sq[k], off, WAVE);
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (on[k]) {
        const float mean = sum[k] * inv_c;
        const float rstd = rsqrtf(sq[k] * inv_c - mean * mean + eps);
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = (__bf16)((s[k][j] - mean) * rstd * wv[j] + bv[j]);
        ((bf16x4 *)out_ln)[(base + k * RPW) * V + pc] = o;
      }
      if constexpr (GATED) {
        rem[k] += 2 * RPW;
        while (rem[k] >= HW) {
          rem[k] -= HW;
          ++bat[k];
        }
      }
    }
  }
}
