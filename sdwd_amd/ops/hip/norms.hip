// Fused normalisation kernels.
//
// group_norm_silu: NCHW GroupNorm with the SiLU folded into the second pass
//   (one kernel instead of GN + act: saves one full HBM round trip of the
//   activation tensor — the UNet/VAE call this before every conv).
//   One 256-thread block per (sample, group); a group's elements are
//   contiguous in NCHW so both passes stream 16 B/lane.
//
// layer_norm: row-wise LN over the last dim (transformer blocks).
//   One block per row batch; fp32 statistics.
//
// channels_last GroupNorm: gn_tile_stats_bf16 (per-128-row-tile partial
//   sums in the conv epilogues' layout; its ADD form is the add_gn entry:
//   a + b plus the sum's partials in one pass), gn_nhwc_stats (finalize),
//   gn_nhwc_norm_bf16 (normalise sweep, per-thread parameters in registers,
//   no index arithmetic per element).
//
// add_layer_norm: residual add + LN, one wave per row, the fp32 row kept in
//   registers (templated on vec8 slices per lane, fully unrolled: no scratch).
#include "common.h"

// ---------------------------------------------------------------------------
// GroupNorm(+SiLU), bf16
// grid.x = N * G   block = 256
// ---------------------------------------------------------------------------
template <bool SILU, bool VEC>
__global__ void group_norm_silu_bf16_kernel(
    const __hip_bfloat16 *__restrict__ x, const float *__restrict__ w,
    const float *__restrict__ b, __hip_bfloat16 *__restrict__ out, int N,
    int C, long HW, int G, float eps) {
  __shared__ float lds[16];
  const int ng = blockIdx.x;
  const int n = ng / G, g = ng % G;
  const int cg = C / G;            // channels per group
  const long len = (long)cg * HW;  // elements per (n, g), contiguous
  const __hip_bfloat16 *base = x + (long)n * C * HW + (long)g * len;
  __hip_bfloat16 *obase = out + (base - x);

  float sum = 0.f, sumsq = 0.f;
  if (VEC) {
    const long nv = len / 8;
    for (long i = threadIdx.x; i < nv; i += blockDim.x) {
      bf16x8 v = ((const bf16x8 *)base)[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = (float)v[j];
        sum += f;
        sumsq += f * f;
      }
    }
  } else {
    for (long i = threadIdx.x; i < len; i += blockDim.x) {
      float f = bf2f(base[i]);
      sum += f;
      sumsq += f * f;
    }
  }
  block_reduce2<256>(sum, sumsq, lds);
  const float mean = sum / (float)len;
  const float var = sumsq / (float)len - mean * mean;
  const float rstd = rsqrtf(var + eps);

  if (VEC) {
    const long nv = len / 8;
    const long hv = HW / 8;  // vectors per channel (HW % 8 == 0 in VEC mode)
    for (long i = threadIdx.x; i < nv; i += blockDim.x) {
      const int c = g * cg + (int)(i / hv);
      const float scale = rstd * w[c];
      const float shift = b[c] - mean * scale;
      bf16x8 v = ((const bf16x8 *)base)[i];
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = (float)v[j] * scale + shift;
        o[j] = (__bf16)(SILU ? silu_f(f) : f);
      }
      ((bf16x8 *)obase)[i] = o;
    }
  } else {
    for (long i = threadIdx.x; i < len; i += blockDim.x) {
      const int c = g * cg + (int)(i / HW);
      float f = (bf2f(base[i]) - mean) * rstd * w[c] + b[c];
      obase[i] = f2bf(SILU ? silu_f(f) : f);
    }
  }
}

// fp32 variant (debug / CPU-parity checks on GPU)
template <bool SILU>
__global__ void group_norm_silu_f32_kernel(const float *__restrict__ x,
                                           const float *__restrict__ w,
                                           const float *__restrict__ b,
                                           float *__restrict__ out, int N,
                                           int C, long HW, int G, float eps) {
  __shared__ float lds[16];
  const int ng = blockIdx.x;
  const int n = ng / G, g = ng % G;
  const int cg = C / G;
  const long len = (long)cg * HW;
  const float *base = x + (long)n * C * HW + (long)g * cg * HW;
  float *obase = out + (base - x);
  float sum = 0.f, sumsq = 0.f;
  for (long i = threadIdx.x; i < len; i += blockDim.x) {
    float f = base[i];
    sum += f;
    sumsq += f * f;
  }
  block_reduce2<256>(sum, sumsq, lds);
  const float mean = sum / (float)len;
  const float rstd = rsqrtf(sumsq / (float)len - mean * mean + eps);
  for (long i = threadIdx.x; i < len; i += blockDim.x) {
    const int c = g * cg + (int)(i / HW);
    float f = (base[i] - mean) * rstd * w[c] + b[c];
    obase[i] = SILU ? silu_f(f) : f;
  }
}

// ---------------------------------------------------------------------------
// LayerNorm over rows [R, D], bf16. One wave per row (D <= a few K).
// block = 256 = 4 waves -> 4 rows per block.
// ---------------------------------------------------------------------------
__global__ void layer_norm_bf16_kernel(const __hip_bfloat16 *__restrict__ x,
                                       const float *__restrict__ w,
                                       const float *__restrict__ b,
                                       __hip_bfloat16 *__restrict__ out,
                                       long R, int D, float eps) {
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const long row = (long)blockIdx.x * 4 + wid;
  if (row >= R) return;
  const __hip_bfloat16 *base = x + row * D;
  __hip_bfloat16 *obase = out + row * D;

  float sum = 0.f, sumsq = 0.f;
  const bool vec = (D % 8) == 0;
  if (vec) {
    const int nv = D / 8;
    for (int i = lane; i < nv; i += WAVE) {
      bf16x8 v = ((const bf16x8 *)base)[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = (float)v[j];
        sum += f;
        sumsq += f * f;
      }
    }
  } else {
    for (int i = lane; i < D; i += WAVE) {
      float f = bf2f(base[i]);
      sum += f;
      sumsq += f * f;
    }
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, WAVE);
    sumsq += __shfl_down(sumsq, off, WAVE);
  }
  sum = __shfl(sum, 0, WAVE);
  sumsq = __shfl(sumsq, 0, WAVE);
  const float mean = sum / D;
  const float rstd = rsqrtf(sumsq / D - mean * mean + eps);

  if (vec) {
    const int nv = D / 8;
    for (int i = lane; i < nv; i += WAVE) {
      bf16x8 v = ((const bf16x8 *)base)[i];
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d = i * 8 + j;
        o[j] = (__bf16)(((float)v[j] - mean) * rstd * w[d] + b[d]);
      }
      ((bf16x8 *)obase)[i] = o;
    }
  } else {
    for (int i = lane; i < D; i += WAVE)
      obase[i] = f2bf((bf2f(base[i]) - mean) * rstd * w[i] + b[i]);
  }
}

__global__ void layer_norm_f32_kernel(const float *__restrict__ x,
                                      const float *__restrict__ w,
                                      const float *__restrict__ b,
                                      float *__restrict__ out, long R, int D,
                                      float eps) {
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const long row = (long)blockIdx.x * 4 + wid;
  if (row >= R) return;
  const float *base = x + row * D;
  float sum = 0.f, sumsq = 0.f;
  for (int i = lane; i < D; i += WAVE) {
    float f = base[i];
    sum += f;
    sumsq += f * f;
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, WAVE);
    sumsq += __shfl_down(sumsq, off, WAVE);
  }
  sum = __shfl(sum, 0, WAVE);
  sumsq = __shfl(sumsq, 0, WAVE);
  const float mean = sum / D;
  const float rstd = rsqrtf(sumsq / D - mean * mean + eps);
  for (int i = lane; i < D; i += WAVE)
    out[row * D + i] = (base[i] - mean) * rstd * w[i] + b[i];
}

// ---------------------------------------------------------------------------
// GroupNorm(+SiLU) for channels_last (NHWC) — the conv-native layout on
// gfx950 (MIOpen NHWC solvers are ~30% faster and need no transposes).
// 3 phases: per-tile per-channel partial sums, per-(n,g) stat finalize,
// fused normalize+SiLU sweep. The first phase usually never runs: the 3x3
// conv epilogues and add_gn emit the same partials as a side channel.
// ---------------------------------------------------------------------------
// Tile-layout statistics: partial[n*tpi + t][2][C] holds, per channel, the
// (sum, sumsq) of the stored bf16 values of rows t*128 .. t*128+127 of image
// n (tpi = ceil(HW/128); the last tile of an image may be short). This is
// the layout the conv epilogues write when HW % 128 == 0.
// grid = (N*tpi, VC/CB), block = 256 laid out as RP = 256/CB row lanes times
// CB vec8 columns (CB divides VC = C/8): every load is 16 B per lane and a
// wave covers whole contiguous row segments. The row lanes are folded
// through LDS in a fixed order, so the result is deterministic.
// ADD: also form a + b (fp32 add, one bf16 rounding: bit-equal to ATen),
// store it to out, and take the statistics over the rounded sums.
template <bool ADD>
__global__ __launch_bounds__(256) void gn_tile_stats_bf16(
    const __hip_bfloat16 *__restrict__ a, const __hip_bfloat16 *__restrict__ b,
    __hip_bfloat16 *__restrict__ out, float *__restrict__ partial, int C,
    long HW, int tpi, int CB) {
  __shared__ float red[256 * 16];  // [ro][sum 0..7 | sumsq 0..7][CB]
  const int tile = blockIdx.x;     // n * tpi + t
  const int n = tile / tpi, t = tile % tpi;
  const int RP = 256 / CB;
  const int tid = threadIdx.x;
  const int ro = tid / CB, vcl = tid % CB;
  const long r0 = (long)t * 128;
  const long r1 = min(HW, r0 + 128);
  if (ro < RP) {
    float s[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.f;
    const long col = ((long)blockIdx.y * CB + vcl) * 8;
    const long base = (long)n * HW * C + col;
    for (long r = r0 + ro; r < r1; r += RP) {
      const long off = base + r * C;
      bf16x8 v = *(const bf16x8 *)(a + off);
      if (ADD) {
        const bf16x8 u = *(const bf16x8 *)(b + off);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = (__bf16)((float)v[j] + (float)u[j]);
        *(bf16x8 *)(out + off) = v;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (float)v[j];
        s[j] += f;
        q[j] += f * f;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[(ro * 16 + j) * CB + vcl] = s[j];
      red[(ro * 16 + 8 + j) * CB + vcl] = q[j];
    }
  }
  __syncthreads();
  const int nch = CB * 8;  // channels of this block's column slab
  float *dst = partial + (long)tile * 2 * C + (long)blockIdx.y * nch;
  for (int e = tid; e < 2 * nch; e += 256) {
    const int kk = e / nch, ch = e % nch;  // kk: 0 = sum, 1 = sumsq
    const float *src = red + (kk * 8 + ch % 8) * CB + ch / 8;
    float acc = 0.f;
    for (int r = 0; r < RP; ++r) acc += src[r * 16 * CB];
    dst[(long)kk * C + ch] = acc;
  }
}

__global__ void gn_nhwc_stats(const float *__restrict__ partial,
                              float *__restrict__ stats,  // [N*G][2]
                              int C, long HW, int G, int S, float eps) {
  const int ng = blockIdx.x;
  const int n = ng / G, g = ng % G;
  const int cg = C / G;
  float sum = 0.f, sumsq = 0.f;
  for (int idx = threadIdx.x; idx < S * cg; idx += WAVE) {
    const int s = idx / cg, c = g * cg + idx % cg;
    const float *p = partial + ((long)n * S + s) * 2 * C;
    sum += p[c];
    sumsq += p[C + c];
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, WAVE);
    sumsq += __shfl_down(sumsq, off, WAVE);
  }
  if (threadIdx.x == 0) {
    const float cnt = (float)(HW * cg);
    const float mean = sum / cnt;
    const float rstd = rsqrtf(sumsq / cnt - mean * mean + eps);
    stats[ng * 2] = mean;
    stats[ng * 2 + 1] = rstd;
  }
}

// Normalise(+SiLU) sweep. grid = N*S: a block covers one sample and one
// contiguous chunk of ceil(HW/S) pixel rows. A thread owns COLS vec8 channel
// columns (COLS = 1: 256/VC row lanes times VC columns; COLS = 2, VC > 256:
// columns tid and tid+256) and loads their 8 mean, rstd, w and b values into
// registers once; the row loop is then one 16 B load, the arithmetic and one
// 16 B store, with no division and no parameter load in it.
// w and b must be 16 B aligned.
template <bool SILU, int COLS>
__global__ __launch_bounds__(256) void gn_nhwc_norm_bf16(
    const __hip_bfloat16 *__restrict__ x, const float *__restrict__ stats,
    const float *__restrict__ w, const float *__restrict__ b,
    __hip_bfloat16 *__restrict__ out, int C, long HW, int G, int S) {
  const int n = blockIdx.x / S, sc = blockIdx.x % S;
  const long chunk = (HW + S - 1) / S;
  const long hw0 = sc * chunk;
  const long hw1 = min(HW, hw0 + chunk);
  const int VC = C / 8, cg = C / G;
  const int tid = threadIdx.x;
  const int RP = COLS == 1 ? 256 / VC : 1;
  const int ro = COLS == 1 ? tid / VC : 0;
  const int vc0 = COLS == 1 ? tid % VC : tid;
  if (ro >= RP) return;

  float mean[COLS][8], rstd[COLS][8], wv[COLS][8], bv[COLS][8];
#pragma unroll
  for (int k = 0; k < COLS; ++k) {
    const int vc = vc0 + k * 256;
    if (vc < VC) {
      const f32x4 w0 = ((const f32x4 *)w)[vc * 2];
      const f32x4 w1 = ((const f32x4 *)w)[vc * 2 + 1];
      const f32x4 b0 = ((const f32x4 *)b)[vc * 2];
      const f32x4 b1 = ((const f32x4 *)b)[vc * 2 + 1];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int g = (vc * 8 + j) / cg;
        mean[k][j] = stats[((long)n * G + g) * 2];
        rstd[k][j] = stats[((long)n * G + g) * 2 + 1];
        wv[k][j] = j < 4 ? w0[j & 3] : w1[j & 3];
        bv[k][j] = j < 4 ? b0[j & 3] : b1[j & 3];
      }
    }
  }
  const bf16x8 *px = (const bf16x8 *)(x + (long)n * HW * C);
  bf16x8 *po = (bf16x8 *)(out + (long)n * HW * C);
  for (long hw = hw0 + ro; hw < hw1; hw += RP) {
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
      const int vc = vc0 + k * 256;
      if (vc < VC) {
        const bf16x8 v = px[hw * VC + vc];
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = ((float)v[j] - mean[k][j]) * rstd[k][j] * wv[k][j] +
                    bv[k][j];
          o[j] = (__bf16)(SILU ? silu_f(f) : f);
        }
        po[hw * VC + vc] = o;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Fused residual-add + LayerNorm: sum = x + res; ln = LN(sum)*w + b.
// The transformer pre-norm chain needs both tensors; fusing saves one full
// HBM round trip per residual. One wave per row; a lane holds its NV vec8
// slices of the fp32 sum in registers between the statistics and the
// normalise step (NV = 1, 2, 3 covers D <= 512, 1024, 1536). Both loops are
// fully unrolled so the staged values have compile-time indices: no scratch.
// w and b must be 16 B aligned.
// GATHER (token merging's unmerge folded in): r is [B, M, D] and row t of
// batch row bb adds r[bb, slot[bb*N + t]]; the entry is clamped to [0, M).
// Without GATHER the three trailing arguments are unused.
// ---------------------------------------------------------------------------
template <int NV, bool GATHER = false>
__global__ __launch_bounds__(256) void add_layer_norm_bf16_kernel(
    const __hip_bfloat16 *__restrict__ x, const __hip_bfloat16 *__restrict__ r,
    const float *__restrict__ w, const float *__restrict__ b,
    __hip_bfloat16 *__restrict__ out_sum, __hip_bfloat16 *__restrict__ out_ln,
    long R, int D, float eps, const int *__restrict__ slot, int N, int M) {
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const long row = (long)blockIdx.x * 4 + wid;
  if (row >= R) return;
  const int nv = D / 8;  // D % 8 == 0 and nv <= NV * WAVE by dispatch
  const bf16x8 *xb = (const bf16x8 *)(x + row * D);
  long rrow = row;
  if constexpr (GATHER) {
    int s = slot[row];
    s = s < 0 ? 0 : (s >= M ? M - 1 : s);
    rrow = (row / N) * M + s;
  }
  const bf16x8 *rb = (const bf16x8 *)(r + rrow * D);
  bf16x8 *sb = (bf16x8 *)(out_sum + row * D);
  bf16x8 *lb = (bf16x8 *)(out_ln + row * D);

  float vals[NV][8];
  float sum = 0.f, sumsq = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = lane + k * WAVE;
    if (i < nv) {
      const bf16x8 vx = xb[i];
      const bf16x8 vr = rb[i];
      bf16x8 vs;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (float)vx[j] + (float)vr[j];
        vals[k][j] = f;
        sum += f;
        sumsq += f * f;
        vs[j] = (__bf16)f;
      }
      sb[i] = vs;
    }
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, WAVE);
    sumsq += __shfl_down(sumsq, off, WAVE);
  }
  sum = __shfl(sum, 0, WAVE);
  sumsq = __shfl(sumsq, 0, WAVE);
  const float mean = sum / D;
  const float rstd = rsqrtf(sumsq / D - mean * mean + eps);

#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = lane + k * WAVE;
    if (i < nv) {
      const f32x4 w0 = ((const f32x4 *)w)[i * 2];
      const f32x4 w1 = ((const f32x4 *)w)[i * 2 + 1];
      const f32x4 b0 = ((const f32x4 *)b)[i * 2];
      const f32x4 b1 = ((const f32x4 *)b)[i * 2 + 1];
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float wj = j < 4 ? w0[j & 3] : w1[j & 3];
        const float bj = j < 4 ? b0[j & 3] : b1[j & 3];
        o[j] = (__bf16)((vals[k][j] - mean) * rstd * wj + bj);
      }
      lb[i] = o;
    }
  }
}
