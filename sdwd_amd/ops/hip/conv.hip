// Implicit-GEMM 3x3 convolution for gfx950, NHWC (channels_last), bf16.
//
// GEMM view: C[M=N*Ho*Wo, Cout] = A[M, K=9*Cin] x B[K, Cout]; A is the
// implicit im2col of the activations (per-(dy,dx)-plane address offsets are
// constant across pixels, so each staged row caches its base address once),
// B is the weight in [Cout][3][3][Cin] (torch channels_last) layout.
//
// v2 structure (guide §5 step-3 + 'glds, 2 LDS buffers' row):
//  * 128x128 tile, BK=64; 4 waves in 2x2, each wave a 64x64 sub-tile as
//    4x4(x2 k-sub) mfma_f32_16x16x32_bf16;
//  * A/B tiles staged by global_load_lds (16 B/lane direct-to-LDS DMA),
//    double-buffered in ONE __shared__ array (a second __shared__ object
//    makes hipcc drain vmcnt before every ds_read - guide §5 trap (a));
//  * tile t+1's 8 DMA instructions stay in flight across the barrier:
//    raw s_barrier + counted `s_waitcnt vmcnt(8)` (a plain __syncthreads
//    would drain the pipeline);
//  * LDS rows are 128 B; the 8 16-B chunks are XOR-permuted by (row>>1)&7
//    applied to the DMA *source* address (rule 21: the glds destination is
//    lane-linear) so the b128 fragment reads are bank-conflict-free;
//  * padding rows ride a 64-B zero page (glds is wave-uniform, lanes with
//    out-of-image taps just read zeros);
//  * WRAP instantiations (seamless tiling) instead fold an out-of-image
//    tap back onto the opposite border, per axis (wrap_h / wrap_w): only
//    the DMA source address differs, an unwrapped axis keeps the zero page;
//  * FOLD instantiations run conv(nearest2x(x)) as four 2x2 sub-pixel convs
//    on the source image with pre-summed weights (K = 4*Cin, not 9*Cin);
//  * bias, per-(sample,channel) bias (time embedding) and the ResBlock
//    residual add are fused into the epilogue;
//  * the epilogue of a full tile is vectorised (conv_epi_strip in
//    conv_epilogue.h): operands fetched ahead of use, the rounded bf16 sub-tile transposed
//    through wave-private LDS (free after the K loop), 16-byte stores of 8
//    channels per lane. Edge tiles, cols % 8 != 0 and unaligned outputs keep
//    the element-wise path; both compute the same bits. The bias is read as
//    stored (bf16 or fp32).
//
// Requirements: Cin % 64 == 0 (every SD1.5/SDXL/VAE hot shape; the small-Cin
// stem convs go to conv_small.hip), any Cout, stride 1 or 2, pad 1, kernel 3x3.
#include "common.h"
#include "conv_epilogue.h"
#include <map>
#include <mutex>
#include <tuple>

typedef __attribute__((ext_vector_type(4))) float f32x4c;

#define CONV_BM 128
#define CONV_BN 128
#define CONV_BK 64
#define TILE_ELEMS (CONV_BM * CONV_BK)  // per operand per buffer

// XOR-permute the 8 16-byte chunks of a 128-byte LDS row: a b128 fragment
// read's 16-lane group touches 16 consecutive rows at one chunk; rows of
// equal parity would collide every 2 rows at a 32-dword stride, so spread
// by (row>>1)&7.
// cswz() lives in conv_v4.hip (included first)

// BN = 128 (default) or 64 (exact tiling for Cout % 128 == 64, e.g. the
// SD1.5 320-channel level: 5 exact 64-col tiles instead of 3 x 128 with a
// 17% masked-FLOP tail). NJ = column fragments per wave.
// UPS: the input is a VIRTUAL nearest-2x upsample of X (H/W are the REAL
// input dims, Ho/Wo the upsampled-output dims): tap (h,w) of the virtual
// image reads X[h>>1][w>>1], fusing Upsample+conv into one kernel with no
// 4x intermediate tensor.
// WRAP: "may wrap" - the border taps of an axis whose wrap_h / wrap_w flag is
// set read the opposite border instead of the zero page (on the virtual
// 2H x 2W grid for UPS). WRAP=false compiles the flags away.
// FOLD: the same fused upsample+conv as UPS, computed as four 2x2 sub-pixel
// convs on the SOURCE image. The 3 virtual rows (columns) a 3x3 window
// touches come from 2 source rows (columns), so output phase
// p = 2a + b = 2(oh&1) + (ow&1) is a 2x2 conv whose weights are sums of the
// 3x3 weights: Wt is the folded [4][Cout][2][2][Cin] (fold_ups2x_weight).
// GEMM rows are the N*H*W source pixels of ONE phase, K = 4*Cin (2.25x
// fewer FLOPs than UPS); M-tile index = 4*(tile in phase) + p, so the four
// phases of a source tile are dispatched together and share A in L2. Tap
// (r,s) of source pixel (i,j) reads X[i-1+a+r][j-1+b+s]: the plain
// addressing with a shifted base, so zero padding and WRAP (on the source
// grid, which equals wrapping the virtual one) are the non-UPS code paths.
template <bool HAS_BIAS, bool HAS_RES, bool HAS_CB, int BN = 128,
          bool UPS = false, bool WRAP = false, bool FOLD = false>
__launch_bounds__(256, 2) __global__ void conv3x3_nhwc_bf16_kernel(
    const __hip_bfloat16 *__restrict__ X,   // [N,H,W,Cin]
    const __hip_bfloat16 *__restrict__ Wt,  // [Cout,3,3,Cin]
    const void *__restrict__ bias,          // [Cout] fp32 or bf16 (flags),
                                            // or null
    const __hip_bfloat16 *__restrict__ Res, // [N,Ho,Wo,Cout] or null
    const __hip_bfloat16 *__restrict__ CB,  // [N,Cout] or null
    const __hip_bfloat16 *__restrict__ Zero,// >=16B of zeros
    __hip_bfloat16 *__restrict__ Y,         // [N,Ho,Wo,ldY] (+col offset)
    int Nn, int H, int W, int Cin, int Cout, int Ho, int Wo, int stride,
    int ldY, int flags, float *__restrict__ GNP = nullptr, int wrap_h = 0,
    int wrap_w = 0) {
  // GNP != null: emit per-(M-tile, channel) partial (sum, sumsq) of the
  // STORED values into GNP[mtile][2][ldY] so GroupNorm's stats pass can
  // skip its full-tensor read (host enables only when Ho*Wo % BM == 0,
  // i.e. every tile lies inside one image). Deterministic: wave shfl
  // reduce + fixed-order cross-wave combine (no atomics).
  // one __shared__ object: [buf0: A(8K elems) B(8K)][buf1: A B]
  __shared__ __align__(16) __bf16 smem[4 * TILE_ELEMS];

  static_assert(!(UPS && FOLD) && !(FOLD && (HAS_RES || HAS_CB)));
  const long M = FOLD ? (long)Nn * H * W : (long)Nn * Ho * Wo;
  // grid: x = Cout tiles, y (+z overflow) = M tiles, so consecutively-
  // dispatched blocks are the column tiles of ONE row tile and share its
  // A reads in L2/L3
  constexpr int NJ = BN / 32;          // 4 or 2 column fragments per wave
  constexpr int BTILE = BN * CONV_BK;  // B-tile elements
  // FOLD: M-tile index = 4 * (tile in phase) + 2a + b
  const int fa = FOLD ? (blockIdx.y >> 1) & 1 : 0;  // output row phase
  const int fb = FOLD ? blockIdx.y & 1 : 0;         // output column phase
  const long m0 =
      (((long)blockIdx.y + (long)blockIdx.z * 32768) >> (FOLD ? 2 : 0)) *
      CONV_BM;
  if constexpr (FOLD) {
    // a grid spilling into z rounds the tile count up: nothing to do there
    // (and no partial slot to write)
    if (m0 >= M) return;
  }
  const int n0 = blockIdx.x * BN;

  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wid = tid / WAVE;
  const int wm = (wid >> 1) * 64;
  const int wn = (wid & 1) * (BN / 2);

  // ---- per-lane DMA row bookkeeping -------------------------------------
  // stage instr i (0..3) per wave writes LDS bytes
  // [i*4096 + wid*1024 + lane*16]; linear row = byte/128:
  //   row_i = i*32 + wid*8 + lane/8, chunk = lane%8 (then source-swizzled)
  long abase[4];
  int hs[4], ws[4];   // ho*stride, wo*stride per staged A row
  int bco[4];         // cout row per staged B row (NB instrs used)
  constexpr int NB = BN / 32;  // B stage instrs (rows BN over 4 waves x 8)
  int nimg[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = i * 32 + wid * 8 + lane / 8;
    const long m = m0 + row;
    const long mm = (m < M) ? m : (M - 1);
    if constexpr (FOLD) {
      // mm is the source pixel's linear index; (hs, ws) = its tap (0,0)
      const unsigned q = (unsigned)mm / (unsigned)W;  // n*H + i (host: int)
      hs[i] = (int)(q % (unsigned)H) - 1 + fa;
      ws[i] = (int)((unsigned)mm - q * (unsigned)W) - 1 + fb;
      nimg[i] = 0;
      abase[i] = (mm + (long)(fa - 1) * W + (fb - 1)) * Cin;
    } else {
      const int n_img = (int)(mm / ((long)Ho * Wo));
      const int rem = (int)(mm % ((long)Ho * Wo));
      hs[i] = (rem / Wo) * stride;
      ws[i] = (rem % Wo) * stride;
      nimg[i] = n_img;
      abase[i] = (((long)n_img * H + hs[i]) * W + ws[i]) * Cin;
    }
    bco[i] = n0 + row;
  }
  const int schunk = lane % 8;

  const int kc_per_plane = Cin / CONV_BK;
  const int NT = (FOLD ? 4 : 9) * kc_per_plane;
  // WRAP: what folding a tap back adds to its address (host checks int)
  const int row_elems = W * Cin, img_elems = H * row_elems;
  (void)row_elems;
  (void)img_elems;

  // stage tile t into buffer b (8 glds: 4 A + 4 B)
  auto stage = [&](int t, int b) {
    const int plane = t / kc_per_plane;
    const int kc = t % kc_per_plane;
    // FOLD: plane = 2r + s, the tap offset from (hs, ws) is (r, s)
    const int dy = FOLD ? plane >> 1 : plane / 3 - 1;
    const int dx = FOLD ? plane & 1 : plane % 3 - 1;
    const long poff = ((long)dy * W + dx) * Cin + (long)kc * CONV_BK;
    __bf16 *abuf = smem + b * (TILE_ELEMS + BTILE);
    __bf16 *bbuf = abuf + TILE_ELEMS;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = i * 32 + wid * 8 + lane / 8;
      const int sc = cswz(row, schunk);
      bool av;
      const __hip_bfloat16 *asrc;
      if constexpr (WRAP && UPS) {
        // wrap on the virtual 2H x 2W grid, then >> 1. |dy|,|dx| <= 1, so
        // one conditional add per side folds the tap back
        int vh = hs[i] + dy, vw = ws[i] + dx;
        if (wrap_h) {
          vh += vh < 0 ? 2 * H : 0;
          vh -= vh >= 2 * H ? 2 * H : 0;
        }
        if (wrap_w) {
          vw += vw < 0 ? 2 * W : 0;
          vw -= vw >= 2 * W ? 2 * W : 0;
        }
        // a wrapped axis is in range by now: only unwrapped axes can fail
        av = vh >= 0 && vh < 2 * H && vw >= 0 && vw < 2 * W;
        asrc = av ? (X +
                     (((long)nimg[i] * H + (vh >> 1)) * W + (vw >> 1)) *
                         Cin +
                     (long)kc * CONV_BK + sc * 8)
                  : Zero;
      } else if constexpr (WRAP) {
        // (nimg, hh, ww) with hh = hs + dy folded back by one conditional
        // add per side (|dy| <= 1, a stride-2 tap never passes the dim; also
        // right at dim == 1) is abase + poff plus a whole image height or
        // width: form that delta instead of redoing the 64-bit multiplies
        const int hh = hs[i] + dy, ww = ws[i] + dx;
        int dlt = 0;
        if (wrap_h) dlt += hh < 0 ? img_elems : (hh >= H ? -img_elems : 0);
        if (wrap_w) dlt += ww < 0 ? row_elems : (ww >= W ? -row_elems : 0);
        // the tap is valid iff every UNWRAPPED axis is in range
        av = (wrap_h || (hh >= 0 && hh < H)) &&
             (wrap_w || (ww >= 0 && ww < W));
        asrc = av ? (X + abase[i] + poff + dlt + sc * 8) : Zero;
      } else if constexpr (UPS) {
        const int vh = hs[i] + dy, vw = ws[i] + dx;  // virtual 2H x 2W
        av = vh >= 0 && vh < 2 * H && vw >= 0 && vw < 2 * W;
        asrc = av ? (X +
                     (((long)nimg[i] * H + (vh >> 1)) * W + (vw >> 1)) *
                         Cin +
                     (long)kc * CONV_BK + sc * 8)
                  : Zero;
      } else {
        av = (hs[i] + dy >= 0) && (hs[i] + dy < H) &&
             (ws[i] + dx >= 0) && (ws[i] + dx < W);
        asrc = av ? (X + abase[i] + poff + sc * 8) : Zero;
      }
      (void)poff;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int *)asrc,
          (__attribute__((address_space(3))) unsigned int
               *)(abuf + i * 2048 + wid * 512),
          16, 0, 0);
      if (i < NB) {
        const bool bv = bco[i] < Cout;
        const __hip_bfloat16 *bsrc;
        if constexpr (FOLD) {
          // phase p's [Cout][2][2][Cin] matrix (Cout = all columns)
          bsrc = bv ? (Wt +
                       (((long)(2 * fa + fb) * Cout + bco[i]) * 4 + plane) *
                           Cin +
                       kc * CONV_BK + sc * 8)
                    : Zero;
        } else {
          bsrc = bv ? (Wt + (long)bco[i] * 9 * Cin + plane * Cin +
                       kc * CONV_BK + sc * 8)
                    : Zero;
        }
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int *)bsrc,
            (__attribute__((address_space(3))) unsigned int
                 *)(bbuf + i * 2048 + wid * 512),
            16, 0, 0);
      }
    }
  };

  f32x4c acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4c){};

  stage(0, 0);
  if (NT > 1) stage(1, 1);

  const int l16 = lane % 16;
  const int kq = (lane / 16) * 8;  // k offset of this lane's 8 elements

  for (int t = 0; t < NT; ++t) {
    // current tile's DMAs landed; the next tile's stay in flight
    if (t + 1 < NT)
      asm volatile("s_waitcnt vmcnt(%0)" :: "i"(4 + NB) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    const __bf16 *abuf = smem + (t & 1) * (TILE_ELEMS + BTILE);
    const __bf16 *bbuf = abuf + TILE_ELEMS;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 af[4], bf[NJ];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int am = wm + i * 16 + l16;
        const int ck = cswz(am, (s * 32 + kq) / 8);
        af[i] = *(const bf16x8 *)((const char *)(abuf + am * CONV_BK) +
                                  ck * 16);
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int bn = wn + j * 16 + l16;
        const int ck = cswz(bn, (s * 32 + kq) / 8);
        bf[j] = *(const bf16x8 *)((const char *)(bbuf + bn * CONV_BK) +
                                  ck * 16);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[i], bf[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    __builtin_amdgcn_s_barrier();  // everyone done reading this buffer
    if (t + 2 < NT) stage(t + 2, t & 1);
  }

  // ---- epilogue: bias, channel-bias, residual, store --------------------
  // Full tiles of a launch the host cleared (flags & CONV_F_VEC) take the
  // vector path, conv_epi_strip in conv_epilogue.h: operands fetched ahead of
  // use, the bf16 sub-tile transposed through wave-private LDS, 16-byte
  // stores. Edge tiles and unaligned launches keep the element-wise path.
  // The arithmetic and the GroupNorm partial order are the same in both.
  const int r4 = (lane / 16) * 4;
  float gs[NJ], gq[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) gs[j] = gq[j] = 0.0f;
  const bool full =
      (flags & CONV_F_VEC) && m0 + CONV_BM <= M && n0 + BN <= Cout;
  if (full) {
    // the wave's coordinates as scalars: bases stay in SGPRs and the loads
    // and stores address as base + 32-bit lane offset
    const int uw = __builtin_amdgcn_readfirstlane(wid);
    const int uwm = (uw >> 1) * 64, uwn = (uw & 1) * (BN / 2);
    float bv[NJ], cbv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      bv[j] = HAS_BIAS ? conv_bias_at(bias, flags, n0 + uwn + j * 16 + l16)
                       : 0.0f;
      cbv[j] = 0.0f;
    }
    const unsigned HoWo = (unsigned)(Ho * Wo);  // host: fits
    bool cb_one = true;
    unsigned rem0 = 0;
    const __hip_bfloat16 *cbw = nullptr;
    if constexpr (HAS_CB) {
      const long ni0 = m0 / (long)HoWo;  // block-uniform, once
      const unsigned remb = (unsigned)(m0 - ni0 * (long)HoWo);
      cb_one = remb + CONV_BM <= HoWo;
      rem0 = remb + uwm;
      cbw = CB + ni0 * (long)ldY + n0 + uwn;
#pragma unroll
      for (int j = 0; j < NJ; ++j) cbv[j] = (float)cbw[j * 16 + l16];
    }
    const long mw = m0 + uwm;
    const __hip_bfloat16 *resw =
        HAS_RES ? Res + mw * (long)ldY + n0 + uwn : nullptr;
    __hip_bfloat16 *yw =
        FOLD ? Y + n0 + uwn : Y + mw * (long)ldY + n0 + uwn;
    // wave-private regions: disjoint from each other and from the
    // GroupNorm staging below, so no barrier anywhere in here
    char *wl = (char *)smem + wid * conv_epi_bytes<NJ>;
    if (cb_one)
      conv_epi_strip<HAS_RES, HAS_CB, true, FOLD, NJ, false>(
          acc, bv, cbv, cbw, rem0, HoWo, resw, yw, mw, W, Wo, fa, fb,
          (unsigned)ldY, wl, lane, gs, gq);
    else
      conv_epi_strip<HAS_RES, HAS_CB, false, FOLD, NJ, false>(
          acc, bv, cbv, cbw, rem0, HoWo, resw, yw, mw, W, Wo, fa, fb,
          (unsigned)ldY, wl, lane, gs, gq);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int co = n0 + wn + j * 16 + l16;
        if (co >= Cout) continue;
        const float bv = HAS_BIAS ? conv_bias_at(bias, flags, co) : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          long m = m0 + wm + i * 16 + r4 + r;
          if (m >= M) continue;
          if constexpr (FOLD) {
            // source pixel (n, i, j) -> output row (n, 2i+a, 2j+b); with
            // q = n*H + i, n*Ho + 2i is 2q
            const unsigned q = (unsigned)m / (unsigned)W;
            const unsigned jw = (unsigned)m - q * (unsigned)W;
            m = (long)(2 * q + fa) * Wo + 2 * jw + fb;
          }
          float v = acc[i][j][r] + bv;
          if (HAS_CB) {
            const int ni = (int)(m / ((long)Ho * Wo));
            v += (float)CB[(long)ni * ldY + co];
          }
          if (HAS_RES) v += (float)Res[m * ldY + co];
          const __hip_bfloat16 vb = f2bf(v);
          Y[m * ldY + co] = vb;
          if (GNP) {
            const float vr = bf2f(vb);  // stats over the STORED values
            gs[j] += vr;
            gq[j] += vr * vr;
          }
        }
      }
    }
  }
  if (GNP) {
    // wave reduce: fold the 4 lane-quarters holding one column. Staged past
    // the four wave-private epilogue regions, which other waves may still
    // be transposing through (the staging LDS is free after the k-loop)
    float *lds = (float *)((char *)smem + 4 * conv_epi_bytes<4>);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
      for (int off = 16; off < 64; off <<= 1) {
        gs[j] += __shfl_down(gs[j], off, WAVE);
        gq[j] += __shfl_down(gq[j], off, WAVE);
      }
      // lanes 0..15 hold the wave's column sums -> LDS [wid][j][l16][2]
      if (lane < 16) {
        float *slot = lds + ((wid * NJ + j) * 16 + lane) * 2;
        slot[0] = gs[j];
        slot[1] = gq[j];
      }
    }
    __syncthreads();
    // fixed-order cross-wave combine: col c's two waves are
    // {c/(BN/2), +2} (wave grid 2Mx2N); one thread per column writes
    // FOLD (host enables only when H*W % BM == 0): a tile lies in one
    // (image, phase); the image's Ho*Wo/BM slots are [phase][tile], any
    // partition of its pixels serves gn_nhwc_stats
    long gslot = (long)blockIdx.y + (long)blockIdx.z * 32768;
    if constexpr (FOLD) {
      const long tps = ((long)H * W) / CONV_BM, tp = gslot >> 2;
      gslot = ((tp / tps) * 4 + (gslot & 3)) * tps + tp % tps;
    }
    for (int c = tid; c < BN; c += 256) {
      const int co = n0 + c;
      if (co >= Cout) continue;
      const int h = c / (BN / 2);
      const int jj = (c % (BN / 2)) / 16;
      const int lc = c % 16;
      const float *s0 = lds + ((h * NJ + jj) * 16 + lc) * 2;
      const float *s1 = lds + (((h + 2) * NJ + jj) * 16 + lc) * 2;
      float *dst = GNP + (gslot * 2) * (long)ldY;
      dst[co] = s0[0] + s1[0];
      dst[ldY + co] = s0[1] + s1[1];
    }
  }
}

// ---------------------------------------------------------------------------
#ifdef __HIP_PLATFORM_AMD__
bool conv3x3_supported(long cin) { return cin % 64 == 0 && cin >= 64; }

// Which kernel serves which output columns: {number of full 256-column
// tiles on the v4 kernel, remainder columns on the v2 kernel, remainder
// uses BN=64 (false when there is no remainder)}. force: 0 = measured
// policy, 2 = v2 everywhere, 4 = v4 on every legal shape (A/B tooling).
// The launcher below follows this and nothing else decides.
std::tuple<long, long, bool> conv3x3_plan(long N, long H, long W, long Cin,
                                          long Cout, long stride,
                                          long force) {
  const long Ho = (H + 2 - 3) / stride + 1;
  const long Wo = (W + 2 - 3) / stride + 1;
  const long M = N * Ho * Wo;
  const long mtiles = (M + CONV_BM - 1) / CONV_BM;
  const long mt4 = (M + V4_BM - 1) / V4_BM;
  // measured winners (profiles/r02_conv_family.md): the 256x256 pipeline
  // wins on the SD-UNet level-0/1 shapes (Cin<=960, Cout<=640, big M) and
  // — since the phase-0 stage-8 schedule — the VAE 512-ch shapes too
  // (+7-12%); the 1280-channel shapes stay on v2 (2 blocks/CU beats the
  // deep pipeline there: 737-765 vs 814-822 TF/s forced).
  // ... and only when the 512-thread 1-block/CU grid actually fills the
  // 256 CUs (small shards at N=8 under-fill 256-row tiles: the 128-row
  // v2 kernel at 2 blocks/CU wins there)
  const bool v4_shape =
      force == 4 ? (Cin % 64 == 0 && Cout >= 256)
                 : (Cin <= 960 && Cout <= 640 && Cout >= 256 &&
                    mt4 * (Cout / 256) >= 256);
  const long nfull = (force == 2 || !v4_shape) ? 0 : Cout / 256;
  const long rem = Cout - nfull * 256;
  // BN=64 when the remainder is one 64-tile OR when the BN=128 grid
  // would under-fill the 256 CUs (small shards: twice the blocks beat
  // the halved B-reuse when occupancy-starved)
  const bool bn64 =
      rem > 0 && (rem <= 64 || mtiles * ((rem + 127) / 128) < 512);
  return {nfull, rem, bn64};
}

// The padding rows' zero page: one 64-element tensor per device ordinal,
// created on first use and kept for the life of the process.
static const __hip_bfloat16 *zero_page_for(const torch::Tensor &x) {
  static std::mutex mu;
  static std::map<int, torch::Tensor> pages;
  std::lock_guard<std::mutex> lock(mu);
  auto &page = pages[x.get_device()];
  if (!page.defined()) page = torch::zeros({64}, x.options());
  return (const __hip_bfloat16 *)page.data_ptr();
}

// Call f with one std::bool_constant per runtime bool, so a generic lambda
// can name the kernel instantiation: dispatch_bools(f, a, b) ends in
// f(bool_constant<a>{}, bool_constant<b>{}).
template <class F>
static void dispatch_bools(F &&f) {
  f();
}
template <class F, class... Rest>
static void dispatch_bools(F &&f, bool b, Rest... rest) {
  if (b)
    dispatch_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
  else
    dispatch_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

// M tiles ride grid y, with the overflow past 32768 in z
static dim3 conv_grid(long col_tiles, long mtiles) {
  return dim3((unsigned)col_tiles, (unsigned)std::min<long>(mtiles, 32768),
              (unsigned)((mtiles + 32767) / 32768));
}

// What the plain and the fused-upsample entry share: checks, output and
// GroupNorm-partial allocation, and the operand pointers. The tensors are
// members so a converted bias / bf16 chan-bias copy outlives the launch call.
// A contiguous bf16 or fp32 bias is read by the kernels as it is stored.
struct ConvArgs {
  int N, Cin, H, W, Cout, Ho, Wo;
  long M;
  torch::Tensor y, gnp, bias_f32, cb_bf16;
  const __hip_bfloat16 *x, *w, *res = nullptr, *cb = nullptr, *zero;
  const char *bias = nullptr;
  int bias_esize = 4;  // bytes per bias element: 4 (fp32) or 2 (bf16)
  __hip_bfloat16 *yp;
  float *gnp_ptr = nullptr;

  // bias pointer of the launch that starts at output column co0
  const void *bias_at(long co0) const {
    return bias ? bias + co0 * bias_esize : nullptr;
  }
  // kernel `flags` of the launch that writes `cols` columns from co0: the
  // vector epilogue stores 16 B = 8 channels per lane, so rows and the
  // column offset must keep Y 16-byte aligned (Res and CB are read by
  // element and need nothing)
  int flags(long co0, long cols) const {
    const bool vec = cols % 8 == 0 && Cout % 8 == 0 &&
                     (reinterpret_cast<uintptr_t>(yp + co0) & 15) == 0;
    return (vec ? CONV_F_VEC : 0) | (bias_esize == 2 ? CONV_F_BIAS_BF16 : 0);
  }

  // x: [N,C,H,W] channels_last; w_prep: [Cout,3,3,Cin] contiguous
  ConvArgs(const torch::Tensor &xt, const torch::Tensor &w_prep,
           const c10::optional<torch::Tensor> &bias_t,
           const c10::optional<torch::Tensor> &residual,
           const c10::optional<torch::Tensor> &chan_bias, int Ho_, int Wo_,
           bool collect_gn)
      : N(xt.size(0)), Cin(xt.size(1)), H(xt.size(2)), W(xt.size(3)),
        Cout(w_prep.size(0)), Ho(Ho_), Wo(Wo_), M((long)N * Ho_ * Wo_) {
    TORCH_CHECK(xt.is_contiguous(torch::MemoryFormat::ChannelsLast),
                "conv3x3: x must be channels_last");
    TORCH_CHECK(xt.scalar_type() == torch::kBFloat16);
    TORCH_CHECK(conv3x3_supported(Cin), "conv3x3: Cin % 64 != 0");
    y = torch::empty({N, Cout, Ho, Wo},
                     xt.options().memory_format(
                         torch::MemoryFormat::ChannelsLast));
    x = (const __hip_bfloat16 *)xt.data_ptr();
    w = (const __hip_bfloat16 *)w_prep.data_ptr();
    yp = (__hip_bfloat16 *)y.data_ptr();
    zero = zero_page_for(xt);
    // the vector epilogue's 32-bit offsets: up to 256 rows of ldY elements
    // within a tile, and a row's index within its image
    TORCH_CHECK(Cout < (1 << 20), "conv3x3: too many output channels");
    TORCH_CHECK((long)Ho * Wo < (1L << 30), "conv3x3: output image too large");
    if (bias_t.has_value()) {
      TORCH_CHECK(bias_t->numel() == Cout, "conv3x3: bias must be [Cout]");
      const auto bt = bias_t->scalar_type();
      if ((bt == torch::kBFloat16 || bt == torch::kFloat) &&
          bias_t->is_contiguous()) {
        bias_f32 = *bias_t;  // no copy: the kernels read either type
        bias_esize = bt == torch::kBFloat16 ? 2 : 4;
      } else {
        bias_f32 = bias_t->to(torch::kFloat).contiguous();
      }
      bias = (const char *)bias_f32.data_ptr();
    }
    if (residual.has_value()) {
      TORCH_CHECK(
          residual->is_contiguous(torch::MemoryFormat::ChannelsLast));
      res = (const __hip_bfloat16 *)residual->data_ptr();
    }
    if (chan_bias.has_value()) {
      cb_bf16 = chan_bias->to(torch::kBFloat16).contiguous();
      cb = (const __hip_bfloat16 *)cb_bf16.data_ptr();
    }
    // GroupNorm partial side-channel (one (sum,sumsq) pair per 128-row
    // tile per channel): only when every 128-row tile lies inside one image
    if (collect_gn && ((long)Ho * Wo) % 128 == 0) {
      gnp = torch::empty({M / 128, 2, (long)Cout},
                         xt.options().dtype(torch::kFloat));
      gnp_ptr = gnp.data_ptr<float>();
    }
  }

  std::tuple<torch::Tensor, c10::optional<torch::Tensor>> result() const {
    if (gnp.defined()) return {y, gnp};
    return {y, c10::nullopt};
  }
};

// returns (y, GroupNorm partials or None)
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> conv3x3_nhwc(
    torch::Tensor x, torch::Tensor w_prep, c10::optional<torch::Tensor> bias,
    c10::optional<torch::Tensor> residual,
    c10::optional<torch::Tensor> chan_bias, long stride, bool collect_gn,
    long force, bool wrap_h = false, bool wrap_w = false) {
  const int Ho = (x.size(2) + 2 - 3) / stride + 1;
  const int Wo = (x.size(3) + 2 - 3) / stride + 1;
  ConvArgs a(x, w_prep, bias, residual, chan_bias, Ho, Wo, collect_gn);
  auto stream = cur_stream();
  // wrap-around padding (seamless tiling) picks the "may wrap"
  // instantiation of whichever kernel the plan names; the plan is the same
  const bool wrap = wrap_h || wrap_w;
  TORCH_CHECK(!wrap || (long)a.H * a.W * a.Cin < (1L << 31),
              "conv3x3: wrapped image too large");
  // v4: the 256x256 8-phase deep pipeline serves full 256-column tiles;
  // the v2 128-tile kernel covers the Cout remainder (e.g. 320 = 256+64).
  const auto [nfull, rem, bn64] =
      conv3x3_plan(a.N, a.H, a.W, a.Cin, a.Cout, stride, force);
  if (nfull > 0) {
    const int cols = (int)(nfull * 256);
    dispatch_bools(
        [&, cols](auto B, auto R, auto C, auto WR) {
          hipLaunchKernelGGL(
              (conv3x3_v4_kernel<decltype(B)::value, decltype(R)::value,
                                 decltype(C)::value, decltype(WR)::value>),
              conv_grid(cols / 256, (a.M + V4_BM - 1) / V4_BM), dim3(512), 0,
              stream, a.x, a.w, a.bias_at(0), a.res, a.cb, a.zero, a.yp, a.N,
              a.H, a.W, a.Cin, cols, a.Cout, a.Ho, a.Wo, (int)stride,
              a.flags(0, cols), a.gnp_ptr, (int)wrap_h, (int)wrap_w);
        },
        a.bias != nullptr, a.res != nullptr, a.cb != nullptr, wrap);
  }
  if (rem > 0) {
    const long co0 = nfull * 256;
    const int cols = (int)rem;
    dispatch_bools(
        [&, co0, cols](auto B, auto R, auto C, auto N64, auto WR) {
          constexpr int BN = decltype(N64)::value ? 64 : 128;
          hipLaunchKernelGGL(
              (conv3x3_nhwc_bf16_kernel<decltype(B)::value,
                                        decltype(R)::value,
                                        decltype(C)::value, BN, false,
                                        decltype(WR)::value>),
              conv_grid((cols + BN - 1) / BN,
                        (a.M + CONV_BM - 1) / CONV_BM),
              dim3(256), 0, stream, a.x, a.w + co0 * 9 * a.Cin,
              a.bias_at(co0), a.res ? a.res + co0 : nullptr,
              a.cb ? a.cb + co0 : nullptr, a.zero, a.yp + co0, a.N, a.H, a.W,
              a.Cin, cols, a.Ho, a.Wo, (int)stride, a.Cout,
              a.flags(co0, cols), a.gnp_ptr ? a.gnp_ptr + co0 : nullptr,
              (int)wrap_h, (int)wrap_w);
        },
        a.bias != nullptr, a.res != nullptr, a.cb != nullptr, bn64, wrap);
  }
  return a.result();
}

static torch::Tensor launch_gn_tile_stats(const torch::Tensor &a,
                                          const torch::Tensor *b,
                                          torch::Tensor *out);  // ext.hip

// nearest-2x upsample fused into the 3x3 conv (VAE decoder / UNet Upsample
// blocks): output is [N, Cout, 2H, 2W]; returns (y, partials or None).
// fold (the default route, every shape): four 2x2 sub-pixel convs with the
// folded weights w_fold = fold_ups2x_weight(w_prep), [4,Cout,2,2,Cin];
// fold = false keeps the 9-tap kernel (A/B baseline).
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> ups2x_conv3x3(
    torch::Tensor x, torch::Tensor w_prep, c10::optional<torch::Tensor> bias,
    bool collect_gn, bool wrap_h = false, bool wrap_w = false,
    c10::optional<torch::Tensor> w_fold = c10::nullopt, bool fold = true) {
  auto stream = cur_stream();
  if (fold) {
    TORCH_CHECK(w_fold.has_value(),
                "ups2x_conv3x3: fold needs w_fold (fold_ups2x_weight)");
    const long H = x.size(2), W = x.size(3), Cin = x.size(1);
    const long Cout = w_prep.size(0), Mp = x.size(0) * H * W;
    TORCH_CHECK(w_fold->is_cuda() && w_fold->is_contiguous() &&
                    w_fold->scalar_type() == torch::kBFloat16 &&
                    w_fold->dim() == 5 && w_fold->size(0) == 4 &&
                    w_fold->size(1) == Cout && w_fold->size(2) == 2 &&
                    w_fold->size(3) == 2 && w_fold->size(4) == Cin,
                "ups2x_conv3x3: w_fold must be bf16 [4,Cout,2,2,Cin]");
    TORCH_CHECK(Mp < (1L << 31), "ups2x_conv3x3: too many source pixels");
    TORCH_CHECK(!(wrap_h || wrap_w) || H * W * Cin < (1L << 31),
                "ups2x_conv3x3: wrapped image too large");
    // the epilogue serves the partials when every 128-row tile of source
    // pixels lies in one image; otherwise a stats pass over y follows
    const bool epi_gn = collect_gn && (H * W) % CONV_BM == 0;
    ConvArgs a(x, w_prep, bias, c10::nullopt, c10::nullopt, 2 * H, 2 * W,
               epi_gn);
    const __hip_bfloat16 *wf = (const __hip_bfloat16 *)w_fold->data_ptr();
    dispatch_bools(
        [&](auto B, auto WR) {
          hipLaunchKernelGGL(
              (conv3x3_nhwc_bf16_kernel<decltype(B)::value, false, false,
                                        128, false, decltype(WR)::value,
                                        true>),
              conv_grid((a.Cout + CONV_BN - 1) / CONV_BN,
                        4 * ((Mp + CONV_BM - 1) / CONV_BM)),
              dim3(256), 0, stream, a.x, wf, a.bias_at(0), a.res, a.cb,
              a.zero, a.yp, a.N, a.H, a.W, a.Cin, a.Cout, a.Ho, a.Wo, 1,
              a.Cout, a.flags(0, a.Cout), a.gnp_ptr, (int)wrap_h,
              (int)wrap_w);
        },
        a.bias != nullptr, wrap_h || wrap_w);
    if (collect_gn && !epi_gn && ((long)a.Ho * a.Wo) % 128 == 0 &&
        a.Cout % 8 == 0)  // the stats kernel reads 8-channel vectors
      a.gnp = launch_gn_tile_stats(a.y, nullptr, nullptr);
    return a.result();
  }
  ConvArgs a(x, w_prep, bias, c10::nullopt, c10::nullopt, 2 * x.size(2),
             2 * x.size(3), collect_gn);
  dispatch_bools(
      [&](auto B, auto WR) {
        hipLaunchKernelGGL(
            (conv3x3_nhwc_bf16_kernel<decltype(B)::value, false, false, 128,
                                      true, decltype(WR)::value>),
            conv_grid((a.Cout + CONV_BN - 1) / CONV_BN,
                      (a.M + CONV_BM - 1) / CONV_BM),
            dim3(256), 0, stream, a.x, a.w, a.bias_at(0), a.res, a.cb,
            a.zero, a.yp, a.N, a.H, a.W, a.Cin, a.Cout, a.Ho, a.Wo, 1,
            a.Cout, a.flags(0, a.Cout), a.gnp_ptr, (int)wrap_h, (int)wrap_w);
      },
      a.bias != nullptr, wrap_h || wrap_w);
  return a.result();
}
#endif

