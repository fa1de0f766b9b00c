// Weight-stationary 3x3 convolution for gfx950: pad 1, stride 1, Cin = 64,
// NHWC bf16, fp32 accumulate. The layers of the compact Real-ESRGAN upscalers
// (SRVGGNetCompact, models/esrgan.py): a chain of 64 -> 64 convs with a
// per-channel PReLU each, ended by a 64 -> 48 conv, PixelShuffle(4) and the
// nearest-4x of the network's input.
//
// Why not conv_dense.hip: that kernel re-stages all nine taps of weights for
// every 16 x 16 rectangle (73.7 KB of weights against 41 KB of patch at
// 64 -> 64). At ONE width the weights of a whole layer fit in LDS next to a
// patch, so here they are loaded once per block and only patches move:
//
//  * work split: a block of 4 waves loads the layer's [9][Cout][64] weights
//    into LDS once and then WALKS output tiles t = blockIdx.x, + gridDim.x,
//    ... of the N * ceil(H/16) * ceil(W/16) tiles (grid = min(tiles, blocks),
//    blocks = the CU count unless the caller caps it). A tile is a 16 x 16
//    rectangle of output pixels of one image; a wave owns 4 output rows x all
//    Cout. __launch_bounds__(256, 1): one block a CU, the LDS budget below
//    leaves room for no second one.
//  * inside the walk only the 18 x 18 halo patch (all 64 channels) is
//    staged. The NEXT tile's patch is loaded from global memory into
//    registers (11 b128 pieces a thread) before the current tile's MFMAs and
//    written to LDS after them. Two barriers a tile (patch read by everyone /
//    patch rewritten), none inside the tap loop, none that touches weights.
//  * out-of-image halo pixels are ZEROS written at staging time (the load
//    address is the pixel clamped into the image, the value is selected).
//  * MFMA: mfma_f32_16x16x32_bf16, K = 64 is two steps. Operands SWAPPED as in
//    conv_dense.hip (D^T = mfma(W_frag, X_frag)): the pixel fragment of patch
//    row R at column shift dx feeds the taps dy = 0..2 of output rows R, R-1,
//    R-2 (18 pixel fragments a K step instead of 36), the weight fragments of
//    the three taps of a column shift stay in registers across the wave's four
//    rows, and a lane ends with 4 consecutive MFMA rows (= output channels)
//    of ONE pixel. Per tile and wave: 36 pixel + 18 * Cout/16 weight b128
//    reads for 72 * Cout/16 MFMAs.
//
// Bank arithmetic (64 banks x 4 B; a b128 read is served 16 lanes at a time,
// and a fragment's 16-lane group reads 16 consecutive pixels, or weight rows,
// at ONE 16-byte channel piece): 64 channels are 128 B = 8 slots of 16 B, so
// at the natural stride pixel p's piece c sits in slot (8p + c) mod 16: two
// slots, 8-way conflicts. Rows are padded to 72 elements = 144 B = 9 slots:
// (9p + c) mod 16 is a bijection of 16 consecutive p because 9 is odd, for
// every start pixel (the nine shifts only move the start) and every piece.
// The 16 B of pad per row are never read.
//
// LDS, one object: [weights 9*Cout x 144 B | patch 324 x 144 B]
//   Cout 64: 82,944 + 46,656 = 129,600 B;  Cout 48: 62,208 + 46,656 = 108,864 B
// of the 160 KiB. Two 18 x 18 patches beside the Cout-64 weights would be
// 176,256 B, hence the register prefetch instead of a second LDS buffer.
//
// Variants (compile time; three instantiations, what the model uses):
//  * PRE_ACT: a per-channel PReLU (slopes of its own) applied to the input as
//    the patch is staged, rounded to bf16 as the activation pass it replaces
//    would have stored it. prelu(0) = 0, so the zero halo stays correct.
//  * epilogue PRELU (SHUFFLE = false, Cout 64): y = bf16(prelu_c(acc + bias)),
//    fp32, one rounding. Weight rows are permuted when staged as in
//    conv_dense.hip, so a lane holds 8 consecutive channels: 16-byte stores.
//  * epilogue SHUFFLE (Cout 48, scale 4, no activation): weight rows in
//    natural order, so fragment j is colour plane j and a lane's 4 channels
//    j*16 + kq*4 + 0..3 are the 4 horizontally adjacent pixels (4y + kq,
//    4x + 0..3) of that plane: one 8-byte store to the planar [N,3,4H,4W]
//    output, after adding base[n, j, y, x] (the nearest-4x of the network's
//    input) in fp32. No 48-channel intermediate exists.
//
// No atomics; every sum has one fixed order. Safety: every address is formed
// from a pixel clamped into the image; rows and columns of a tile past H or W
// are computed and never stored.
#include "common.h"

constexpr int CMP_T = 16;                       // tile edge (pixels)
constexpr int CMP_PW = CMP_T + 2;               // patch edge
constexpr int CMP_PPIX = CMP_PW * CMP_PW;       // 324 patch pixels
constexpr int CMP_CIN = 64;
constexpr int CMP_S = 72;                       // LDS row stride, elements
constexpr int CMP_PU = CMP_PPIX * 8;            // 16-byte pieces per patch
constexpr int CMP_NPI = (CMP_PU + 255) / 256;   // 11, the last one partial

struct CompactArgs {
  const __bf16 *x;      // [N,H,W,64]
  const __bf16 *w;      // [Cout,3,3,64]
  const void *bias;     // [Cout] fp32 or bf16, or null
  const void *slope;    // [64] epilogue PReLU slopes (PRELU)
  const void *pre;      // [64] input PReLU slopes (PRE_ACT)
  const __bf16 *base;   // [N,3,H,W], any strides (SHUFFLE)
  __bf16 *y;            // [N,H,W,64], or planar [N,3,4H,4W] (SHUFFLE)
  long base_n;          // base strides (elements)
  int base_c, base_h, base_w;
  int H, W, tiles_h, tiles_w, tiles;  // tiles = N * tiles_h * tiles_w
  int bias_bf16, slope_bf16, pre_bf16;
};

// element i of a vector stored as fp32 or bf16
__device__ __forceinline__ float cmp_ldf(const void *p, int is_bf16, int i) {
  return is_bf16 ? (float)((const __bf16 *)p)[i] : ((const float *)p)[i];
}

// tile t -> its image and the image coordinates of its first output pixel
__device__ __forceinline__ void cmp_decode(const CompactArgs &a, int t, int &n,
                                           int &h0, int &w0) {
  const int per = a.tiles_h * a.tiles_w;
  n = t / per;
  const int r = t - n * per;
  const int th = r / a.tiles_w;
  h0 = th * CMP_T;
  w0 = (r - th * a.tiles_w) * CMP_T;
}

// piece i of a thread exists (only the last index is partial; the first test
// folds at compile time for the others)
__device__ __forceinline__ bool cmp_piece(int i, int tid) {
  return (i + 1) * 256 <= CMP_PU || tid + i * 256 < CMP_PU;
}

// issue the global loads of the patch of the tile at (n, h0, w0); bit i of
// the result says that piece i's pixel is inside the image
__device__ __forceinline__ unsigned cmp_issue(
    const CompactArgs &a, int n, int h0, int w0, int tid, int c8,
    const int (&pr)[CMP_NPI], const int (&pc)[CMP_NPI],
    dense_u32x4 (&pst)[CMP_NPI]) {
  // host: N * H * W * 64 < 2^31
  const __bf16 *X = a.x + n * a.H * a.W * CMP_CIN + c8;
  unsigned in = 0u;
#pragma unroll
  for (int i = 0; i < CMP_NPI; ++i) {
    if (cmp_piece(i, tid)) {
      const int h = h0 - 1 + pr[i], w = w0 - 1 + pc[i];
      if (h >= 0 && h < a.H && w >= 0 && w < a.W) in |= 1u << i;
      const int hc = dense_min(dense_max(h, 0), a.H - 1);
      const int wc = dense_min(dense_max(w, 0), a.W - 1);
      pst[i] = *(const dense_u32x4 *)(X + (hc * a.W + wc) * CMP_CIN);
    }
  }
  return in;
}

// write the loaded patch to LDS: zeros outside the image, the input PReLU
// (slopes psl of the thread's 8 channels) applied on the way
template <bool PRE_ACT>
__device__ __forceinline__ void cmp_commit(
    __bf16 *pb, int tid, unsigned in, const int (&plo)[CMP_NPI],
    const dense_u32x4 (&pst)[CMP_NPI], const float (&psl)[8]) {
#pragma unroll
  for (int i = 0; i < CMP_NPI; ++i) {
    if (cmp_piece(i, tid)) {
      dense_u32x4 v = pst[i];
      if constexpr (PRE_ACT) {
        bf16x8 b = __builtin_bit_cast(bf16x8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f = (float)b[e];
          b[e] = (__bf16)(f > 0.0f ? f : f * psl[e]);
        }
        v = __builtin_bit_cast(dense_u32x4, b);
      }
      if (!((in >> i) & 1u)) v = (dense_u32x4){0u, 0u, 0u, 0u};
      *(dense_u32x4 *)(pb + plo[i]) = v;
    }
  }
}

template <bool PRE_ACT, bool SHUFFLE>
DENSE_KERNEL_ATTR __launch_bounds__(256, 1) __global__
void conv_compact_bf16_kernel(CompactArgs a) {
  constexpr int COUT = SHUFFLE ? 48 : 64;
  constexpr int NJ = COUT / 16;             // weight fragments per tap
  constexpr int WROWS = 9 * COUT;
  constexpr int WELEM = WROWS * CMP_S;
  constexpr int WU = WROWS * 8;             // 16-byte pieces of the weights
  __shared__ __align__(16) __bf16 smem[WELEM + CMP_PPIX * CMP_S];
  __bf16 *pb = smem + WELEM;

  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wid = tid / WAVE;
  const int H = a.H, W = a.W;

  // ---- the layer's weights, once. Piece u is channel piece u%8 of LDS row
  // u/8 = tap*COUT + jm. PRELU: row j*16 + m holds output channel (j/2)*32 +
  // (m/4)*8 + (j%2)*4 + m%4 (fragments 2t, 2t+1 give a lane 8 consecutive
  // channels); SHUFFLE: natural order (fragment j = colour plane j)
  for (int u = tid; u < WU; u += 256) {
    const int row = u >> 3, c16 = u & 7;
    const int tap = row / COUT, jm = row - tap * COUT;
    const int j = jm >> 4, m = jm & 15;
    const int co = SHUFFLE ? jm
                           : (j >> 1) * 32 + (m >> 2) * 8 + (j & 1) * 4 + (m & 3);
    *(dense_u32x4 *)(smem + row * CMP_S + c16 * 8) =
        *(const dense_u32x4 *)(a.w + (co * 9 + tap) * CMP_CIN + c16 * 8);
  }

  // ---- staging bookkeeping: piece u = tid + i*256 of a patch is 16 bytes
  // (8 channels) u%8 of patch pixel u/8; u%8 = tid%8 for every i
  const int c8 = (tid & 7) * 8;
  int pr[CMP_NPI], pc[CMP_NPI], plo[CMP_NPI];
#pragma unroll
  for (int i = 0; i < CMP_NPI; ++i) {
    const int pix = dense_min(tid + i * 256, CMP_PU - 1) >> 3;
    pr[i] = pix / CMP_PW;
    pc[i] = pix - pr[i] * CMP_PW;
    plo[i] = pix * CMP_S + c8;
  }
  float psl[8];
#pragma unroll
  for (int e = 0; e < 8; ++e)
    psl[e] = PRE_ACT ? cmp_ldf(a.pre, a.pre_bf16, c8 + e) : 0.0f;

  const int l16 = lane % 16;
  const int kq = lane / 16;    // which 8 of a K step's 32 channels
  const int r0 = wid * 4;      // the wave's first output row in the tile
  // lane's element offset into a patch row segment / a tap's weight rows
  const int aoff = (r0 * CMP_PW + l16) * CMP_S + kq * 8;
  const int boff = l16 * CMP_S + kq * 8;

  // ---- epilogue constants of the lane
  constexpr int NB = SHUFFLE ? 3 * 4 : 2 * 8;
  float bv[NB], sv[SHUFFLE ? 1 : NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    // SHUFFLE: plane i/4, channel plane*16 + kq*4 + i%4; PRELU: group i/8,
    // channel group*32 + kq*8 + i%8
    const int co = SHUFFLE ? (i >> 2) * 16 + kq * 4 + (i & 3)
                           : (i >> 3) * 32 + kq * 8 + (i & 7);
    bv[i] = a.bias ? cmp_ldf(a.bias, a.bias_bf16, co) : 0.0f;
    if constexpr (!SHUFFLE) sv[i] = cmp_ldf(a.slope, a.slope_bf16, co);
  }

  dense_u32x4 pst[CMP_NPI];
  int t = blockIdx.x;          // host: gridDim.x <= tiles
  int n, h0, w0;
  cmp_decode(a, t, n, h0, w0);
  unsigned in = cmp_issue(a, n, h0, w0, tid, c8, pr, pc, pst);
  cmp_commit<PRE_ACT>(pb, tid, in, plo, pst, psl);
  dense_barrier();             // weights and the first patch are in LDS

  for (;;) {
    const int tn = t + (int)gridDim.x;
    const bool more = tn < a.tiles;       // block-uniform
    int nn = 0, nh0 = 0, nw0 = 0;
    if (more) {
      cmp_decode(a, tn, nn, nh0, nw0);
      in = cmp_issue(a, nn, nh0, nw0, tid, c8, pr, pc, pst);
    }

    dense_f32x4 acc[4][NJ];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        acc[r][j] = (dense_f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 bfr[3][NJ];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            bfr[dy][j] = *(const bf16x8 *)(smem + boff + kk * 32 +
                                           ((dy * 3 + dx) * COUT + j * 16) *
                                               CMP_S);
#pragma unroll
        for (int R = 0; R < 6; ++R) {
          // patch row r0 + R, columns dx .. dx + 15
          const bf16x8 af = *(const bf16x8 *)(pb + aoff + kk * 32 +
                                              (R * CMP_PW + dx) * CMP_S);
#pragma unroll
          for (int dy = 0; dy < 3; ++dy) {
            const int r = R - dy;  // output row whose tap (dy, dx) this is
            if (r >= 0 && r < 4) {
#pragma unroll
              for (int j = 0; j < NJ; ++j)
                acc[r][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    bfr[dy][j], af, acc[r][j], 0, 0, 0);
            }
          }
        }
      }
    }

    dense_barrier();           // every wave has read the patch
    if (more) cmp_commit<PRE_ACT>(pb, tid, in, plo, pst, psl);

    // ---- epilogue: lane = pixel (row r0 + r, column l16) of the tile
    const int w = w0 + l16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = h0 + r0 + r;
      const bool inside = h < H && w < W;
      const int hc = dense_min(h, H - 1), wc = dense_min(w, W - 1);
      if constexpr (SHUFFLE) {
        // host: the extents of base and of y are below 2^31
        const __bf16 *B = a.base + n * a.base_n + hc * a.base_h + wc * a.base_w;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float b = (float)B[j * a.base_c];
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            o[e] = (__bf16)(acc[r][j][e] + bv[j * 4 + e] + b);
          // plane j of image n, row 4h + kq, columns 4w .. 4w + 3
          if (inside)
            *(bf16x4 *)(a.y + (((n * 3 + j) * 4 * H + 4 * hc + kq) * 4 * W +
                               4 * wc)) = o;
        }
      } else {
        __bf16 *Y = a.y + ((n * H + hc) * W + wc) * CMP_CIN + kq * 8;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float v = acc[r][2 * g + (e >> 2)][e & 3] + bv[g * 8 + e];
            o[e] = (__bf16)(v > 0.0f ? v : v * sv[g * 8 + e]);
          }
          if (inside) *(bf16x8 *)(Y + g * 32) = o;
        }
      }
    }

    if (!more) break;
    dense_barrier();           // the next patch is in LDS
    t = tn;
    n = nn;
    h0 = nh0;
    w0 = nw0;
  }
}

// ---------------------------------------------------------------------------
// host entry
// ---------------------------------------------------------------------------
// a [len] fp32 or bf16 vector on x's device, read as stored
static const void *compact_vec(const c10::optional<torch::Tensor> &v,
                               const char *name, long len,
                               const torch::Tensor &x, int &is_bf16) {
  TORCH_CHECK(v.has_value(), "conv_compact: ", name, " is required");
  const auto st = v->scalar_type();
  TORCH_CHECK(v->dim() == 1 && v->numel() == len && v->is_contiguous() &&
                  (st == torch::kFloat || st == torch::kBFloat16) &&
                  v->device() == x.device(),
              "conv_compact: ", name, " must be a contiguous fp32 or bf16 [",
              len, "] on x's device");
  is_bf16 = st == torch::kBFloat16;
  return v->data_ptr();
}

// slope given: y = prelu(conv3x3(prelu?(x, pre_slope), w) + bias, slope),
// [N,64,H,W] channels_last. shuffle_base given: y = pixel_shuffle(conv3x3(x,
// w) + bias, 4) + nearest4x(shuffle_base), [N,3,4H,4W] contiguous.
torch::Tensor conv_compact(torch::Tensor x, torch::Tensor w_prep,
                           c10::optional<torch::Tensor> bias,
                           c10::optional<torch::Tensor> slope,
                           c10::optional<torch::Tensor> pre_slope,
                           c10::optional<torch::Tensor> shuffle_base,
                           long blocks) {
  const bool shuffle = shuffle_base.has_value();
  TORCH_CHECK(shuffle != slope.has_value(),
              "conv_compact: exactly one of slope and shuffle_base");
  TORCH_CHECK(!(shuffle && pre_slope.has_value()),
              "conv_compact: no kernel for pre_slope with shuffle_base");
  TORCH_CHECK(x.dim() == 4 && x.is_cuda() &&
                  x.scalar_type() == torch::kBFloat16,
              "conv_compact: x must be a 4-d bf16 GPU tensor");
  const long N = x.size(0), H = x.size(2), W = x.size(3);
  const long Cout = shuffle ? 48 : 64;
  TORCH_CHECK(x.size(1) == CMP_CIN, "conv_compact: x must have 64 channels");
  TORCH_CHECK(N >= 1 && H >= 1 && W >= 1, "conv_compact: empty input");
  TORCH_CHECK(x.is_contiguous(torch::MemoryFormat::ChannelsLast) &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "conv_compact: x must be channels_last and 16-byte aligned");
  TORCH_CHECK(N * H * W * CMP_CIN < (1L << 31),
              "conv_compact: N * H * W * 64 must be below 2^31");
  TORCH_CHECK(w_prep.is_cuda() && w_prep.scalar_type() == torch::kBFloat16 &&
                  w_prep.dim() == 4 && w_prep.is_contiguous() &&
                  w_prep.size(0) == Cout && w_prep.size(1) == 3 &&
                  w_prep.size(2) == 3 && w_prep.size(3) == CMP_CIN &&
                  w_prep.device() == x.device() &&
                  reinterpret_cast<uintptr_t>(w_prep.data_ptr()) % 16 == 0,
              "conv_compact: w_prep must be a contiguous bf16 [", Cout,
              ",3,3,64] on x's device");
  TORCH_CHECK(blocks >= 1, "conv_compact: blocks must be >= 1");

  CompactArgs a{};
  a.x = (const __bf16 *)x.data_ptr();
  a.w = (const __bf16 *)w_prep.data_ptr();
  if (bias.has_value())
    a.bias = compact_vec(bias, "bias", Cout, x, a.bias_bf16);
  if (pre_slope.has_value())
    a.pre = compact_vec(pre_slope, "pre_slope", CMP_CIN, x, a.pre_bf16);
  a.H = (int)H;
  a.W = (int)W;
  a.tiles_h = (int)((H + CMP_T - 1) / CMP_T);
  a.tiles_w = (int)((W + CMP_T - 1) / CMP_T);
  a.tiles = (int)(N * a.tiles_h * a.tiles_w);  // < N * H * W < 2^31

  torch::Tensor y;
  if (shuffle) {
    const torch::Tensor &b = *shuffle_base;
    TORCH_CHECK(b.dim() == 4 && b.is_cuda() && b.device() == x.device() &&
                    b.scalar_type() == torch::kBFloat16 && b.size(0) == N &&
                    b.size(1) == 3 && b.size(2) == H && b.size(3) == W,
                "conv_compact: shuffle_base must be a bf16 [", N, ",3,", H,
                ",", W, "] on x's device");
    long extent = 1;
    for (int d = 0; d < 4; ++d) {
      TORCH_CHECK(b.stride(d) >= 0,
                  "conv_compact: shuffle_base has a negative stride");
      extent += (b.size(d) - 1) * b.stride(d);
    }
    TORCH_CHECK(extent < (1L << 31),
                "conv_compact: shuffle_base spans 2^31 elements or more");
    a.base = (const __bf16 *)b.data_ptr();
    a.base_n = b.stride(0);
    a.base_c = (int)b.stride(1);
    a.base_h = (int)b.stride(2);
    a.base_w = (int)b.stride(3);
    // 48 * N * H * W elements: below 2^31 by the check on x
    y = torch::empty({N, 3, 4 * H, 4 * W}, x.options());
  } else {
    a.slope = compact_vec(slope, "slope", CMP_CIN, x, a.slope_bf16);
    y = torch::empty({N, CMP_CIN, H, W},
                     x.options().memory_format(
                         torch::MemoryFormat::ChannelsLast));
  }
  a.y = (__bf16 *)y.data_ptr();

  const dim3 grid((unsigned)std::min<long>(a.tiles, blocks));
  auto stream = cur_stream();
  if (shuffle)
    hipLaunchKernelGGL((conv_compact_bf16_kernel<false, true>), grid,
                       dim3(256), 0, stream, a);
  else if (a.pre)
    hipLaunchKernelGGL((conv_compact_bf16_kernel<true, false>), grid,
                       dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((conv_compact_bf16_kernel<false, false>), grid,
                       dim3(256), 0, stream, a);
  return y;
}
