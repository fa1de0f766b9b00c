// Dense-block 3x3 convolution for gfx950: pad 1, stride 1, NHWC bf16, fp32
// accumulate, NARROW outputs (Cout 32 or 64) and channel-sliced operands (the
// RRDBNet trunk of the ESRGAN upscalers, models/esrgan.py).
//
// Operands are channel slices of wider NHWC buffers: X is the first Cin
// channels of pixels ldx elements apart, Y a channel range of pixels ldy
// apart (possibly the same buffer), res1 / res2 slices with strides of their
// own. A residual dense block lives in one [N,H,W,192] workspace
// x | x1 | x2 | x3 | x4; conv k reads a prefix and writes the next 32
// channels in place, so nothing is ever concatenated.
//
// Why not conv.hip: with one 32/64-wide column tile A is never shared between
// blocks and a staged byte feeds a quarter of the 128-column kernel's MFMAs.
// An im2col tile per tap would move every input element into LDS nine times;
// that movement would be the limit. So a block stages a spatial PATCH:
//
//  * work split: a block owns a 16 x 16 rectangle of output pixels of one
//    image (grid.x = rectangles, grid.y = image), 4 waves, each wave 4 output
//    rows x all Cout. __launch_bounds__(256, 1): one wave per SIMD; latency is
//    hidden by the software pipeline, not by occupancy (the LDS budget below
//    leaves room for one block).
//  * K loop over 32-channel chunks. Per chunk the 18 x 18 patch (rectangle +
//    one-pixel halo) is in LDS once; all nine taps read their fragments from
//    it at shifted pixel addresses. Out-of-image halo pixels are ZEROS written
//    at staging time (the load address is the pixel clamped into the image,
//    the value is selected): no zero page, no validity bits in the tap loop.
//    The chunk's weights (9 x Cout rows of 32 channels) sit beside it.
//  * pipeline per chunk, not per tap: chunk c+1's global loads (6 patch + 5 or
//    9 weight b128 pieces a thread) are issued before chunk c's MFMAs and
//    written to the other LDS buffer after them; ONE barrier per chunk (a
//    wave writes buffer cur^1 only after its own reads of cur; the barrier of
//    chunk c-1 saw every read of cur^1 finish).
//  * MFMA: mfma_f32_16x16x32_bf16. For a 32-wide N both shapes read the same
//    LDS bytes per FLOP once fragments are reused in registers (an M x 32
//    wave tile reads its A bytes and its B bytes once per K step with either:
//    (M/32 + 1) KiB per 16 k with 32x32x16, (M/16 + 2) KiB per 32 k with
//    16x16x32), so that count does not decide. 16x16x32 is chosen because one
//    instruction's K is exactly the 32-channel chunk and its 16-row fragment
//    is exactly one 16-pixel row segment of the rectangle: a ragged W wastes
//    at most 15 columns (31 with 32-pixel fragments), and the segment is what
//    makes the row reuse below possible.
//  * register reuse, the point of the design. The operands are SWAPPED
//    (D^T = mfma(W_frag, X_frag)): the pixel fragment of patch row R at
//    column shift dx is read ONCE and feeds the taps dy = 0..2 of output rows
//    R, R-1, R-2, so a wave reads 6 rows x 3 shifts = 18 pixel fragments a
//    chunk instead of 4 rows x 9 taps = 36. The weight fragments of the three
//    taps of a column shift (3 x Cout/16) stay in registers across the wave's
//    four output rows. LDS reads a chunk and block: 72 KiB pixels + 72 KiB
//    (Cout 32) or 144 KiB (Cout 64) weights for 288 / 576 MFMAs.
//  * the swap also fixes the epilogue: a lane holds 4 consecutive MFMA rows
//    (= output channels) of ONE pixel. Weight rows are permuted when staged
//    (LDS row j*16 + m of a tap holds channel (j/2)*32 + (m/4)*8 + (j%2)*4 +
//    m%4), so fragments 2t and 2t+1 give a lane the 8 consecutive channels
//    t*32 + (lane/16)*8 .. +7 of pixel lane%16: 16-byte residual loads and
//    16-byte stores straight from the accumulators, no LDS transpose.
//
// Bank arithmetic (64 banks x 4 B; a b128 read is served 16 lanes at a time,
// and a fragment's 16-lane group reads 16 consecutive pixels, or weight rows,
// at ONE 16-byte channel piece): with 32 channels = 64 B a pixel, pixel p's
// piece starts at 16-byte slot 4p mod 16: four slots, 4-way conflicts. The
// pixel stride is padded to 40 elements = 80 B = 5 slots: slot (5p + c) mod
// 16 is a bijection of 16 consecutive p because 5 is odd, for EVERY start
// pixel, so all nine shifts (which only move the start: (r+dy)*18 + dx) are
// conflict-free, and so are the weight rows (16 consecutive rows, same
// stride). The 16 B of pad per pixel are never read.
//
// LDS: one object (a second __shared__ array makes hipcc drain vmcnt before
// every ds_read), [buf0: patch 324 x 80 B | weights 9*Cout x 80 B][buf1: ..]
// = 97,920 B (Cout 32) / 144,000 B (Cout 64) of the 160 KiB.
//
// Epilogue: y = bf16(alpha * (acc + bias) + beta * res1 + res2), LeakyReLU
// with a run-time slope applied in fp32 before that one rounding. Flags are
// compile-time; the bias is read as stored (bf16 or fp32).
//
// Safety: every address is formed from a pixel clamped into the image; rows
// and columns of the rectangle past H or W are computed and never stored.
#include "common.h"

constexpr int DENSE_T = 16;                      // rectangle edge (pixels)
constexpr int DENSE_PW = DENSE_T + 2;            // patch edge
constexpr int DENSE_PPIX = DENSE_PW * DENSE_PW;  // 324 patch pixels
constexpr int DENSE_KC = 32;                     // channels per K chunk
constexpr int DENSE_PS = 40;                     // LDS row stride, elements
constexpr int DENSE_PBUF = DENSE_PPIX * DENSE_PS;
constexpr int DENSE_PU = DENSE_PPIX * 4;         // 16-byte pieces per patch
constexpr int DENSE_NPI = (DENSE_PU + 255) / 256;

// compiled without packed fp32 VALU ops, as attention_wide.hip's kernel is:
// the attribute is per function, so only force-inlined helpers and builtins
// are called from the kernel (no lambdas, no HIP header conversions)
#if defined(__HIP_DEVICE_COMPILE__)
#define DENSE_KERNEL_ATTR __attribute__((target("no-packed-fp32-ops")))
#else
#define DENSE_KERNEL_ATTR
#endif

struct DenseArgs {
  const __bf16 *x;     // image 0, channel 0 of the X slice
  const __bf16 *w;     // [Cout,3,3,Cin]
  const void *bias;    // [Cout] fp32 or bf16, or null
  const __bf16 *r1;    // res1 slice or null
  const __bf16 *r2;    // res2 slice or null
  __bf16 *y;           // Y slice
  long xs, ys, r1s, r2s;   // image strides (elements)
  int ldx, ldy, ld1, ld2;  // pixel strides (elements)
  int H, W, Cin, tiles_w;
  float alpha, beta, slope;
  int bias_bf16;
};

typedef __attribute__((ext_vector_type(4))) float dense_f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned dense_u32x4;

__device__ __forceinline__ int dense_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int dense_max(int a, int b) { return a > b ? a : b; }

__device__ __forceinline__ void dense_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int COUT, bool HAS_BIAS, bool HAS_R1, bool HAS_R2, bool LRELU>
DENSE_KERNEL_ATTR __launch_bounds__(256, 1) __global__
void conv3x3_dense_bf16_kernel(DenseArgs a) {
  static_assert(COUT == 32 || COUT == 64, "dense conv: Cout 32 or 64");
  constexpr int NJ = COUT / 16;           // weight fragments per tap
  constexpr int NT = COUT / 32;           // 8-channel groups per lane
  constexpr int WROWS = 9 * COUT;         // weight rows per chunk
  constexpr int WBUF = WROWS * DENSE_PS;
  constexpr int WU = WROWS * 4;           // 16-byte pieces per weight chunk
  constexpr int NWI = (WU + 255) / 256;
  constexpr int BUF = DENSE_PBUF + WBUF;
  __shared__ __align__(16) __bf16 smem[2 * BUF];

  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wid = tid / WAVE;
  const int H = a.H, W = a.W, Cin = a.Cin;
  const int th = blockIdx.x / a.tiles_w;
  const int h0 = th * DENSE_T;
  const int w0 = (blockIdx.x - th * a.tiles_w) * DENSE_T;
  const long img = blockIdx.y;
  const __bf16 *X = a.x + img * a.xs;

  // ---- staging bookkeeping: piece u = tid + i*256 of the patch -----------
  // piece u is 16 bytes (8 channels) c16 = u%4 of patch pixel u/4
  int pgo[DENSE_NPI];    // element offset of the clamped pixel in the image
  int plo[DENSE_NPI];    // element offset in the LDS patch
  bool pin[DENSE_NPI];   // pixel inside the image (else zeros)
#pragma unroll
  for (int i = 0; i < DENSE_NPI; ++i) {
    const int u = dense_min(tid + i * 256, DENSE_PU - 1);
    const int pix = u >> 2, c16 = u & 3;
    const int pr = pix / DENSE_PW, pc = pix - pr * DENSE_PW;
    const int h = h0 - 1 + pr, w = w0 - 1 + pc;
    pin[i] = h >= 0 && h < H && w >= 0 && w < W;
    const int hc = dense_min(dense_max(h, 0), H - 1);
    const int wc = dense_min(dense_max(w, 0), W - 1);
    pgo[i] = (hc * W + wc) * a.ldx + c16 * 8;  // host: H*W*ldx < 2^31
    plo[i] = pix * DENSE_PS + c16 * 8;
  }
  // weights: piece u is channel piece u%4 of LDS row u/4 = tap*COUT + jm,
  // which holds output channel (j/2)*32 + (m/4)*8 + (j%2)*4 + m%4
  int wgo[NWI], wlo[NWI];
#pragma unroll
  for (int i = 0; i < NWI; ++i) {
    const int u = dense_min(tid + i * 256, WU - 1);
    const int row = u >> 2, c16 = u & 3;
    const int tap = row / COUT, jm = row % COUT;
    const int j = jm >> 4, m = jm & 15;
    const int co = (j >> 1) * 32 + (m >> 2) * 8 + (j & 1) * 4 + (m & 3);
    wgo[i] = (co * 9 + tap) * Cin + c16 * 8;
    wlo[i] = row * DENSE_PS + c16 * 8;
  }

  // the chunk in flight; only the last piece index of each operand is partial
  // (the first test below folds at compile time for the others)
  dense_u32x4 pst[DENSE_NPI], wst[NWI];
  const int NC = Cin / DENSE_KC;

  // chunk 0 straight into buffer 0
#pragma unroll
  for (int i = 0; i < DENSE_NPI; ++i) {
    if ((i + 1) * 256 <= DENSE_PU || tid + i * 256 < DENSE_PU) {
      dense_u32x4 v = *(const dense_u32x4 *)(X + pgo[i]);
      if (!pin[i]) v = (dense_u32x4){0u, 0u, 0u, 0u};
      *(dense_u32x4 *)(smem + plo[i]) = v;
    }
  }
#pragma unroll
  for (int i = 0; i < NWI; ++i) {
    if ((i + 1) * 256 <= WU || tid + i * 256 < WU)
      *(dense_u32x4 *)(smem + DENSE_PBUF + wlo[i]) =
          *(const dense_u32x4 *)(a.w + wgo[i]);
  }
  dense_barrier();

  dense_f32x4 acc[4][NJ];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[r][j] = (dense_f32x4){0.f, 0.f, 0.f, 0.f};

  const int l16 = lane % 16;
  const int kq = lane / 16;    // which 8 of the chunk's 32 channels
  const int r0 = wid * 4;      // the wave's first output row in the rectangle
  // lane's element offset into a patch row segment / a tap's weight rows
  const int aoff = (r0 * DENSE_PW + l16) * DENSE_PS + kq * 8;
  const int boff = l16 * DENSE_PS + kq * 8;

  for (int c = 0; c < NC; ++c) {
    const bool more = c + 1 < NC;
    if (more) {
      const int k1 = (c + 1) * DENSE_KC;
#pragma unroll
      for (int i = 0; i < DENSE_NPI; ++i)
        if ((i + 1) * 256 <= DENSE_PU || tid + i * 256 < DENSE_PU)
          pst[i] = *(const dense_u32x4 *)(X + pgo[i] + k1);
#pragma unroll
      for (int i = 0; i < NWI; ++i)
        if ((i + 1) * 256 <= WU || tid + i * 256 < WU)
          wst[i] = *(const dense_u32x4 *)(a.w + wgo[i] + k1);
    }

    const __bf16 *pb = smem + (c & 1) * BUF;
    const __bf16 *wb = pb + DENSE_PBUF;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      bf16x8 bfr[3][NJ];
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          bfr[dy][j] = *(const bf16x8 *)(wb + boff +
                                         ((dy * 3 + dx) * COUT + j * 16) *
                                             DENSE_PS);
#pragma unroll
      for (int R = 0; R < 6; ++R) {
        // patch row r0 + R, columns dx .. dx + 15
        const bf16x8 af =
            *(const bf16x8 *)(pb + aoff + (R * DENSE_PW + dx) * DENSE_PS);
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

    if (more) {
      __bf16 *nb = smem + ((c + 1) & 1) * BUF;
#pragma unroll
      for (int i = 0; i < DENSE_NPI; ++i) {
        if ((i + 1) * 256 <= DENSE_PU || tid + i * 256 < DENSE_PU) {
          dense_u32x4 v = pst[i];
          if (!pin[i]) v = (dense_u32x4){0u, 0u, 0u, 0u};
          *(dense_u32x4 *)(nb + plo[i]) = v;
        }
      }
#pragma unroll
      for (int i = 0; i < NWI; ++i)
        if ((i + 1) * 256 <= WU || tid + i * 256 < WU)
          *(dense_u32x4 *)(nb + DENSE_PBUF + wlo[i]) = wst[i];
    }
    dense_barrier();
  }

  // ---- epilogue: lane = pixel (row r0 + r, column l16), channels
  // t*32 + kq*8 .. +7 in acc[r][2t] (first four) and acc[r][2t+1] ----------
  float bv[NT][8];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int co = t * 32 + kq * 8 + e;
      bv[t][e] = !HAS_BIAS ? 0.0f
                 : a.bias_bf16 ? (float)((const __bf16 *)a.bias)[co]
                               : ((const float *)a.bias)[co];
    }
  const __bf16 *R1 = HAS_R1 ? a.r1 + img * a.r1s : nullptr;
  const __bf16 *R2 = HAS_R2 ? a.r2 + img * a.r2s : nullptr;
  __bf16 *Y = a.y + img * a.ys;
  const int w = w0 + l16;
  const int wc = dense_min(w, W - 1);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int h = h0 + r0 + r;
    const bool inside = h < H && w < W;
    // clamped: the residual loads are always legal
    const int pix = dense_min(h, H - 1) * W + wc;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int ch = t * 32 + kq * 8;
      bf16x8 r1v, r2v;
      if constexpr (HAS_R1) r1v = *(const bf16x8 *)(R1 + pix * a.ld1 + ch);
      if constexpr (HAS_R2) r2v = *(const bf16x8 *)(R2 + pix * a.ld2 + ch);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = a.alpha * (acc[r][2 * t + (e >> 2)][e & 3] + bv[t][e]);
        if constexpr (HAS_R1) v += a.beta * (float)r1v[e];
        if constexpr (HAS_R2) v += (float)r2v[e];
        if constexpr (LRELU) v = v > 0.0f ? v : v * a.slope;
        o[e] = (__bf16)v;
      }
      if (inside) *(bf16x8 *)(Y + pix * a.ldy + ch) = o;
    }
  }
}

// ---------------------------------------------------------------------------
// host entry
// ---------------------------------------------------------------------------
bool conv3x3_dense_supported_widths(long cin, long cout) {
  return cin % 32 == 0 && cin >= 64 && cin <= 256 && (cout == 32 || cout == 64);
}

// a 4-d bf16 GPU view [N,C,H,W] that is a channel slice of an NHWC buffer
static void dense_check_view(const torch::Tensor &t, const char *name, long N,
                             long C, long H, long W) {
  TORCH_CHECK(t.dim() == 4, "conv3x3_dense: ", name, " must be 4-d");
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16,
              "conv3x3_dense: ", name, " must be a bf16 GPU tensor");
  TORCH_CHECK(t.size(0) == N && t.size(1) == C && t.size(2) == H &&
                  t.size(3) == W,
              "conv3x3_dense: ", name, " must be [", N, ",", C, ",", H, ",", W,
              "], got ", t.sizes());
  const long ld = t.stride(3);
  TORCH_CHECK(t.stride(1) == 1, "conv3x3_dense: ", name,
              " needs unit channel stride");
  TORCH_CHECK(ld >= C && ld % 8 == 0 && t.stride(2) == W * ld &&
                  t.stride(0) % 8 == 0 && (N == 1 || t.stride(0) >= H * W * ld),
              "conv3x3_dense: ", name, " needs NHWC-ordered strides with a "
              "pixel stride that is a multiple of 8 elements");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "conv3x3_dense: ", name, " must be 16-byte aligned");
  TORCH_CHECK(H * W * ld < (1L << 31), "conv3x3_dense: ", name,
              ": H * W * pixel stride must be below 2^31");
}

// out against another operand in the same storage: the channel ranges must be
// disjoint, or (a residual) identical
static void dense_check_alias(const torch::Tensor &y, const torch::Tensor &t,
                              const char *name, bool identical_ok) {
  if (!y.is_alias_of(t)) return;
  auto extent = [](const torch::Tensor &v) {
    return (v.size(0) - 1) * v.stride(0) + (v.size(2) - 1) * v.stride(2) +
           (v.size(3) - 1) * v.stride(3) + v.size(1);
  };
  const long y0 = y.storage_offset(), t0 = t.storage_offset();
  if (y0 + extent(y) <= t0 || t0 + extent(t) <= y0) return;
  const long ld = y.stride(3);
  TORCH_CHECK(t.stride(3) == ld && t.stride(2) == y.stride(2) &&
                  t.stride(0) == y.stride(0),
              "conv3x3_dense: out shares storage with ", name,
              " under a different layout");
  const long cy = y0 % ld, ct = t0 % ld;
  TORCH_CHECK(y0 - cy == t0 - ct && cy + y.size(1) <= ld &&
                  ct + t.size(1) <= ld,
              "conv3x3_dense: out and ", name,
              " are not channel slices of the same pixels");
  const bool disjoint = cy + y.size(1) <= ct || ct + t.size(1) <= cy;
  const bool identical = cy == ct && y.size(1) == t.size(1);
  TORCH_CHECK(disjoint || (identical_ok && identical),
              "conv3x3_dense: out overlaps the channels of ", name);
}

// out = lrelu(alpha * (conv3x3(x, w) + bias) + beta * res1 + res2), in place
torch::Tensor conv3x3_dense(torch::Tensor x, torch::Tensor w_prep,
                            c10::optional<torch::Tensor> bias,
                            torch::Tensor out, double alpha,
                            c10::optional<torch::Tensor> res1, double beta,
                            c10::optional<torch::Tensor> res2, bool lrelu,
                            double slope) {
  TORCH_CHECK(x.dim() == 4 && out.dim() == 4,
              "conv3x3_dense: x and out must be 4-d");
  const long N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  const long Cout = out.size(1);
  TORCH_CHECK(conv3x3_dense_supported_widths(Cin, Cout),
              "conv3x3_dense: no kernel for Cin=", Cin, " Cout=", Cout,
              " (Cin % 32 == 0 in [64, 256], Cout 32 or 64)");
  TORCH_CHECK(N >= 1 && H >= 1 && W >= 1 && N <= 65535,
              "conv3x3_dense: empty input or N > 65535");
  dense_check_view(x, "x", N, Cin, H, W);
  dense_check_view(out, "out", N, Cout, H, W);
  TORCH_CHECK(w_prep.is_cuda() && w_prep.scalar_type() == torch::kBFloat16 &&
                  w_prep.dim() == 4 && w_prep.is_contiguous() &&
                  w_prep.size(0) == Cout && w_prep.size(1) == 3 &&
                  w_prep.size(2) == 3 && w_prep.size(3) == Cin &&
                  reinterpret_cast<uintptr_t>(w_prep.data_ptr()) % 16 == 0,
              "conv3x3_dense: w_prep must be a contiguous bf16 [Cout,3,3,Cin]");
  TORCH_CHECK(w_prep.device() == x.device() && out.device() == x.device(),
              "conv3x3_dense: tensors must share a device");
  dense_check_alias(out, x, "x", false);

  DenseArgs a{};
  a.x = (const __bf16 *)x.data_ptr();
  a.w = (const __bf16 *)w_prep.data_ptr();
  a.y = (__bf16 *)out.data_ptr();
  a.xs = x.stride(0);
  a.ys = out.stride(0);
  a.ldx = (int)x.stride(3);
  a.ldy = (int)out.stride(3);
  a.H = (int)H;
  a.W = (int)W;
  a.Cin = (int)Cin;
  a.alpha = (float)alpha;
  a.beta = (float)beta;
  a.slope = (float)slope;
  torch::Tensor bias_t;  // outlives the launch call
  if (bias.has_value()) {
    TORCH_CHECK(bias->numel() == Cout && bias->device() == x.device(),
                "conv3x3_dense: bias must be [Cout] on x's device");
    const auto bt = bias->scalar_type();
    bias_t = ((bt == torch::kBFloat16 || bt == torch::kFloat) &&
              bias->is_contiguous())
                 ? *bias  // read as stored
                 : bias->to(torch::kFloat).contiguous();
    a.bias = bias_t.data_ptr();
    a.bias_bf16 = bias_t.scalar_type() == torch::kBFloat16;
  }
  if (res1.has_value()) {
    dense_check_view(*res1, "res1", N, Cout, H, W);
    TORCH_CHECK(res1->device() == x.device(), "conv3x3_dense: res1 device");
    dense_check_alias(out, *res1, "res1", true);
    a.r1 = (const __bf16 *)res1->data_ptr();
    a.r1s = res1->stride(0);
    a.ld1 = (int)res1->stride(3);
  }
  if (res2.has_value()) {
    dense_check_view(*res2, "res2", N, Cout, H, W);
    TORCH_CHECK(res2->device() == x.device(), "conv3x3_dense: res2 device");
    dense_check_alias(out, *res2, "res2", true);
    a.r2 = (const __bf16 *)res2->data_ptr();
    a.r2s = res2->stride(0);
    a.ld2 = (int)res2->stride(3);
  }
  const long tw = (W + DENSE_T - 1) / DENSE_T;
  const long thh = (H + DENSE_T - 1) / DENSE_T;
  TORCH_CHECK(tw * thh < (1L << 31), "conv3x3_dense: image too large");
  a.tiles_w = (int)tw;
  const dim3 grid((unsigned)(tw * thh), (unsigned)N);
  auto stream = cur_stream();
  dispatch_bools(
      [&](auto C64, auto B, auto R1, auto R2, auto L) {
        hipLaunchKernelGGL(
            (conv3x3_dense_bf16_kernel<decltype(C64)::value ? 64 : 32,
                                       decltype(B)::value, decltype(R1)::value,
                                       decltype(R2)::value,
                                       decltype(L)::value>),
            grid, dim3(256), 0, stream, a);
      },
      Cout == 64, a.bias != nullptr, a.r1 != nullptr, a.r2 != nullptr, lrelu);
  return out;
}
