// Ragged-width 3x3 / 1x1 convolution for gfx950: stride 1, "same" padding,
// NHWC bf16, fp32 accumulate, ANY Cin and Cout that are multiples of 4 in
// [4, 512] (the SwinIR convs at embed 180 / 240 and their 60-wide 3conv
// stacks, models/swinir.py). The other conv kernels need Cin % 64 == 0
// (conv.hip) or Cin % 32 == 0 with Cout 32 / 64 (conv_dense.hip).
//
// The design is conv_dense.hip's COUT = 64 case, whose constants, barrier and
// vector types this file uses (it is included after it): a block owns a
// 16 x 16 rectangle of output pixels of one image, 4 waves of 4 output rows;
// the K loop runs over 32-channel chunks whose (16 + KS - 1)^2 halo patch is
// staged into LDS once and read by all KS * KS taps at shifted pixel
// addresses; 80-byte pixel and weight-row stride; swapped
// mfma_f32_16x16x32_bf16 with pixel fragments reused across dy and weight
// fragments across the wave's rows; the next chunk's global loads are issued
// under the current chunk's MFMAs, one barrier per chunk; out-of-image halo
// pixels are zeros selected at staging time over clamped addresses.
//
// What is new:
//
//  * Cout tiles. A block computes ONE 64-wide Cout tile; blockIdx.x =
//    rectangle * ceil(Cout / 64) + tile, so the blocks that read one patch
//    are neighbours in launch order and find it in L2. LDS is the dense
//    kernel's 144,000 B (KS = 3; 51,200 B for KS = 1), one block per CU. All
//    of a 256-wide Cout in one block would need 147 KB of weights a chunk.
//  * Padded weights. The host pads the weights once to [ceil64(Cout), KS, KS,
//    ceil32(Cin)] with zeros (ops.conv_ragged_prepare), so weight staging is
//    the dense kernel's: always 16-byte pieces, no masks, same row
//    permutation (LDS row j*16 + m of a tap holds channel (j/2)*32 + (m/4)*8
//    + (j%2)*4 + m%4 of the tile).
//  * Ragged Cin. The last chunk may be partial (180 = 5 * 32 + 20). A piece
//    of VIN bytes (16: 8 channels, 4 pieces a pixel; 8: 4 channels, 8 pieces
//    a pixel) whose first channel is at or past Cin is written to LDS as
//    zeros: the value is selected, and its load address is clamped to the
//    LAST legal piece of the same pixel (channel Cin - VIN/2), so no load
//    touches a byte outside the Cin channels of a pixel of the view. Cin is a
//    multiple of the piece width, so a piece is never partly valid. The host
//    picks VIN from Cin, the pixel stride and the base alignment.
//  * Ragged Cout. A lane holds channels tile*64 + t*32 + kq*8 .. +7 of its
//    pixel in two accumulator quads. VOUT = 16 moves them as 8 channels (Cout
//    % 8 == 0 makes a group whole or absent), VOUT = 8 each quad on its own
//    (Cout % 4 == 0 makes a quad whole or absent). A group or quad at or past
//    Cout is not loaded from res and not stored; the bias index is clamped to
//    Cout - 1 and the value selected.
//  * KS = 1: the same kernel with a 16 x 16 patch and one tap.
//
// Epilogue, fp32 with one rounding: v = acc + bias; LeakyReLU (run-time
// slope); v += res; y = bf16(v). res may be exactly out's slice: a lane reads
// the residual of exactly the elements it then writes, and no other block
// touches them.
//
// Safety: every address is formed from a pixel clamped into the image and a
// channel clamped into the slice; rows and columns of the rectangle past H
// or W are computed and never stored.

struct RaggedArgs {
  const __bf16 *x;     // image 0, channel 0 of the X slice
  const __bf16 *w;     // [ceil64(Cout),KS,KS,ceil32(Cin)], zero padded
  const void *bias;    // [Cout] fp32 or bf16, or null
  const __bf16 *res;   // residual slice or null
  __bf16 *y;           // Y slice
  long xs, ys, rs;     // image strides (elements)
  int ldx, ldy, ldr;   // pixel strides (elements)
  int H, W, Cin, Cinp, Cout, tiles_w, ctiles;
  float slope;
  int bias_bf16;
};

typedef __attribute__((ext_vector_type(2))) unsigned ragged_u32x2;
template <int VIN> struct ragged_piece { typedef dense_u32x4 type; };
template <> struct ragged_piece<8> { typedef ragged_u32x2 type; };

template <int KS, int VIN, int VOUT, bool HAS_BIAS, bool HAS_RES, bool LRELU>
DENSE_KERNEL_ATTR __launch_bounds__(256, 1) __global__
void conv_ragged_bf16_kernel(RaggedArgs a) {
  static_assert(KS == 1 || KS == 3, "ragged conv: 1x1 or 3x3");
  static_assert((VIN == 8 || VIN == 16) && (VOUT == 8 || VOUT == 16),
                "ragged conv: 8- or 16-byte pieces");
  typedef typename ragged_piece<VIN>::type piece_t;
  constexpr int PW = DENSE_T + KS - 1;    // patch edge
  constexpr int PPIX = PW * PW;
  constexpr int TAPS = KS * KS;
  constexpr int PE = VIN / 2;             // channels per activation piece
  constexpr int PPP = DENSE_KC / PE;      // pieces per patch pixel and chunk
  constexpr int PU = PPIX * PPP;
  constexpr int NPI = (PU + 255) / 256;
  constexpr int PBUF = PPIX * DENSE_PS;
  constexpr int COUT = 64;                // the block's Cout tile
  constexpr int NJ = COUT / 16;
  constexpr int NT = COUT / 32;
  constexpr int WROWS = TAPS * COUT;
  constexpr int WBUF = WROWS * DENSE_PS;
  constexpr int WU = WROWS * 4;           // 16-byte pieces per weight chunk
  constexpr int NWI = (WU + 255) / 256;
  constexpr int BUF = PBUF + WBUF;
  constexpr int NR = 4 + KS - 1;          // patch rows a wave reads
  static_assert(256 % PPP == 0, "a thread's pieces share one channel offset");
  __shared__ __align__(16) __bf16 smem[2 * BUF];

  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wid = tid / WAVE;
  const int H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout;
  const int rect = blockIdx.x / a.ctiles;
  const int tile = blockIdx.x - rect * a.ctiles;   // fastest: shares the patch
  const int th = rect / a.tiles_w;
  const int h0 = th * DENSE_T;
  const int w0 = (rect - th * a.tiles_w) * DENSE_T;
  const long img = blockIdx.y;
  const __bf16 *X = a.x + img * a.xs;

  // ---- staging bookkeeping: piece u = tid + i*256 of the patch is channel
  // piece u % PPP (= tid % PPP for every i) of patch pixel u / PPP ----------
  const int pch = (tid % PPP) * PE;  // the pieces' channel offset in a chunk
  int pgo[NPI];    // element offset of the clamped pixel in the image
  int plo[NPI];    // element offset in the LDS patch
  bool pin[NPI];   // pixel inside the image (else zeros)
#pragma unroll
  for (int i = 0; i < NPI; ++i) {
    const int pix = dense_min((tid + i * 256) / PPP, PPIX - 1);
    const int pr = pix / PW, pc = pix - pr * PW;
    const int h = h0 - KS / 2 + pr, w = w0 - KS / 2 + pc;
    pin[i] = h >= 0 && h < H && w >= 0 && w < W;
    const int hc = dense_min(dense_max(h, 0), H - 1);
    const int wc = dense_min(dense_max(w, 0), W - 1);
    pgo[i] = (hc * W + wc) * a.ldx;  // host: H*W*ldx < 2^31
    plo[i] = pix * DENSE_PS + pch;
  }
  // weights: piece u is channel piece u%4 of LDS row u/4 = tap*64 + jm, which
  // holds the tile's output channel (j/2)*32 + (m/4)*8 + (j%2)*4 + m%4. The
  // padded tensor has every row and every channel piece: no masks
  int wgo[NWI], wlo[NWI];
#pragma unroll
  for (int i = 0; i < NWI; ++i) {
    const int u = dense_min(tid + i * 256, WU - 1);
    const int row = u >> 2, c16 = u & 3;
    const int tap = row / COUT, jm = row % COUT;
    const int j = jm >> 4, m = jm & 15;
    const int co = (j >> 1) * 32 + (m >> 2) * 8 + (j & 1) * 4 + (m & 3);
    wgo[i] = ((tile * COUT + co) * TAPS + tap) * a.Cinp + c16 * 8;
    wlo[i] = row * DENSE_PS + c16 * 8;
  }

  piece_t pst[NPI];
  dense_u32x4 wst[NWI];
  const int NC = a.Cinp / DENSE_KC;

  // chunk 0 straight into buffer 0. A piece at or past Cin: clamped address
  // (the last legal piece of the pixel), zero value
  {
    const bool cok = pch < Cin;
    const int chc = dense_min(pch, Cin - PE);
#pragma unroll
    for (int i = 0; i < NPI; ++i) {
      if ((i + 1) * 256 <= PU || tid + i * 256 < PU) {
        piece_t v = *(const piece_t *)(X + pgo[i] + chc);
        if (!(pin[i] && cok)) v = piece_t{};
        *(piece_t *)(smem + plo[i]) = v;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NWI; ++i) {
    if ((i + 1) * 256 <= WU || tid + i * 256 < WU)
      *(dense_u32x4 *)(smem + PBUF + wlo[i]) =
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
  const int aoff = (r0 * PW + l16) * DENSE_PS + kq * 8;
  const int boff = l16 * DENSE_PS + kq * 8;

  for (int c = 0; c < NC; ++c) {
    const bool more = c + 1 < NC;
    const int k1 = (c + 1) * DENSE_KC;
    const bool cok = k1 + pch < Cin;   // only the last chunk can be partial
    if (more) {
      const int chc = dense_min(k1 + pch, Cin - PE);
#pragma unroll
      for (int i = 0; i < NPI; ++i)
        if ((i + 1) * 256 <= PU || tid + i * 256 < PU)
          pst[i] = *(const piece_t *)(X + pgo[i] + chc);
#pragma unroll
      for (int i = 0; i < NWI; ++i)
        if ((i + 1) * 256 <= WU || tid + i * 256 < WU)
          wst[i] = *(const dense_u32x4 *)(a.w + wgo[i] + k1);
    }

    const __bf16 *pb = smem + (c & 1) * BUF;
    const __bf16 *wb = pb + PBUF;
#pragma unroll
    for (int dx = 0; dx < KS; ++dx) {
      bf16x8 bfr[KS][NJ];
#pragma unroll
      for (int dy = 0; dy < KS; ++dy)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          bfr[dy][j] = *(const bf16x8 *)(wb + boff +
                                         ((dy * KS + dx) * COUT + j * 16) *
                                             DENSE_PS);
#pragma unroll
      for (int R = 0; R < NR; ++R) {
        // patch row r0 + R, columns dx .. dx + 15
        const bf16x8 af =
            *(const bf16x8 *)(pb + aoff + (R * PW + dx) * DENSE_PS);
#pragma unroll
        for (int dy = 0; dy < KS; ++dy) {
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
      for (int i = 0; i < NPI; ++i) {
        if ((i + 1) * 256 <= PU || tid + i * 256 < PU) {
          piece_t v = pst[i];
          if (!(pin[i] && cok)) v = piece_t{};
          *(piece_t *)(nb + plo[i]) = v;
        }
      }
#pragma unroll
      for (int i = 0; i < NWI; ++i)
        if ((i + 1) * 256 <= WU || tid + i * 256 < WU)
          *(dense_u32x4 *)(nb + PBUF + wlo[i]) = wst[i];
    }
    dense_barrier();
  }

  // ---- epilogue: lane = pixel (row r0 + r, column l16), channels
  // tile*64 + t*32 + kq*8 .. +7 in acc[r][2t] (first four) and acc[r][2t+1] --
  const int cbase = tile * COUT + kq * 8;
  float bv[NT][8];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int co = cbase + t * 32 + e;
      const int cc = dense_min(co, Cout - 1);
      float b = 0.0f;
      if constexpr (HAS_BIAS)
        b = a.bias_bf16 ? (float)((const __bf16 *)a.bias)[cc]
                        : ((const float *)a.bias)[cc];
      bv[t][e] = co < Cout ? b : 0.0f;
    }
  const __bf16 *RS = HAS_RES ? a.res + img * a.rs : nullptr;
  __bf16 *Y = a.y + img * a.ys;
  const int w = w0 + l16;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int h = h0 + r0 + r;
    const bool inside = h < H && w < W;
    const int pix = dense_min(h, H - 1) * W + dense_min(w, W - 1);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int ch = cbase + t * 32;
      if constexpr (VOUT == 16) {
        if (inside && ch < Cout) {   // Cout % 8 == 0: all eight exist
          bf16x8 rv, o;
          if constexpr (HAS_RES) rv = *(const bf16x8 *)(RS + pix * a.ldr + ch);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float v = acc[r][2 * t + (e >> 2)][e & 3] + bv[t][e];
            if constexpr (LRELU) v = v > 0.0f ? v : v * a.slope;
            if constexpr (HAS_RES) v += (float)rv[e];
            o[e] = (__bf16)v;
          }
          *(bf16x8 *)(Y + pix * a.ldy + ch) = o;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int cq = ch + q * 4;
          if (inside && cq < Cout) {  // Cout % 4 == 0: all four exist
            bf16x4 rv, o;
            if constexpr (HAS_RES)
              rv = *(const bf16x4 *)(RS + pix * a.ldr + cq);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float v = acc[r][2 * t + q][e] + bv[t][q * 4 + e];
              if constexpr (LRELU) v = v > 0.0f ? v : v * a.slope;
              if constexpr (HAS_RES) v += (float)rv[e];
              o[e] = (__bf16)v;
            }
            *(bf16x4 *)(Y + pix * a.ldy + cq) = o;
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host entry
// ---------------------------------------------------------------------------
bool conv_ragged_supported_widths(long cin, long cout, long ks) {
  return (ks == 1 || ks == 3) && cin % 4 == 0 && cin >= 4 && cin <= 512 &&
         cout % 4 == 0 && cout >= 4 && cout <= 512;
}

// a 4-d bf16 GPU view [N,C,H,W] that is a channel slice of an NHWC buffer;
// returns the widest piece (16 or 8 bytes) its rows can be moved in
static int ragged_check_view(const torch::Tensor &t, const char *name, long N,
                             long C, long H, long W) {
  TORCH_CHECK(t.dim() == 4, "conv_ragged: ", name, " must be 4-d");
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16,
              "conv_ragged: ", name, " must be a bf16 GPU tensor");
  TORCH_CHECK(t.size(0) == N && t.size(1) == C && t.size(2) == H &&
                  t.size(3) == W,
              "conv_ragged: ", name, " must be [", N, ",", C, ",", H, ",", W,
              "], got ", t.sizes());
  const long ld = t.stride(3);
  const long is = N == 1 ? 0 : t.stride(0);  // unused for one image
  TORCH_CHECK(t.stride(1) == 1, "conv_ragged: ", name,
              " needs unit channel stride");
  TORCH_CHECK(ld >= C && ld % 4 == 0 && t.stride(2) == W * ld && is % 4 == 0 &&
                  (N == 1 || is >= H * W * ld),
              "conv_ragged: ", name, " needs NHWC-ordered strides with a "
              "pixel stride that is a multiple of 4 elements");
  const uintptr_t p = reinterpret_cast<uintptr_t>(t.data_ptr());
  TORCH_CHECK(p % 8 == 0, "conv_ragged: ", name, " must be 8-byte aligned");
  TORCH_CHECK(H * W * ld < (1L << 31), "conv_ragged: ", name,
              ": H * W * pixel stride must be below 2^31");
  return C % 8 == 0 && ld % 8 == 0 && is % 8 == 0 && p % 16 == 0 ? 16 : 8;
}

// out against another operand in the same storage: the channel ranges must be
// disjoint, or (the residual) identical
static void ragged_check_alias(const torch::Tensor &y, const torch::Tensor &t,
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
                  (y.size(0) == 1 || t.stride(0) == y.stride(0)),
              "conv_ragged: out shares storage with ", name,
              " under a different layout");
  const long cy = y0 % ld, ct = t0 % ld;
  TORCH_CHECK(y0 - cy == t0 - ct && cy + y.size(1) <= ld &&
                  ct + t.size(1) <= ld,
              "conv_ragged: out and ", name,
              " are not channel slices of the same pixels");
  const bool disjoint = cy + y.size(1) <= ct || ct + t.size(1) <= cy;
  const bool identical = cy == ct && y.size(1) == t.size(1);
  TORCH_CHECK(disjoint || (identical_ok && identical),
              "conv_ragged: out overlaps the channels of ", name);
}

template <int KS, int VIN, int VOUT>
static void ragged_launch(const RaggedArgs &a, dim3 grid, bool lrelu) {
  auto stream = cur_stream();
  dispatch_bools(
      [&](auto B, auto R, auto L) {
        hipLaunchKernelGGL(
            (conv_ragged_bf16_kernel<KS, VIN, VOUT, decltype(B)::value,
                                     decltype(R)::value, decltype(L)::value>),
            grid, dim3(256), 0, stream, a);
      },
      a.bias != nullptr, a.res != nullptr, lrelu);
}

// out = lrelu(conv(x, w) + bias) + res, in place into out
torch::Tensor conv_ragged(torch::Tensor x, torch::Tensor w_prep,
                          c10::optional<torch::Tensor> bias, torch::Tensor out,
                          long ksize, c10::optional<torch::Tensor> res,
                          bool lrelu, double slope) {
  TORCH_CHECK(x.dim() == 4 && out.dim() == 4,
              "conv_ragged: x and out must be 4-d");
  const long N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  const long Cout = out.size(1);
  TORCH_CHECK(conv_ragged_supported_widths(Cin, Cout, ksize),
              "conv_ragged: no kernel for Cin=", Cin, " Cout=", Cout,
              " ksize=", ksize,
              " (multiples of 4 in [4, 512], ksize 1 or 3)");
  TORCH_CHECK(N >= 1 && H >= 1 && W >= 1 && N <= 65535,
              "conv_ragged: empty input or N > 65535");
  const int vin = ragged_check_view(x, "x", N, Cin, H, W);
  int vout = ragged_check_view(out, "out", N, Cout, H, W);
  const long cinp = (Cin + 31) / 32 * 32, coutp = (Cout + 63) / 64 * 64;
  TORCH_CHECK(w_prep.is_cuda() && w_prep.scalar_type() == torch::kBFloat16 &&
                  w_prep.dim() == 4 && w_prep.is_contiguous() &&
                  w_prep.size(0) == coutp && w_prep.size(1) == ksize &&
                  w_prep.size(2) == ksize && w_prep.size(3) == cinp &&
                  reinterpret_cast<uintptr_t>(w_prep.data_ptr()) % 16 == 0,
              "conv_ragged: w_prep must be a contiguous bf16 [", coutp, ",",
              ksize, ",", ksize, ",", cinp, "] (conv_ragged_prepare)");
  TORCH_CHECK(w_prep.device() == x.device() && out.device() == x.device(),
              "conv_ragged: tensors must share a device");
  ragged_check_alias(out, x, "x", false);

  RaggedArgs a{};
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
  a.Cinp = (int)cinp;
  a.Cout = (int)Cout;
  a.slope = (float)slope;
  torch::Tensor bias_t;  // outlives the launch call
  if (bias.has_value()) {
    TORCH_CHECK(bias->numel() == Cout && bias->device() == x.device(),
                "conv_ragged: bias must be [Cout] on x's device");
    const auto bt = bias->scalar_type();
    bias_t = ((bt == torch::kBFloat16 || bt == torch::kFloat) &&
              bias->is_contiguous())
                 ? *bias  // read as stored
                 : bias->to(torch::kFloat).contiguous();
    a.bias = bias_t.data_ptr();
    a.bias_bf16 = bias_t.scalar_type() == torch::kBFloat16;
  }
  if (res.has_value()) {
    const int vres = ragged_check_view(*res, "res", N, Cout, H, W);
    TORCH_CHECK(res->device() == x.device(), "conv_ragged: res device");
    ragged_check_alias(out, *res, "res", true);
    vout = std::min(vout, vres);
    a.res = (const __bf16 *)res->data_ptr();
    a.rs = res->stride(0);
    a.ldr = (int)res->stride(3);
  }
  const long tw = (W + DENSE_T - 1) / DENSE_T;
  const long thh = (H + DENSE_T - 1) / DENSE_T;
  const long ct = coutp / 64;
  TORCH_CHECK(tw * thh * ct < (1L << 31), "conv_ragged: image too large");
  a.tiles_w = (int)tw;
  a.ctiles = (int)ct;
  const dim3 grid((unsigned)(tw * thh * ct), (unsigned)N);
  if (ksize == 3) {
    if (vin == 16 && vout == 16) ragged_launch<3, 16, 16>(a, grid, lrelu);
    else if (vin == 16) ragged_launch<3, 16, 8>(a, grid, lrelu);
    else if (vout == 16) ragged_launch<3, 8, 16>(a, grid, lrelu);
    else ragged_launch<3, 8, 8>(a, grid, lrelu);
  } else {
    if (vin == 16 && vout == 16) ragged_launch<1, 16, 16>(a, grid, lrelu);
    else if (vin == 16) ragged_launch<1, 16, 8>(a, grid, lrelu);
    else if (vout == 16) ragged_launch<1, 8, 16>(a, grid, lrelu);
    else ragged_launch<1, 8, 8>(a, grid, lrelu);
  }
  return out;
}
