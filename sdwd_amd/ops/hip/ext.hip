// sdwd_amd HIP extension: torch bindings + launches for the gfx950 kernels.
// Built in-tree by sdwd_amd/ops/build.py (hipcc --offload-arch=gfx950 via
// torch.utils.cpp_extension); the .so travels with the repo snapshot.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

// defined before the kernel includes: hipify only rewrites this top-level
// file, so included .hip sources call cur_stream() instead of the ATen API.
static inline hipStream_t cur_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

#include "elementwise.hip"
#include "norms.hip"
#include "softmax.hip"
#include "probe.hip"
#include "attention.hip"
#include "conv_v4.hip"
#include "conv.hip"
#include "conv_small.hip"
#include "rng.hip"
#include "tome.hip"

#define CHECK_IN(x)                                                     \
  TORCH_CHECK(x.is_cuda(), #x " must be on GPU");                        \
  TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

static inline int ew_grid(long n) {
  long blocks = (n + 255) / 256;
  return (int)std::min<long>(blocks, 2048);  // grid-stride past this
}

// ---------------------------------------------------------------------------
torch::Tensor silu(torch::Tensor x) {
  CHECK_IN(x);
  auto out = torch::empty_like(x);
  long n = x.numel();
  if (x.scalar_type() == torch::kBFloat16) {
    long nv = n / 8;
    hipLaunchKernelGGL(silu_bf16_kernel, dim3(ew_grid(nv ? nv : n)), dim3(256),
                       0, cur_stream(),
                       (const __hip_bfloat16 *)x.data_ptr(),
                       (__hip_bfloat16 *)out.data_ptr(), nv, n);
  } else if (x.scalar_type() == torch::kFloat) {
    hipLaunchKernelGGL(silu_f32_kernel, dim3(ew_grid(n)), dim3(256), 0,
                       cur_stream(), x.data_ptr<float>(),
                       out.data_ptr<float>(), n);
  } else {
    TORCH_CHECK(false, "silu: unsupported dtype");
  }
  return out;
}

torch::Tensor geglu(torch::Tensor x) {
  CHECK_IN(x);
  long d2 = x.size(-1);
  TORCH_CHECK(d2 % 2 == 0, "geglu: last dim must be even");
  long d = d2 / 2;
  long rows = x.numel() / d2;
  auto sizes = x.sizes().vec();
  sizes.back() = d;
  auto out = torch::empty(sizes, x.options());
  long total = rows * d;
  if (x.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(geglu_bf16_kernel, dim3(ew_grid(total / 8 + 1)),
                       dim3(256), 0, cur_stream(),
                       (const __hip_bfloat16 *)x.data_ptr(),
                       (__hip_bfloat16 *)out.data_ptr(), rows, d);
  } else if (x.scalar_type() == torch::kFloat) {
    hipLaunchKernelGGL(geglu_f32_kernel, dim3(ew_grid(total)), dim3(256), 0,
                       cur_stream(), x.data_ptr<float>(),
                       out.data_ptr<float>(), rows, d);
  } else {
    TORCH_CHECK(false, "geglu: unsupported dtype");
  }
  return out;
}

torch::Tensor axpby(torch::Tensor x, torch::Tensor y, double a, double b) {
  CHECK_IN(x);
  CHECK_IN(y);
  TORCH_CHECK(x.sizes() == y.sizes() && x.scalar_type() == y.scalar_type());
  auto out = torch::empty_like(x);
  long n = x.numel();
  if (x.scalar_type() == torch::kBFloat16) {
    long nv = n / 8;
    hipLaunchKernelGGL(axpby_bf16_kernel, dim3(ew_grid(nv ? nv : n)),
                       dim3(256), 0, cur_stream(),
                       (const __hip_bfloat16 *)x.data_ptr(),
                       (const __hip_bfloat16 *)y.data_ptr(),
                       (__hip_bfloat16 *)out.data_ptr(), (float)a, (float)b,
                       nv, n);
  } else if (x.scalar_type() == torch::kFloat) {
    hipLaunchKernelGGL(axpby_f32_kernel, dim3(ew_grid(n)), dim3(256), 0,
                       cur_stream(), x.data_ptr<float>(), y.data_ptr<float>(),
                       out.data_ptr<float>(), (float)a, (float)b, n);
  } else {
    TORCH_CHECK(false, "axpby: unsupported dtype");
  }
  return out;
}

torch::Tensor euler_step(torch::Tensor x, torch::Tensor denoised, double sigma,
                         double sigma_next) {
  // x + (x - den)/sigma * (s_next - s)  ==  (1+r)*x + (-r)*den, r=(sn-s)/s
  double r = (sigma_next - sigma) / sigma;
  return axpby(x, denoised, 1.0 + r, -r);
}

// ---------------------------------------------------------------------------
// fp32 copy of a norm weight/bias for the kernels that read it as 16 B
// vectors (a view at an odd storage offset is re-materialised)
static torch::Tensor f32_vec_aligned(const torch::Tensor &t) {
  auto f = t.to(torch::kFloat).contiguous();
  if (reinterpret_cast<uintptr_t>(f.data_ptr()) % 16 != 0) f = f.clone();
  return f;
}

static void check_nhwc_bf16(const torch::Tensor &x, const char *what) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 &&
                  x.scalar_type() == torch::kBFloat16 &&
                  x.is_contiguous(torch::MemoryFormat::ChannelsLast) &&
                  x.size(1) % 8 == 0,
              what, ": bf16 channels_last with C % 8 == 0 only");
}

// Launch the tile-layout statistics kernel over a (or a + b -> out when b is
// given); returns the partials [N*ceil(HW/128)][2][C].
static torch::Tensor launch_gn_tile_stats(const torch::Tensor &a,
                                          const torch::Tensor *b,
                                          torch::Tensor *out) {
  const long N = a.size(0);
  const int C = a.size(1);
  const long HW = a.size(2) * (long)a.size(3);
  const long tpi = (HW + 127) / 128;
  const int VC = C / 8;
  int CB = 1;  // widest column slab <= 64 that divides VC
  for (int d = std::min(VC, 64); d >= 1; --d)
    if (VC % d == 0) {
      CB = d;
      break;
    }
  auto partial = torch::empty({N * tpi, 2L, (long)C},
                              a.options().dtype(torch::kFloat));
  if (N * tpi == 0) return partial;
  TORCH_CHECK(N * tpi < (1L << 31), "gn tile stats: too many tiles");
  dim3 grid((unsigned)(N * tpi), (unsigned)(VC / CB));
  if (b) {
    hipLaunchKernelGGL(gn_tile_stats_bf16<true>, grid, dim3(256), 0,
                       cur_stream(), (const __hip_bfloat16 *)a.data_ptr(),
                       (const __hip_bfloat16 *)b->data_ptr(),
                       (__hip_bfloat16 *)out->data_ptr(),
                       partial.data_ptr<float>(), C, HW, (int)tpi, CB);
  } else {
    hipLaunchKernelGGL(gn_tile_stats_bf16<false>, grid, dim3(256), 0,
                       cur_stream(), (const __hip_bfloat16 *)a.data_ptr(),
                       (const __hip_bfloat16 *)nullptr,
                       (__hip_bfloat16 *)nullptr, partial.data_ptr<float>(),
                       C, HW, (int)tpi, CB);
  }
  return partial;
}

// Per-tile per-channel (sum, sumsq) of one channels_last bf16 tensor, in the
// layout the conv epilogues emit.
torch::Tensor gn_tile_stats(torch::Tensor x) {
  check_nhwc_bf16(x, "gn_tile_stats");
  return launch_gn_tile_stats(x, nullptr, nullptr);
}

// a + b (bit-equal to the ATen bf16 add) and the sum's GroupNorm partials in
// one pass over memory.
std::tuple<torch::Tensor, torch::Tensor> add_gn(torch::Tensor a,
                                                torch::Tensor b) {
  check_nhwc_bf16(a, "add_gn");
  check_nhwc_bf16(b, "add_gn");
  TORCH_CHECK(a.sizes() == b.sizes(), "add_gn: shape mismatch");
  auto out = torch::empty_like(a);  // keeps channels_last strides
  auto partial = launch_gn_tile_stats(a, &b, &out);
  return {out, partial};
}

// GroupNorm(+SiLU) over channels_last x from per-tile partials
// [N*tiles_per_image][2][C]: finalize the per-(n, g) statistics, then the
// normalise sweep.
static torch::Tensor gn_nhwc_apply(const torch::Tensor &x,
                                   const torch::Tensor &w,
                                   const torch::Tensor &b, long groups,
                                   double eps, bool silu_act,
                                   const torch::Tensor &partial,
                                   long tiles_per_image) {
  const long N = x.size(0);
  const int C = x.size(1);
  const long HW = x.size(2) * (long)x.size(3);
  TORCH_CHECK(C % 8 == 0 && C <= 3072, "nhwc GN: C%8==0 and C<=3072");
  TORCH_CHECK(groups > 0 && C % groups == 0, "nhwc GN: C % groups != 0");
  auto wf = f32_vec_aligned(w);
  auto bf = f32_vec_aligned(b);
  TORCH_CHECK(wf.numel() == C && bf.numel() == C, "nhwc GN: w/b size");
  auto out = torch::empty_like(x);  // keeps channels_last strides
  if (x.numel() == 0) return out;
  auto stats = torch::empty({N * (long)groups, 2L},
                            x.options().dtype(torch::kFloat));
  auto stream = cur_stream();
  hipLaunchKernelGGL(gn_nhwc_stats, dim3((unsigned)(N * groups)), dim3(WAVE),
                     0, stream, partial.data_ptr<float>(),
                     stats.data_ptr<float>(), C, HW, (int)groups,
                     (int)tiles_per_image, (float)eps);
  // enough blocks to fill 256 CUs several times over, but at least ~4 rows
  // per thread so the per-thread parameter loads stay amortised
  const int VC = C / 8;
  const long RP = VC <= 256 ? 256 / VC : 1;
  const long S = std::max<long>(
      1, std::min<long>(4096 / N, (HW + RP * 4 - 1) / (RP * 4)));
  dispatch_bools(
      [&](auto SL, auto TWO) {
        hipLaunchKernelGGL(
            (gn_nhwc_norm_bf16<decltype(SL)::value,
                               decltype(TWO)::value ? 2 : 1>),
            dim3((unsigned)(N * S)), dim3(256), 0, stream,
            (const __hip_bfloat16 *)x.data_ptr(), stats.data_ptr<float>(),
            wf.data_ptr<float>(), bf.data_ptr<float>(),
            (__hip_bfloat16 *)out.data_ptr(), C, HW, (int)groups, (int)S);
      },
      silu_act, VC > 256);
  return out;
}

torch::Tensor group_norm_silu_nhwc(torch::Tensor x, torch::Tensor w,
                                   torch::Tensor b, long groups, double eps,
                                   bool silu_act) {
  // x: NCHW sizes, channels_last memory (= NHWC rows of C)
  check_nhwc_bf16(x, "nhwc GN");
  const long HW = x.size(2) * (long)x.size(3);
  auto partial = launch_gn_tile_stats(x, nullptr, nullptr);
  return gn_nhwc_apply(x, w, b, groups, eps, silu_act, partial,
                       (HW + 127) / 128);
}

torch::Tensor group_norm_silu_pre(torch::Tensor x, torch::Tensor w,
                                  torch::Tensor b, long groups, double eps,
                                  bool silu_act, torch::Tensor gnp,
                                  long tiles_per_image) {
  // GroupNorm with partials that a producer already emitted (conv epilogue,
  // add_gn, gn_tile_stats): skips the full-tensor stats read
  check_nhwc_bf16(x, "group_norm_silu_pre");
  const long N = x.size(0);
  const int C = x.size(1);
  TORCH_CHECK(gnp.is_cuda() && gnp.scalar_type() == torch::kFloat &&
              gnp.is_contiguous());
  TORCH_CHECK(gnp.numel() == N * tiles_per_image * 2 * C,
              "gn partials shape mismatch");
  return gn_nhwc_apply(x, w, b, groups, eps, silu_act, gnp, tiles_per_image);
}

torch::Tensor group_norm_silu(torch::Tensor x, torch::Tensor w,
                              torch::Tensor b, long groups, double eps,
                              bool silu_act) {
  TORCH_CHECK(x.dim() == 4, "expect NCHW");
  if (x.is_contiguous(torch::MemoryFormat::ChannelsLast) &&
      x.scalar_type() == torch::kBFloat16 && x.size(1) % 8 == 0 &&
      x.size(1) <= 3072 && x.size(1) > 8) {
    return group_norm_silu_nhwc(x, w, b, groups, eps, silu_act);
  }
  CHECK_IN(x);
  const int N = x.size(0), C = x.size(1);
  const long HW = x.size(2) * (long)x.size(3);
  TORCH_CHECK(C % groups == 0);
  auto wf = w.to(torch::kFloat).contiguous();
  auto bf = b.to(torch::kFloat).contiguous();
  auto out = torch::empty_like(x);
  dim3 grid(N * (int)groups), block(256);
  if (x.scalar_type() == torch::kBFloat16) {
    const long len = (C / groups) * HW;
    const bool vec = (HW % 8 == 0) && (len % 8 == 0);
    auto kern = silu_act
                    ? (vec ? group_norm_silu_bf16_kernel<true, true>
                           : group_norm_silu_bf16_kernel<true, false>)
                    : (vec ? group_norm_silu_bf16_kernel<false, true>
                           : group_norm_silu_bf16_kernel<false, false>);
    hipLaunchKernelGGL(kern, grid, block, 0, cur_stream(),
                       (const __hip_bfloat16 *)x.data_ptr(),
                       wf.data_ptr<float>(), bf.data_ptr<float>(),
                       (__hip_bfloat16 *)out.data_ptr(), N, C, HW,
                       (int)groups, (float)eps);
  } else if (x.scalar_type() == torch::kFloat) {
    auto kern = silu_act ? group_norm_silu_f32_kernel<true>
                         : group_norm_silu_f32_kernel<false>;
    hipLaunchKernelGGL(kern, grid, block, 0, cur_stream(),
                       x.data_ptr<float>(), wf.data_ptr<float>(),
                       bf.data_ptr<float>(), out.data_ptr<float>(), N, C, HW,
                       (int)groups, (float)eps);
  } else {
    TORCH_CHECK(false, "group_norm_silu: unsupported dtype");
  }
  return out;
}

torch::Tensor layer_norm(torch::Tensor x, torch::Tensor w, torch::Tensor b,
                         double eps) {
  auto xc = x.contiguous();
  TORCH_CHECK(xc.is_cuda());
  const int D = xc.size(-1);
  const long R = xc.numel() / D;
  auto wf = w.to(torch::kFloat).contiguous();
  auto bf = b.to(torch::kFloat).contiguous();
  auto out = torch::empty_like(xc);
  dim3 grid((unsigned)((R + 3) / 4)), block(256);
  if (xc.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(layer_norm_bf16_kernel, grid, block, 0, cur_stream(),
                       (const __hip_bfloat16 *)xc.data_ptr(),
                       wf.data_ptr<float>(), bf.data_ptr<float>(),
                       (__hip_bfloat16 *)out.data_ptr(), R, D, (float)eps);
  } else if (xc.scalar_type() == torch::kFloat) {
    hipLaunchKernelGGL(layer_norm_f32_kernel, grid, block, 0, cur_stream(),
                       xc.data_ptr<float>(), wf.data_ptr<float>(),
                       bf.data_ptr<float>(), out.data_ptr<float>(), R, D,
                       (float)eps);
  } else {
    TORCH_CHECK(false, "layer_norm: unsupported dtype");
  }
  return out;
}

std::vector<torch::Tensor> add_layer_norm(torch::Tensor x, torch::Tensor r,
                                          torch::Tensor w, torch::Tensor b,
                                          double eps) {
  auto xc = x.contiguous();
  auto rc = r.contiguous();
  const int D = xc.size(-1);
  const long R = xc.numel() / D;
  TORCH_CHECK(xc.scalar_type() == torch::kBFloat16 && D % 8 == 0 &&
                  D <= 1536,
              "add_layer_norm: bf16, D%8==0, D<=1536");
  TORCH_CHECK(xc.is_cuda() && rc.scalar_type() == torch::kBFloat16 &&
                  rc.sizes() == xc.sizes(),
              "add_layer_norm: x and r must match");
  auto wf = f32_vec_aligned(w);
  auto bf = f32_vec_aligned(b);
  TORCH_CHECK(wf.numel() == D && bf.numel() == D, "add_layer_norm: w/b size");
  auto out_sum = torch::empty_like(xc);
  auto out_ln = torch::empty_like(xc);
  if (R == 0) return {out_sum, out_ln};
  dim3 grid((unsigned)((R + 3) / 4)), block(256);
  // vec8 slices per lane: D <= 512 -> 1, <= 1024 -> 2, <= 1536 -> 3
  auto kern = D <= 512    ? add_layer_norm_bf16_kernel<1>
              : D <= 1024 ? add_layer_norm_bf16_kernel<2>
                          : add_layer_norm_bf16_kernel<3>;
  hipLaunchKernelGGL(kern, grid, block, 0, cur_stream(),
                     (const __hip_bfloat16 *)xc.data_ptr(),
                     (const __hip_bfloat16 *)rc.data_ptr(),
                     wf.data_ptr<float>(), bf.data_ptr<float>(),
                     (__hip_bfloat16 *)out_sum.data_ptr(),
                     (__hip_bfloat16 *)out_ln.data_ptr(), R, D, (float)eps,
                     (const int *)nullptr, 0, 0);
  return {out_sum, out_ln};
}

static void check_tome_table(const torch::Tensor &t, const torch::Tensor &x,
                             const char *name) {
  TORCH_CHECK(t.is_cuda() && t.device() == x.device() &&
                  t.scalar_type() == torch::kInt && t.is_contiguous(),
              "tome: ", name, " must be a contiguous int32 tensor on x's device");
}

// add_layer_norm with token merging's unmerge folded in: x [B,N,D], r
// [B,M,D], slot int32 [B,N]; row t adds r[b, slot[b,t]]
std::vector<torch::Tensor> add_layer_norm_gather(torch::Tensor x,
                                                 torch::Tensor r,
                                                 torch::Tensor w,
                                                 torch::Tensor b, double eps,
                                                 torch::Tensor slot) {
  TORCH_CHECK(x.dim() == 3 && r.dim() == 3, "add_layer_norm: gather takes "
                                            "x [B,N,D] and r [B,M,D]");
  auto xc = x.contiguous();
  auto rc = r.contiguous();
  const int D = xc.size(-1);
  const long B = xc.size(0), N = xc.size(1), M = rc.size(1);
  TORCH_CHECK(xc.scalar_type() == torch::kBFloat16 && D % 8 == 0 &&
                  D <= 1536,
              "add_layer_norm: bf16, D%8==0, D<=1536");
  TORCH_CHECK(xc.is_cuda() && rc.scalar_type() == torch::kBFloat16 &&
                  rc.size(0) == B && rc.size(2) == D && M >= 1 &&
                  rc.device() == xc.device(),
              "add_layer_norm: r must be a bf16 [B,M,D] next to x");
  check_tome_table(slot, xc, "slot");
  TORCH_CHECK(slot.numel() == B * N, "add_layer_norm: slot must be [B,N]");
  TORCH_CHECK(N < (1L << 31) && M < (1L << 31), "add_layer_norm: N, M < 2^31");
  auto wf = f32_vec_aligned(w);
  auto bf = f32_vec_aligned(b);
  TORCH_CHECK(wf.numel() == D && bf.numel() == D, "add_layer_norm: w/b size");
  auto out_sum = torch::empty_like(xc);
  auto out_ln = torch::empty_like(xc);
  const long R = B * N;
  if (R == 0) return {out_sum, out_ln};
  dim3 grid((unsigned)((R + 3) / 4)), block(256);
  auto kern = D <= 512    ? add_layer_norm_bf16_kernel<1, true>
              : D <= 1024 ? add_layer_norm_bf16_kernel<2, true>
                          : add_layer_norm_bf16_kernel<3, true>;
  hipLaunchKernelGGL(kern, grid, block, 0, cur_stream(),
                     (const __hip_bfloat16 *)xc.data_ptr(),
                     (const __hip_bfloat16 *)rc.data_ptr(),
                     wf.data_ptr<float>(), bf.data_ptr<float>(),
                     (__hip_bfloat16 *)out_sum.data_ptr(),
                     (__hip_bfloat16 *)out_ln.data_ptr(), R, D, (float)eps,
                     (const int *)slot.data_ptr(), (int)N, (int)M);
  return {out_sum, out_ln};
}

// ---------------------------------------------------------------------------
// token merging (tome.hip)
// ---------------------------------------------------------------------------
bool tome_match_supported_width(long c) { return c == 320; }

// x bf16 [B,N,C] contiguous; src_tok [Ns], dst_tok [Nd] int32 ->
// (node_max fp32 [B,Ns], node_idx int32 [B,Ns])
std::vector<torch::Tensor> tome_match(torch::Tensor x, torch::Tensor src_tok,
                                      torch::Tensor dst_tok) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous() &&
                  x.scalar_type() == torch::kBFloat16,
              "tome_match: x must be a contiguous bf16 [B,N,C] GPU tensor");
  const long B = x.size(0), N = x.size(1), C = x.size(2);
  TORCH_CHECK(tome_match_supported_width(C),
              "tome_match: no kernel for C=", C);
  check_tome_table(src_tok, x, "src_tok");
  check_tome_table(dst_tok, x, "dst_tok");
  const long Ns = src_tok.numel(), Nd = dst_tok.numel();
  TORCH_CHECK(Ns >= 1 && Nd >= 1 && Ns + Nd == N && N < (1L << 31),
              "tome_match: src_tok and dst_tok must partition the N tokens");
  TORCH_CHECK(B <= 65535, "tome_match: B <= 65535");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "tome_match: x must be 16 B aligned");
  auto fopt = x.options().dtype(torch::kFloat);
  auto rn = torch::empty({B, N}, fopt);
  auto node_max = torch::empty({B, Ns}, fopt);
  auto node_idx = torch::empty({B, Ns}, x.options().dtype(torch::kInt));
  if (B == 0) return {node_max, node_idx};
  hipLaunchKernelGGL(tome_rnorm_bf16_kernel,
                     dim3((unsigned)((B * N + 3) / 4)), dim3(256), 0,
                     cur_stream(), (const __hip_bfloat16 *)x.data_ptr(),
                     rn.data_ptr<float>(), B * N, (int)C);
  hipLaunchKernelGGL(tome_match_bf16_kernel<320>,
                     dim3((unsigned)((Ns + 127) / 128), (unsigned)B),
                     dim3(256), 0, cur_stream(),
                     (const __hip_bfloat16 *)x.data_ptr(),
                     rn.data_ptr<float>(), (const int *)src_tok.data_ptr(),
                     (const int *)dst_tok.data_ptr(),
                     node_max.data_ptr<float>(), (int *)node_idx.data_ptr(),
                     (int)N, (int)Ns, (int)Nd);
  return {node_max, node_idx};
}

// x bf16 [B,N,C]; dst_tok [Nd]; unm_tok [B,Nu]; seg_start [B,Nd+1];
// members [B,r] -> [B, Nu+Nd, C]
torch::Tensor tome_merge(torch::Tensor x, torch::Tensor dst_tok,
                         torch::Tensor unm_tok, torch::Tensor seg_start,
                         torch::Tensor members) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous() &&
                  x.scalar_type() == torch::kBFloat16 && x.size(2) % 8 == 0,
              "tome_merge: x must be a contiguous bf16 [B,N,C], C%8==0");
  const long B = x.size(0), N = x.size(1), C = x.size(2);
  check_tome_table(dst_tok, x, "dst_tok");
  check_tome_table(unm_tok, x, "unm_tok");
  check_tome_table(seg_start, x, "seg_start");
  check_tome_table(members, x, "members");
  const long Nd = dst_tok.numel();
  TORCH_CHECK(unm_tok.dim() == 2 && members.dim() == 2 &&
                  seg_start.dim() == 2 && unm_tok.size(0) == B &&
                  members.size(0) == B && seg_start.size(0) == B &&
                  seg_start.size(1) == Nd + 1,
              "tome_merge: table shapes");
  const long Nu = unm_tok.size(1), r = members.size(1);
  TORCH_CHECK(Nd >= 1 && Nu + r + Nd == N && N < (1L << 31),
              "tome_merge: the tables must cover the N tokens");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "tome_merge: x must be 16 B aligned");
  auto out = torch::empty({B, Nu + Nd, C}, x.options());
  const long rows = B * (Nu + Nd);
  if (rows == 0) return out;
  hipLaunchKernelGGL(tome_merge_bf16_kernel, dim3((unsigned)((rows + 3) / 4)),
                     dim3(256), 0, cur_stream(),
                     (const __hip_bfloat16 *)x.data_ptr(),
                     (const int *)dst_tok.data_ptr(),
                     (const int *)unm_tok.data_ptr(),
                     (const int *)seg_start.data_ptr(),
                     (const int *)members.data_ptr(),
                     (__hip_bfloat16 *)out.data_ptr(), (int)B, (int)N,
                     (int)Nu, (int)Nd, (int)r, (int)C);
  return out;
}

// y bf16 [B,M,C]; slot int32 [B,N] -> [B,N,C]
torch::Tensor tome_unmerge(torch::Tensor y, torch::Tensor slot) {
  TORCH_CHECK(y.is_cuda() && y.dim() == 3 && y.is_contiguous() &&
                  y.scalar_type() == torch::kBFloat16 && y.size(2) % 8 == 0,
              "tome_unmerge: y must be a contiguous bf16 [B,M,C], C%8==0");
  check_tome_table(slot, y, "slot");
  const long B = y.size(0), M = y.size(1), C = y.size(2);
  TORCH_CHECK(slot.dim() == 2 && slot.size(0) == B && M >= 1 &&
                  M < (1L << 31) && slot.size(1) < (1L << 31),
              "tome_unmerge: slot must be [B,N]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(y.data_ptr()) % 16 == 0,
              "tome_unmerge: y must be 16 B aligned");
  const long N = slot.size(1);
  auto out = torch::empty({B, N, C}, y.options());
  const long total = B * N * (C / 8);
  if (total == 0) return out;
  hipLaunchKernelGGL(tome_unmerge_bf16_kernel, dim3(ew_grid(total)), dim3(256),
                     0, cur_stream(), (const __hip_bfloat16 *)y.data_ptr(),
                     (const int *)slot.data_ptr(),
                     (__hip_bfloat16 *)out.data_ptr(), B * N, (int)N, (int)M,
                     (int)(C / 8));
  return out;
}

// ---------------------------------------------------------------------------
// attention
// ---------------------------------------------------------------------------
void row_softmax_(torch::Tensor x, double scale) {
  CHECK_IN(x);
  const int S = x.size(-1);
  const long R = x.numel() / S;
  dim3 grid((unsigned)((R + 3) / 4)), block(256);
  if (x.scalar_type() == torch::kFloat) {
    hipLaunchKernelGGL(row_softmax_f32_kernel, grid, block, 0, cur_stream(),
                       x.data_ptr<float>(), R, S, (float)scale);
  } else if (x.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(row_softmax_bf16_kernel, grid, block, 0, cur_stream(),
                       (__hip_bfloat16 *)x.data_ptr(), R, S, (float)scale);
  } else {
    TORCH_CHECK(false, "row_softmax: unsupported dtype");
  }
}

torch::Tensor attention_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                            double scale, long force = 0) {
  // [B,H,S,D]; the flash path reads strided (no transpose/pad copies).
  // attention_plan names the kernel (and rejects a forced flash kernel on
  // a head dim that has none); a flash plan also needs bf16, unit-stride D
  const bool flash_layout = q.scalar_type() == torch::kBFloat16 &&
                            q.stride(3) == 1 && k.stride(3) == 1 &&
                            v.stride(3) == 1;
  const bool composed =
      std::get<0>(attention_plan(q.size(3), k.size(2), force)) == "composed";
  if (!composed && flash_layout) {
    return flash_attention_raw(q, k, v, scale, /*bshd=*/false, force);
  }
  TORCH_CHECK(force == 0,
              "attention_fwd: a forced flash kernel needs bf16 q/k/v with "
              "unit stride in D");
  auto qc = q.contiguous(), kc = k.contiguous(), vc = v.contiguous();
  const long B = qc.size(0), H = qc.size(1);
  const long Sq = qc.size(2), Sk = kc.size(2), D = qc.size(3);
  // fallback composition: hipBLASLt GEMMs + fused-softmax kernel, chunked
  // over B*H to bound the score buffer.
  auto q3 = qc.view({B * H, Sq, D});
  auto k3 = kc.view({B * H, Sk, D});
  auto v3 = vc.view({B * H, Sk, D});
  auto out = torch::empty_like(q3);
  const long budget_rows = std::max<long>(1, (1LL << 31) / (Sq * Sk * 2));
  for (long s = 0; s < B * H; s += budget_rows) {
    long e = std::min(B * H, s + budget_rows);
    auto scores = at::matmul(q3.slice(0, s, e),
                             k3.slice(0, s, e).transpose(1, 2));
    row_softmax_(scores, scale);
    out.slice(0, s, e) = at::matmul(scores, v3.slice(0, s, e));
  }
  return out.view(qc.sizes());
}

// ---------------------------------------------------------------------------
torch::Tensor probe_mfma32(torch::Tensor A, torch::Tensor B) {
  CHECK_IN(A);
  CHECK_IN(B);
  auto C = torch::zeros({32, 32}, A.options());
  hipLaunchKernelGGL(probe_mfma_32x32x16, dim3(1), dim3(64), 0, cur_stream(),
                     A.data_ptr<float>(), B.data_ptr<float>(),
                     C.data_ptr<float>());
  return C;
}

torch::Tensor probe_mfma16(torch::Tensor A, torch::Tensor B) {
  CHECK_IN(A);
  CHECK_IN(B);
  auto C = torch::zeros({16, 16}, A.options());
  hipLaunchKernelGGL(probe_mfma_16x16x32, dim3(1), dim3(64), 0, cur_stream(),
                     A.data_ptr<float>(), B.data_ptr<float>(),
                     C.data_ptr<float>());
  return C;
}

torch::Tensor probe_tr16(long stride_bytes, long base_bytes) {
  auto out = torch::zeros(
      {64, 4}, torch::dtype(torch::kFloat32).device(torch::kCUDA));
  hipLaunchKernelGGL(probe_tr_b16, dim3(1), dim3(64), 0, cur_stream(),
                     out.data_ptr<float>(), (int)stride_bytes,
                     (int)base_bytes);
  return out;
}

torch::Tensor attention_fwd_bshd(torch::Tensor q, torch::Tensor k,
                                 torch::Tensor v, double scale,
                                 long force = 0) {
  // [B,S,H,D] (the natural projection layout; avoids transposes entirely)
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
                  flash_supported(q.size(3)),
              "attention_fwd_bshd: bf16 with supported head dim only");
  return flash_attention_raw(q, k, v, scale, /*bshd=*/true, force);
}

torch::Tensor attention_window_bshd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, long gh, long gw, long th,
                                    long tw, double scale) {
  // softmax attention inside each th x tw window of the gh x gw token grid;
  // everything an address is formed from is checked here, so a bad argument
  // raises and never becomes an out-of-range read
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4,
              "attention_window: q/k/v must be [B,S,H,D]");
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda(),
              "attention_window: q/k/v must be on the GPU");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
                  k.scalar_type() == torch::kBFloat16 &&
                  v.scalar_type() == torch::kBFloat16 &&
                  flash_supported(q.size(3)),
              "attention_window: bf16 q/k/v with a supported head dim only");
  TORCH_CHECK(q.sizes() == k.sizes() && q.sizes() == v.sizes(),
              "attention_window: q, k and v shapes differ");
  TORCH_CHECK(q.size(0) > 0 && q.size(2) > 0,
              "attention_window: empty q/k/v");
  TORCH_CHECK(gh > 0 && gw > 0 && gh <= (1L << 30) / gw,
              "attention_window: grid must be positive and below 2^30 tokens");
  TORCH_CHECK(q.size(1) == gh * gw, "attention_window: grid ", gh, "x", gw,
              " does not match the token count ", q.size(1));
  TORCH_CHECK(th > 0 && th <= gh && gh % th == 0,
              "attention_window: window height ", th,
              " must divide the grid height ", gh);
  TORCH_CHECK(tw > 0 && tw <= gw && gw % tw == 0,
              "attention_window: window width ", tw,
              " must divide the grid width ", gw);
  for (const auto &t : {q, k, v}) {
    bool rows16 = t.stride(3) == 1 && ((uintptr_t)t.data_ptr()) % 16 == 0;
    for (int i = 0; i < 3; ++i)
      rows16 = rows16 && (t.size(i) == 1 || t.stride(i) % 8 == 0);
    TORCH_CHECK(rows16,
                "attention_window: q/k/v need unit stride in D and "
                "16-byte-aligned rows");
  }
  return flash_window_raw(q, k, v, scale, gh, gw, th, tw);
}

torch::Tensor attention_blend_bshd(torch::Tensor q, torch::Tensor k,
                                   torch::Tensor v, torch::Tensor w,
                                   torch::Tensor kv_index,
                                   c10::optional<torch::Tensor> kv_len,
                                   double scale) {
  // sum_c w[b,c,s] * attention(q[b], k[kv_index[b,c]], v[kv_index[b,c]]);
  // the Python wrapper validates the table VALUES, this checks everything
  // the launch itself depends on
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4,
              "attention_blend: q/k/v must be [B,S,H,D]");
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda() && w.is_cuda() &&
                  kv_index.is_cuda(),
              "attention_blend: tensors must be on the GPU");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
                  k.scalar_type() == torch::kBFloat16 &&
                  v.scalar_type() == torch::kBFloat16 &&
                  flash_supported(q.size(3)),
              "attention_blend: bf16 with supported head dim only");
  const long B = q.size(0), Sq = q.size(1), H = q.size(2), D = q.size(3);
  TORCH_CHECK(B > 0 && Sq > 0 && H > 0 && k.size(0) > 0 && k.size(1) > 0,
              "attention_blend: empty q/k/v");
  TORCH_CHECK(k.sizes() == v.sizes() && k.size(2) == H && k.size(3) == D,
              "attention_blend: k/v shape mismatch");
  for (const auto &t : {q, k, v}) {
    bool rows16 = t.stride(3) == 1 && ((uintptr_t)t.data_ptr()) % 16 == 0;
    for (int i = 0; i < 3; ++i)
      rows16 = rows16 && (t.size(i) == 1 || t.stride(i) % 8 == 0);
    TORCH_CHECK(rows16,
                "attention_blend: q/k/v need unit stride in D and "
                "16-byte-aligned rows");
  }
  TORCH_CHECK(w.scalar_type() == torch::kFloat && w.dim() == 3 &&
                  (w.size(0) == B || w.size(0) == 1) && w.size(1) >= 1 &&
                  w.size(2) == Sq && w.stride(2) == 1,
              "attention_blend: w must be fp32 [B or 1, C, Sq], unit stride "
              "in Sq");
  const long C = w.size(1);
  TORCH_CHECK(kv_index.scalar_type() == torch::kInt &&
                  kv_index.is_contiguous() && kv_index.numel() == B * C,
              "attention_blend: kv_index must be contiguous int32 [B, C]");
  if (kv_len.has_value()) {
    TORCH_CHECK(kv_len->is_cuda() && kv_len->scalar_type() == torch::kInt &&
                    kv_len->is_contiguous() && kv_len->numel() == k.size(0),
                "attention_blend: kv_len must be contiguous int32 [Bk]");
  }
  return flash_blend_raw(q, k, v, w, kv_index, kv_len, scale);
}

// ---------------------------------------------------------------------------
// counter-based noise (rng.hip): Philox4x32-10 + Box-Muller
// ---------------------------------------------------------------------------
torch::Tensor philox4x32(torch::Tensor counter, torch::Tensor key) {
  CHECK_IN(counter);
  CHECK_IN(key);
  TORCH_CHECK(counter.scalar_type() == torch::kLong &&
                  key.scalar_type() == torch::kLong && counter.dim() == 2 &&
                  key.dim() == 2 && counter.size(1) == 4 &&
                  key.size(1) == 2 && counter.size(0) == key.size(0),
              "philox4x32: int64 counter [N,4] and key [N,2]");
  auto out = torch::empty_like(counter);
  const long n = counter.size(0);
  if (n == 0) return out;
  hipLaunchKernelGGL(philox4x32_kernel, dim3(ew_grid(n)), dim3(256), 0,
                     cur_stream(), (const long long *)counter.data_ptr(),
                     (const long long *)key.data_ptr(),
                     (long long *)out.data_ptr(), n);
  return out;
}

static void check_philox_seeds(const torch::Tensor &seeds, long B,
                               const torch::Tensor *like) {
  TORCH_CHECK(seeds.is_cuda() && seeds.scalar_type() == torch::kLong &&
                  seeds.dim() == 1 && seeds.is_contiguous() &&
                  seeds.size(0) == B,
              "philox: seeds must be a contiguous int64 [B] on the GPU");
  TORCH_CHECK(!like || seeds.device() == like->device(),
              "philox: seeds and x must share a device");
}

static void check_philox_offset(long off_lo, long off_hi) {
  TORCH_CHECK(off_lo >= 0 && off_lo <= 0xFFFFFFFFL && off_hi >= 0 &&
                  off_hi <= 0xFFFFFFFFL,
              "philox: the offset halves are 32-bit words");
}

// [B, n] normals; row b is draw (off_hi:off_lo) of the generator seeds[b]
torch::Tensor philox_randn(torch::Tensor seeds, long off_lo, long off_hi,
                           long n, bool bf16) {
  TORCH_CHECK(seeds.dim() == 1, "philox_randn: seeds must be [B]");
  const long B = seeds.size(0);
  check_philox_seeds(seeds, B, nullptr);
  check_philox_offset(off_lo, off_hi);
  TORCH_CHECK(n >= 0 && n < (1L << 32), "philox_randn: n must be < 2^32");
  auto out = torch::empty(
      {B, n}, seeds.options().dtype(bf16 ? torch::kBFloat16 : torch::kFloat));
  const long total = B * n;
  if (total == 0) return out;
  if (bf16) {
    const long nv = total / 8;
    hipLaunchKernelGGL(philox_randn_kernel<__hip_bfloat16>,
                       dim3(ew_grid(nv ? nv : total)), dim3(256), 0,
                       cur_stream(), (const long long *)seeds.data_ptr(),
                       (__hip_bfloat16 *)out.data_ptr(), (unsigned)off_lo,
                       (unsigned)off_hi, (unsigned)n, nv, total);
  } else {
    const long nv = total / 4;
    hipLaunchKernelGGL(philox_randn_kernel<float>,
                       dim3(ew_grid(nv ? nv : total)), dim3(256), 0,
                       cur_stream(), (const long long *)seeds.data_ptr(),
                       out.data_ptr<float>(), (unsigned)off_lo,
                       (unsigned)off_hi, (unsigned)n, nv, total);
  }
  return out;
}

// a*x + b*randn(seeds[img], offset, j) for x [B,C,H,W], contiguous or
// channels_last; the result keeps x's memory format
torch::Tensor axpby_philox(torch::Tensor x, torch::Tensor seeds, long off_lo,
                           long off_hi, double a, double b) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "axpby_philox: x must be a GPU "
                                           "[B,C,H,W] tensor");
  const bool cl = !x.is_contiguous() &&
                  x.is_contiguous(torch::MemoryFormat::ChannelsLast);
  TORCH_CHECK(x.is_contiguous() || cl,
              "axpby_philox: x must be contiguous or channels_last");
  const long B = x.size(0), C = x.size(1);
  const long HW = x.size(2) * (long)x.size(3);
  const long n = C * HW;
  check_philox_seeds(seeds, B, &x);
  check_philox_offset(off_lo, off_hi);
  TORCH_CHECK(n < (1L << 32), "axpby_philox: C*H*W must be < 2^32");
  auto out = torch::empty_like(x);  // keeps x's strides
  const long total = B * n;
  if (total == 0) return out;
  // a view at an odd storage offset is re-materialised for the 16 B loads
  if (reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 != 0) x = x.clone();
  auto launch = [&](auto kern, auto *xp, auto *op, long vec) {
    const long nv = total / vec;
    hipLaunchKernelGGL(kern, dim3(ew_grid(nv ? nv : total)), dim3(256), 0,
                       cur_stream(), xp, (const long long *)seeds.data_ptr(),
                       op, (float)a, (float)b, (unsigned)off_lo,
                       (unsigned)off_hi, (unsigned)n, (unsigned)C,
                       (unsigned)HW, nv, total);
  };
  if (x.scalar_type() == torch::kBFloat16) {
    auto *xp = (const __hip_bfloat16 *)x.data_ptr();
    auto *op = (__hip_bfloat16 *)out.data_ptr();
    if (cl)
      launch(axpby_philox_kernel<__hip_bfloat16, true>, xp, op, 8);
    else
      launch(axpby_philox_kernel<__hip_bfloat16, false>, xp, op, 8);
  } else if (x.scalar_type() == torch::kFloat) {
    auto *xp = (const float *)x.data_ptr();
    auto *op = (float *)out.data_ptr();
    if (cl)
      launch(axpby_philox_kernel<float, true>, xp, op, 4);
    else
      launch(axpby_philox_kernel<float, false>, xp, op, 4);
  } else {
    TORCH_CHECK(false, "axpby_philox: unsupported dtype");
  }
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("silu", &silu);
  m.def("geglu", &geglu);
  m.def("axpby", &axpby);
  m.def("euler_step", &euler_step);
  m.def("philox4x32", &philox4x32);
  m.def("philox_randn", &philox_randn);
  m.def("axpby_philox", &axpby_philox);
  m.def("group_norm_silu", &group_norm_silu);
  m.def("group_norm_silu_pre", &group_norm_silu_pre);
  m.def("gn_tile_stats", &gn_tile_stats);
  m.def("add_gn", &add_gn);
  m.def("layer_norm", &layer_norm);
  m.def("add_layer_norm", &add_layer_norm);
  m.def("add_layer_norm_gather", &add_layer_norm_gather);
  m.def("tome_match_supported_width", &tome_match_supported_width);
  m.def("tome_match", &tome_match);
  m.def("tome_merge", &tome_merge);
  m.def("tome_unmerge", &tome_unmerge);
  m.def("row_softmax_", &row_softmax_);
  m.def("attention_fwd", &attention_fwd, py::arg("q"), py::arg("k"),
        py::arg("v"), py::arg("scale"), py::arg("force") = 0);
  m.def("attention_fwd_bshd", &attention_fwd_bshd, py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("scale"), py::arg("force") = 0);
  m.def("attention_plan", &attention_plan);
  m.def("attention_blend_bshd", &attention_blend_bshd, py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("w"), py::arg("kv_index"),
        py::arg("kv_len"), py::arg("scale"));
  m.def("attention_blend_plan", &attention_blend_plan);
  m.def("attention_window_bshd", &attention_window_bshd, py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("gh"), py::arg("gw"),
        py::arg("th"), py::arg("tw"), py::arg("scale"));
  m.def("attention_window_plan", &attention_window_plan);
  m.def("probe_mfma32", &probe_mfma32);
  m.def("probe_mfma16", &probe_mfma16);
  m.def("probe_tr16", &probe_tr16);
  m.def("flash_supported", &flash_supported);
  // the wrap flags (seamless tiling) go last, defaulted: earlier callers
  // pass everything before them positionally
  m.def("conv3x3_nhwc", &conv3x3_nhwc, py::arg("x"), py::arg("w_prep"),
        py::arg("bias"), py::arg("residual"), py::arg("chan_bias"),
        py::arg("stride"), py::arg("collect_gn"), py::arg("force"),
        py::arg("wrap_h") = false, py::arg("wrap_w") = false);
  m.def("conv3x3_supported", &conv3x3_supported);
  m.def("conv3x3_plan", &conv3x3_plan);
  m.def("conv3x3_small", &conv3x3_small, py::arg("x"), py::arg("w_prep"),
        py::arg("bias"), py::arg("stride"), py::arg("wrap_h") = false,
        py::arg("wrap_w") = false);
  m.def("ups2x_conv3x3", &ups2x_conv3x3, py::arg("x"), py::arg("w_prep"),
        py::arg("bias"), py::arg("collect_gn"), py::arg("wrap_h") = false,
        py::arg("wrap_w") = false, py::arg("w_fold") = py::none(),
        py::arg("fold") = true);
  m.def("conv3x3_small_supported", &conv3x3_small_supported);
}
