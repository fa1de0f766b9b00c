// Flash attention forward for the wide head dims 256 and 512 (the VAE
// mid-block: one head, D = 512) on gfx950. Included after attention.hip: it
// reuses AttnStrides / attn_strides, load_q_frags and dispatch_dpad_in from
// there (crow, p_relayout and the shuffle are common.h's) and leaves that
// file alone.
//
// Why a kernel of its own: v2/v3 keep a wave's O tile and Q fragments in
// registers for QS sub-tiles under two blocks per CU (256 registers a lane).
// At D = 512 one 32-row sub-tile alone is 256 (O) + 128 (Q) registers. So:
//
//  * work split: 4 waves, __launch_bounds__(256, 1): one wave per SIMD, the
//    unified 512 registers a lane. Each wave owns ONE 32-row q sub-tile, a
//    block covers 128 q rows, grid = (ceil(Sq / 128), B * H).
//  * registers at DPAD 512: O 32 x 512 fp32 = 256 (the MFMA accumulator,
//    AGPRs), Q fragments 32 chunks x 4 = 128 (read once), scores 16, the two
//    P A-fragments 8, one operand's staged tile 32.
//  * LDS: K and V tiles of KVB keys, row-major, rows padded by 8 bf16 (row
//    stride 1040 B = 65 16-byte slots at DPAD 512, 33 at 256: odd, so the 32
//    rows a b128 fragment read touches fall in distinct slots). One tile is
//    16 Ki elements whatever DPAD is (KVB = 32 at 512, 64 at 256), K and V
//    double-buffered: 133,120 B / 135,168 B of the 160 KiB, ONE barrier per
//    tile (tile t+1 is written into buffer cur^1 while cur is read; the
//    barrier of tile t-1 saw every read of cur^1 finish).
//  * staging: through registers, one operand in flight at a time. Next-K is
//    issued before the QK^T phase and written to LDS after it, next-V is
//    issued before softmax + PV and written after it: 8 b128 pieces a thread
//    each (32 registers, not 64), the same count for every thread, so no
//    wave idles at the barrier.
//  * arithmetic: v2's. Swapped QK^T (S^T = mfma(K_frag, Q_frag)), fp32
//    scores scaled by scale*log2(e) after the MFMA (Q is never pre-scaled),
//    base-2 online softmax, l from the unrounded fp32 P, P rounded to bf16
//    once and relaid with the permlane swap, V fragments by the hardware
//    transpose read, fp32 O, one bf16 rounding of the output. Defer-max with
//    v3's threshold (2^8): with O in AGPRs a rescale is 256 reads, multiplies
//    and writes, more VALU time than the tile's 64 MFMAs, so it must be rare.
//  * tails: q rows past Sq re-read the last row and are never stored; keys
//    past Sk are staged as a clamped re-read and masked on the ragged last
//    tile only. No address is formed from an unclamped row.
//  * D == DPAD only: no in-D masking anywhere.

template <int DPAD>
struct WideGeom {
  static_assert(DPAD == 256 || DPAD == 512, "wide head dims are 256 and 512");
  static constexpr int KVB = 16384 / DPAD;  // keys per staged tile
  static constexpr int PADK = 8;            // bf16 row pad: odd 16-byte slots
  static constexpr int RS = DPAD + PADK;    // LDS row stride (elements)
  static constexpr int NSUB = KVB / 32;     // 32-key S^T sub-tiles per tile
  static constexpr int NC = DPAD / 16;      // QK^T k-chunks
  static constexpr int ND = DPAD / 32;      // O accumulator tiles
  static constexpr int PPR = DPAD / 8;      // 16-byte pieces per row
  static constexpr int RPS = 256 / PPR;     // rows the block stages per step
  static constexpr int NST = KVB / RPS;     // pieces per thread and operand
  static constexpr int QROWS = 128;         // q rows per block (4 waves x 32)
  static constexpr int FB = 4;              // LDS fragments per pipelined batch
};
constexpr int wide_q_rows() { return 128; }

typedef __attribute__((ext_vector_type(4))) int wide_i32x4;

// S^T accumulation with the accumulator in arch VGPRs. The compiler picks
// one MFMA form per function; with O filling all 256 AGPRs the builtin would
// put the 16 score registers there too (272 > 256: half of O and all of Q
// went to scratch). C/D of an MFMA sit in one file per instruction, so QK^T
// is spelled with "v" operands and PV keeps the builtin. FIRST starts the
// chain from a zero C. Same-accumulator MFMAs issue back to back; the chain's
// readers wait in wide_mfma_settle.
template <bool FIRST>
__device__ __forceinline__ void wide_mfma_vgpr(f32x16 &acc, const bf16x8 &a,
                                               const bf16x8 &b) {
  const wide_i32x4 ai = *(const wide_i32x4 *)&a, bi = *(const wide_i32x4 *)&b;
  if constexpr (FIRST)
    asm("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0"
        : "=&v"(acc)
        : "v"(ai), "v"(bi));
  else
    asm("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0"
        : "+v"(acc)
        : "v"(ai), "v"(bi));
}
// the wait states between the last MFMA of a chain and a VALU read of its
// result (passes + 2; 20 covers a 16-pass MFMA), which the compiler cannot
// count through inline assembly
__device__ __forceinline__ void wide_mfma_settle(f32x16 &acc) {
  asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc));
}

// O tile element *= a, in place in the AGPR it lives in. Written as plain
// `o[d][r] *= a` the allocator moves half of O to VGPRs for the whole loop
// and spills Q (1244 B/lane of scratch at DPAD 512). The reads are far from
// the PV MFMAs that wrote O: a barrier and the next QK^T phase lie between.
__device__ __forceinline__ void wide_scale_acc(f32x16 &tile, int r, float a) {
  float t;
  asm volatile("v_accvgpr_read_b32 %1, %0\n\t"
               "v_mul_f32 %1, %1, %2\n\t"
               "v_accvgpr_write_b32 %0, %1"
               : "+a"(tile[r]), "=&v"(t)
               : "v"(a));
}

template <int DPAD>
WIDE_KERNEL_ATTR __launch_bounds__(256, 1) __global__
void flash_wide_bf16_kernel(
    const __hip_bfloat16 *__restrict__ Q, const __hip_bfloat16 *__restrict__ K,
    const __hip_bfloat16 *__restrict__ V, __hip_bfloat16 *__restrict__ O,
    int H, long Sq, long Sk, float scale, AttnStrides st) {
  using G = WideGeom<DPAD>;
  constexpr int KVB = G::KVB, RS = G::RS, NSUB = G::NSUB, NC = G::NC,
                ND = G::ND, NST = G::NST, FB = G::FB;
  constexpr float THR = 8.0f;  // defer-max threshold (log2), as v3
  static_assert(G::QROWS == wide_q_rows(), "plan rows");

  __shared__ __align__(16) __bf16 kt[2][KVB][RS];
  __shared__ __align__(16) __bf16 vt[2][KVB][RS];

  const int bh = blockIdx.y;
  const int bb = bh / H, hh = bh % H;
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int lq = lane % 32;    // q row (softmax) / d column (PV C)
  const int half = lane / 32;  // half-wave id
  const long q0 = (long)blockIdx.x * G::QROWS + wid * 32;

  const __hip_bfloat16 *Qb = Q + bb * st.qb + hh * st.qh;
  const __hip_bfloat16 *Kb = K + bb * st.kb + hh * st.kh;
  const __hip_bfloat16 *Vb = V + bb * st.vb + hh * st.vh;
  __hip_bfloat16 *Ob = O + bb * st.ob + hh * st.oh;

  bf16x8 qf[NC];
  load_q_frags<false>(qf, Qb, st.qr, q0 + lq, Sq, DPAD, half);

  // staging: piece s of a thread is row s * RPS + sr, 8 elements at sc * 8;
  // a wave reads whole rows (DPAD 512: one row of 1 KiB per wave and step)
  const int sr = threadIdx.x / G::PPR, sc = threadIdx.x % G::PPR;
  const __hip_bfloat16 *Kc = Kb + sc * 8, *Vc = Vb + sc * 8;
  const int soff = sr * RS + sc * 8;
  // rows at or past Sk re-read the last key (masked at score time)
  const auto issue = [&](bf16x8(&stg)[NST], const __hip_bfloat16 *base,
                         long rstride, long kv)
                        __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < NST; ++s) {
      const long r = kv + s * G::RPS + sr;
      stg[s] = *(const bf16x8 *)(base + ((r < Sk) ? r : (Sk - 1)) * rstride);
    }
  };
  const auto commit = [&](__bf16 *tile, const bf16x8(&stg)[NST])
                         __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < NST; ++s)
      *(bf16x8 *)(tile + soff + s * G::RPS * RS) = stg[s];
  };

  // this lane's transpose-read base in a V tile (mapping decoded by
  // tools/tr16_probe.py, as v3): with this address lane l receives
  // V[k0 + 8 * half + j][d0 + l % 32], j = 0..3; rows j + 4 are 4 rows on
  const __bf16 *vlane = &vt[0][0][0] +
                        (((lane & 15) >> 2) + 8 * half) * RS +
                        4 * (lane & 3) + ((lane >> 4) & 1) * 16;

  f32x16 o[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) o[d] = (f32x16){};
  float m = -1e30f, l = 0.f;
  const float l2scale = scale * 1.4426950408889634f;

  {
    bf16x8 stg[NST];
    issue(stg, Kc, st.kr, 0);
    commit(&kt[0][0][0], stg);
    issue(stg, Vc, st.vr, 0);
    commit(&vt[0][0][0], stg);
  }
  wide_barrier();

  int cur = 0;
  for (long kv = 0; kv < Sk; kv += KVB, cur ^= 1) {
    const bool more = kv + KVB < Sk;
    bf16x8 stg[NST];
    if (more) issue(stg, Kc, st.kr, kv + KVB);

    // QK^T, software-pipelined by hand: the K fragments of batch b + 1 are
    // in flight under the MFMAs of batch b. The scheduling barriers keep the
    // compiler from hoisting all 32 fragment reads (128 registers) at once,
    // which spills the Q fragments.
    f32x16 s[NSUB];
    {
      bf16x8 kf[2][FB];
      const auto kload = [&](int b, bf16x8(&dst)[FB])
                             __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < FB; ++j) {
          const int i = b * FB + j, sub = i / NC, c = i % NC;
          dst[j] = *(const bf16x8 *)&kt[cur][sub * 32 + lq][c * 16 + 8 * half];
        }
      };
      kload(0, kf[0]);
#pragma unroll
      for (int b = 0; b < NSUB * NC / FB; ++b) {
        if (b + 1 < NSUB * NC / FB) kload(b + 1, kf[(b + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < FB; ++j) {
          const int i = b * FB + j, sub = i / NC, c = i % NC;
          if (c == 0) wide_mfma_vgpr<true>(s[sub], kf[b & 1][j], qf[c]);
          else wide_mfma_vgpr<false>(s[sub], kf[b & 1][j], qf[c]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int sub = 0; sub < NSUB; ++sub) wide_mfma_settle(s[sub]);
    }

    if (more) {
      commit(&kt[cur ^ 1][0][0], stg);
      issue(stg, Vc, st.vr, kv + KVB);
    }

    // scores to log2 units in fp32; the key mask only on the ragged tile
    float pmax = -1e30f;
    if (kv + KVB <= Sk) {
#pragma unroll
      for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[sub][r] *= l2scale;
          pmax = fmaxf(pmax, s[sub][r]);
        }
    } else {
#pragma unroll
      for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kk = sub * 32 + crow(r, half);
          s[sub][r] = (kv + kk < Sk) ? s[sub][r] * l2scale : -1e30f;
          pmax = fmaxf(pmax, s[sub][r]);
        }
    }
    pmax = fmaxf(pmax, wide_shfl(pmax, lane ^ 32));

    // defer-max: rescale only when some row's max grew past THR
    if (__builtin_amdgcn_ballot_w64(!(pmax <= m + THR)) != 0) {
      const float mnew = fmaxf(m, pmax);
      const float alpha = __builtin_amdgcn_exp2f(m - mnew);
      l *= alpha;
      m = mnew;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float a = wide_shfl(alpha, crow(r, half));
#pragma unroll
        for (int d = 0; d < ND; ++d) wide_scale_acc(o[d], r, a);
      }
    }
    float rowsum = 0.f;
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[sub][r] = __builtin_amdgcn_exp2f(s[sub][r] - m);
        rowsum += s[sub][r];
      }
    rowsum += wide_shfl(rowsum, lane ^ 32);
    l += rowsum;

    // PV: per 16-key chunk and 32-column O tile, two transpose reads give
    // the B fragment V[k..k+7][d column] from the row-major tile. Pipelined
    // in batches of FB fragments like QK^T.
    {
      bf16x8 pa[NSUB][2];
#pragma unroll
      for (int sub = 0; sub < NSUB; ++sub)
        p_relayout(s[sub], pa[sub][0], pa[sub][1]);
      bf16x8 vf[2][FB];
      const auto vload = [&](int b, bf16x8(&dst)[FB])
                             __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < FB; ++j) {
          const int i = b * FB + j, kc = i / ND, d = i % ND;  // kc: 16 keys
          const __bf16 *a = vlane + (cur * KVB + kc * 16) * RS + d * 32;
          const wide_bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (wide_lds_bf16x4 *)a);
          const wide_bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (wide_lds_bf16x4 *)(a + 4 * RS));
          dst[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
      };
      vload(0, vf[0]);
#pragma unroll
      for (int b = 0; b < NSUB * 2 * ND / FB; ++b) {
        if (b + 1 < NSUB * 2 * ND / FB) vload(b + 1, vf[(b + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < FB; ++j) {
          const int i = b * FB + j, kc = i / ND, d = i % ND;
          o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              pa[kc / 2][kc % 2], vf[b & 1][j], o[d], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    if (more) commit(&vt[cur ^ 1][0][0], stg);
    wide_barrier();
  }

  // epilogue: O / l, one bf16 rounding, rows past Sq not stored (store_row's
  // sequence with D == DPAD)
  const float linv = 1.0f / fmaxf(l, 1e-30f);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float inv = wide_shfl(linv, crow(r, half));
    const long qq = q0 + crow(r, half);
    if (qq >= Sq) continue;
#pragma unroll
    for (int d = 0; d < ND; ++d)
      Ob[qq * st.or_ + d * 32 + lq] = f2bf(o[d][r] * inv);
  }
}

// ---------------------------------------------------------------------------
// host-side dispatch (torch API lives in ext.hip which includes this file)
// ---------------------------------------------------------------------------
bool attention_wide_supported(long d_head) {
  return d_head == 256 || d_head == 512;
}

// The wide kernel's geometry: {padded head dim (== the head dim), q rows per
// workgroup}. Any other head dim is an error. The launcher below follows
// this and nothing else decides.
std::tuple<long, long> attention_wide_plan(long d_head) {
  TORCH_CHECK(attention_wide_supported(d_head), "attention_wide: head dim ",
              d_head, " has no wide flash kernel (256 and 512 do)");
  return {d_head, (long)wide_q_rows()};
}

#ifdef __HIP_PLATFORM_AMD__
// q [B,H,Sq,D], k/v [B,H,Sk,D] views (the caller checked everything an
// address is formed from)
static torch::Tensor flash_wide_raw(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, double scale) {
  const long B = q.size(0), H = q.size(1), Sq = q.size(2), D = q.size(3);
  const long Sk = k.size(2);
  auto out = torch::empty({B, H, Sq, D}, q.options());
  const AttnStrides st = attn_strides(q, k, v, out, /*bshd=*/false);
  const auto [dpad, qrows] = attention_wide_plan(D);
  const long rows = qrows;  // (a structured binding cannot be captured)
  const dim3 grid((unsigned)((Sq + rows - 1) / rows), (unsigned)(B * H));
  const dim3 block(256);
  auto stream = cur_stream();
  dispatch_dpad_in(
      dpad, "flash_wide",
      [&](auto dp) {
        constexpr int DP = decltype(dp)::value;
        TORCH_CHECK(rows == WideGeom<DP>::QROWS,
                    "flash_wide: plan rows do not match the instantiation");
        hipLaunchKernelGGL(flash_wide_bf16_kernel<DP>, grid, block, 0, stream,
                           (const __hip_bfloat16 *)q.data_ptr(),
                           (const __hip_bfloat16 *)k.data_ptr(),
                           (const __hip_bfloat16 *)v.data_ptr(),
                           (__hip_bfloat16 *)out.data_ptr(), (int)H, Sq, Sk,
                           (float)scale, st);
      },
      std::integer_sequence<int, 256, 512>{});
  return out;
}
#endif
