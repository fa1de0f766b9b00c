// Token merging: the merge plan in one launch, gfx950.
//
// tome_plan_kernel turns the match's (node_max fp32, node_idx int32) [B,Ns]
// into the four int32 tables of a TomePlan (ops/__init__.py, tome_plan: that
// torch code is the definition, and the result is equal to it, not close):
// slot [B,N], unm_tok [B,Ns-r], seg_start [B,Nd+1], members [B,r].
//
// One workgroup of 16 waves per batch row; the row never leaves LDS and no
// second launch or global scratch exists. Src position i belongs to thread
// i % 1024 in round i / 1024, so a wave's lanes hold consecutive positions
// and (round, wave) pairs ascend with i: 16 x 16 = 256 of them at the most,
// which is the one table shape every scan here has.
//
//  1. Keys. node_max -> uint32 that orders as torch's stable descending sort
//     compares: NaN above everything, -0.0 == +0.0, +-inf in their places.
//     Stored in buf[i].
//  2. Radix select of the r-th largest key: four passes over a 256-bin LDS
//     histogram of the next byte among the keys that share the prefix found
//     so far. The bins are filled by integer LDS adds (order-independent);
//     a wave whose candidates all carry the same byte - cosine scores share
//     their exponent - adds its count once. Wave 0 scans the bins from the
//     top and picks the one that holds rank r. The result is the threshold
//     key and `take`, how many keys EQUAL to it are merged.
//  3. Ties at the threshold go to the lower src position: the exclusive scan
//     of the "equals threshold" flags ranks them. Flag scans are a ballot and
//     a popcount of the lower lanes; the per-(round, wave) counts go to a
//     256-entry table that wave 0 scans once (four entries per lane, then
//     __shfl_up).
//  4. The same scan over "not merged" gives urank, hence slot and unm_tok.
//     A merged token's rank among the merged is i - urank; it writes the
//     composite key didx << 14 | i to buf[i - urank]: in place, since every
//     key has been read by then (the merged flags sit in a register bitmask).
//  5. CSR. The composite keys are sorted in LDS by a bitonic network (padded
//     with ~0 to a power of two; strides below 64 run in registers through
//     __shfl_xor, the rest through LDS). Sorted, they are members in the
//     order the plan wants - by dst, then by ascending position - whatever
//     the segment lengths are: one dst may own all r. seg_start[d] is the
//     lower bound of d << 14, a binary search per dst.
//
// Nothing depends on scheduling, there are no global atomics, and every
// global address comes from a loop bound or a clamped table entry.
#include "common.h"

static constexpr int TP_THREADS = 1024;
static constexpr int TP_WAVES = TP_THREADS / WAVE;
static constexpr int TP_POS_BITS = 14;  // src position field of a composite
static constexpr int TP_MAX_TOKENS = 1 << TP_POS_BITS;  // 16 rounds
static_assert(TP_MAX_TOKENS == TP_THREADS * TP_WAVES,
              "tome_plan: the (round, wave) table has 256 entries");

__device__ __forceinline__ unsigned tome_plan_key(float f) {
  if (f != f) return 0xFFFFFFFFu;
  const unsigned u = __float_as_uint(f == 0.f ? 0.f : f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int tome_plan_clamp(int v, int hi /*exclusive*/) {
  return v < 0 ? 0 : (v >= hi ? hi - 1 : v);
}

// Exclusive prefix sum of tab[0..256) in place, by ONE full wave: lane l owns
// entries 4l..4l+3. Returns the lane's exclusive prefixes, cnt its entries.
__device__ __forceinline__ uint4 tome_plan_scan256(unsigned *tab, int lane,
                                                   uint4 &cnt) {
  cnt = ((const uint4 *)tab)[lane];
  const unsigned own = cnt.x + cnt.y + cnt.z + cnt.w;
  unsigned inc = own;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const unsigned o = __shfl_up(inc, off, WAVE);
    if (lane >= off) inc += o;
  }
  uint4 ex;
  ex.x = inc - own;
  ex.y = ex.x + cnt.x;
  ex.z = ex.y + cnt.y;
  ex.w = ex.z + cnt.z;
  ((uint4 *)tab)[lane] = ex;
  return ex;
}

// Ascending bitonic sort of s[0..n), n a power of two >= 64, by the whole
// workgroup. Element e sits at lane e % 64 in the register phases, so a
// partner at a stride below 64 is a lane of the same wave.
__device__ __forceinline__ void tome_plan_sort(unsigned *s, int n, int tid) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j >= WAVE; j >>= 1) {
      for (int t = tid; t < n / 2; t += TP_THREADS) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int hi = lo | j;
        const unsigned a = s[lo], b = s[hi];
        if ((a > b) == ((lo & k) == 0)) {
          s[lo] = b;
          s[hi] = a;
        }
      }
      __syncthreads();
    }
    const int j0 = k >> 1 < WAVE ? k >> 1 : WAVE / 2;
    for (int e = tid; e < n; e += TP_THREADS) {  // whole waves: n % 64 == 0
      unsigned v = s[e];
      const bool up = (e & k) == 0;
      for (int j = j0; j >= 1; j >>= 1) {
        const unsigned o = __shfl_xor(v, j, WAVE);
        const bool keep_min = ((e & j) == 0) == up;
        v = keep_min ? (v < o ? v : o) : (v > o ? v : o);
      }
      s[e] = v;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(TP_THREADS) void tome_plan_kernel(
    const float *__restrict__ node_max, const int *__restrict__ node_idx,
    const int *__restrict__ src_tok, const int *__restrict__ dst_tok,
    int *__restrict__ slot, int *__restrict__ unm_tok,
    int *__restrict__ seg_start, int *__restrict__ members, int N, int Ns,
    int Nd, int r) {
  __shared__ unsigned buf[TP_MAX_TOKENS];  // keys, then composite keys
  __shared__ __align__(16) unsigned hist[256];
  __shared__ __align__(16) unsigned tab_eq[256];
  __shared__ __align__(16) unsigned tab_un[256];
  __shared__ unsigned sel[2];  // threshold key, keys equal to it to take

  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int lane = tid % WAVE;
  const long bb = blockIdx.x;
  const int rounds = (Ns + TP_THREADS - 1) / TP_THREADS;  // <= 16
  const int nu = Ns - r;
  const unsigned long long lower = (1ull << lane) - 1ull;

  const float *nm = node_max + bb * Ns;
  const int *ni = node_idx + bb * Ns;
  int *slot_b = slot + bb * N;
  int *unm_b = unm_tok + bb * nu;
  int *seg_b = seg_start + bb * (Nd + 1);
  int *mem_b = members + bb * r;

  // 1. keys; the scan tables start at zero (rounds past Ns stay zero)
  for (int i = tid; i < Ns; i += TP_THREADS) buf[i] = tome_plan_key(nm[i]);
  if (tid < 256) {
    tab_eq[tid] = 0;
    tab_un[tid] = 0;
  }
  if (tid == 0) {  // r == 0: no key is above or equal-and-taken
    sel[0] = 0xFFFFFFFFu;
    sel[1] = 0;
  }
  __syncthreads();

  // 2. radix select, most significant byte first. Bin 255 - byte, so the
  // exclusive prefix of a bin counts the candidates with a LARGER byte.
  if (r > 0) {
    unsigned prefix = 0, rem = (unsigned)r;
    for (int shift = 24; shift >= 0; shift -= 8) {
      const unsigned hmask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int q = 0; q < rounds; ++q) {
        const int i = q * TP_THREADS + tid;
        const unsigned key = i < Ns ? buf[i] : 0u;
        const bool cand = i < Ns && (key & hmask) == prefix;
        const unsigned bin = 255u - ((key >> shift) & 255u);
        const unsigned long long bc = __ballot(cand);
        if (bc == 0) continue;
        const int first = __ffsll((long long)bc) - 1;
        const unsigned bin0 = __shfl(bin, first, WAVE);
        if (__ballot(cand && bin == bin0) == bc) {
          if (lane == first) atomicAdd(&hist[bin0], (unsigned)__popcll(bc));
        } else if (cand) {
          atomicAdd(&hist[bin], 1u);
        }
      }
      __syncthreads();
      if (wid == 0) {
        uint4 cnt;
        const uint4 ex = tome_plan_scan256(hist, lane, cnt);
        const unsigned e[4] = {ex.x, ex.y, ex.z, ex.w};
        const unsigned c[4] = {cnt.x, cnt.y, cnt.z, cnt.w};
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (e[t] < rem && rem <= e[t] + c[t]) {  // exactly one bin
            sel[0] = prefix | ((255u - (unsigned)(4 * lane + t)) << shift);
            sel[1] = rem - e[t];
          }
      }
      __syncthreads();
      prefix = sel[0];
      rem = sel[1];
    }
  }
  const unsigned thr = sel[0];
  const unsigned take = sel[1];

  // 3. rank the keys equal to the threshold by position
  for (int q = 0; q < rounds; ++q) {
    const int i = q * TP_THREADS + tid;
    const bool eq = i < Ns && buf[i] == thr;
    const unsigned long long be = __ballot(eq);
    if (lane == 0) tab_eq[q * TP_WAVES + wid] = (unsigned)__popcll(be);
  }
  __syncthreads();
  if (wid == 0) {
    uint4 cnt;
    tome_plan_scan256(tab_eq, lane, cnt);
  }
  __syncthreads();

  // merged flags (bit q of mbits: this thread's token of round q)
  unsigned mbits = 0;
  for (int q = 0; q < rounds; ++q) {
    const int i = q * TP_THREADS + tid;
    const unsigned key = i < Ns ? buf[i] : 0u;
    const bool eq = i < Ns && key == thr;
    const unsigned long long be = __ballot(eq);
    const unsigned eqrank =
        tab_eq[q * TP_WAVES + wid] + (unsigned)__popcll(be & lower);
    const bool merged = i < Ns && (key > thr || (eq && eqrank < take));
    mbits |= (unsigned)merged << q;
    const unsigned long long bu = __ballot(i < Ns && !merged);
    if (lane == 0) tab_un[q * TP_WAVES + wid] = (unsigned)__popcll(bu);
  }
  __syncthreads();  // every key has been read: buf is free from here on
  if (wid == 0) {
    uint4 cnt;
    tome_plan_scan256(tab_un, lane, cnt);
  }
  __syncthreads();

  // 4. slot, unm_tok, and the composite keys of the merged tokens
  const int nsort = r <= WAVE ? WAVE : 1 << (32 - __clz(r - 1));
  for (int p = r + tid; p < nsort; p += TP_THREADS) buf[p] = 0xFFFFFFFFu;
  for (int q = 0; q < rounds; ++q) {
    const int i = q * TP_THREADS + tid;
    const bool valid = i < Ns;
    const bool merged = (mbits >> q) & 1u;
    const unsigned long long bu = __ballot(valid && !merged);
    const int urank =
        (int)(tab_un[q * TP_WAVES + wid] + (unsigned)__popcll(bu & lower));
    if (!valid) continue;
    const int tok = tome_plan_clamp(src_tok[i], N);
    if (merged) {
      const int d = tome_plan_clamp(ni[i], Nd);
      slot_b[tok] = nu + d;
      const int mrank = i - urank;
      if (mrank < r) buf[mrank] = ((unsigned)d << TP_POS_BITS) | (unsigned)i;
    } else {
      slot_b[tok] = urank;
      if (urank < nu) unm_b[urank] = tok;
    }
  }
  for (int j = tid; j < Nd; j += TP_THREADS)
    slot_b[tome_plan_clamp(dst_tok[j], N)] = nu + j;
  __syncthreads();

  // 5. members and seg_start from the sorted composite keys
  if (r > 0) tome_plan_sort(buf, nsort, tid);
  for (int p = tid; p < r; p += TP_THREADS) {
    const int i = tome_plan_clamp((int)(buf[p] & (TP_MAX_TOKENS - 1)), Ns);
    mem_b[p] = tome_plan_clamp(src_tok[i], N);
  }
  for (int d = tid; d <= Nd; d += TP_THREADS) {
    const unsigned target = (unsigned)d << TP_POS_BITS;
    int lo = 0, hi = r;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (buf[mid] < target) lo = mid + 1;
      else hi = mid;
    }
    seg_b[d] = lo;
  }
}
