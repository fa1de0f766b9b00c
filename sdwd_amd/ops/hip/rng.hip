// Counter-based noise: Philox4x32-10 + Box-Muller, keyed by the image seed
// (the host application's "NV" random source; docs/usage.md has the
// definition). Element j of draw `offset` of image `seed` is a pure function
// of (seed, offset, j): counter (offset_lo, offset_hi, j, 0), key (seed_lo,
// seed_hi), words 0 and 1 of the output make ONE normal. Do not widen this to
// four normals per counter: the stream would no longer be that source.
#include "common.h"

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

struct philox_words {
  unsigned x0, x1, x2, x3;
};

__device__ __forceinline__ philox_words philox4x32_10(unsigned c0, unsigned c1,
                                                      unsigned c2, unsigned c3,
                                                      unsigned k0,
                                                      unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(PHILOX_M0, c0), l0 = PHILOX_M0 * c0;
    const unsigned h1 = __umulhi(PHILOX_M1, c2), l1 = PHILOX_M1 * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  return {c0, c1, c2, c3};
}

// u in (0, 1], v in (0, 2*pi]; the precise libm calls, not the fast
// intrinsics (the CPU op is the oracle and uses the same three functions)
__device__ __forceinline__ float philox_normal(unsigned long long seed,
                                               unsigned off_lo,
                                               unsigned off_hi, unsigned j) {
  const philox_words w = philox4x32_10(off_lo, off_hi, j, 0u, (unsigned)seed,
                                       (unsigned)(seed >> 32));
  const float u = (float)w.x0 * 2.3283064365386963e-10f   // 2^-32
                  + 1.1641532182693481e-10f;              // 2^-33
  const float v = (float)w.x1 * 1.4629180792671596e-09f   // 2*pi * 2^-32
                  + 7.3145903963357980e-10f;              // 2*pi * 2^-33
  return sqrtf(-2.0f * logf(u)) * sinf(v);
}

// raw core at arbitrary counters/keys (bit-exact tests): int64 tensors that
// hold uint32 values, counters [N,4], keys [N,2], out [N,4]
__global__ void philox4x32_kernel(const long long *__restrict__ counter,
                                  const long long *__restrict__ key,
                                  long long *__restrict__ out, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const philox_words w = philox4x32_10(
        (unsigned)counter[i * 4], (unsigned)counter[i * 4 + 1],
        (unsigned)counter[i * 4 + 2], (unsigned)counter[i * 4 + 3],
        (unsigned)key[i * 2], (unsigned)key[i * 2 + 1]);
    out[i * 4] = w.x0;
    out[i * 4 + 1] = w.x1;
    out[i * 4 + 2] = w.x2;
    out[i * 4 + 3] = w.x3;
  }
}

template <typename T> struct rng_io;
template <> struct rng_io<float> {
  static constexpr int VEC = 4;
  typedef f32x4 vec;
  typedef float elt;
  static __device__ __forceinline__ float ld(const float *p) { return *p; }
  static __device__ __forceinline__ void st(float *p, float v) { *p = v; }
};
template <> struct rng_io<__hip_bfloat16> {
  static constexpr int VEC = 8;
  typedef bf16x8 vec;
  typedef __bf16 elt;
  static __device__ __forceinline__ float ld(const __hip_bfloat16 *p) {
    return bf2f(*p);
  }
  static __device__ __forceinline__ void st(__hip_bfloat16 *p, float v) {
    *p = f2bf(v);
  }
};

// Walks the memory positions of a [B, n] buffer one element at a time from
// `start`: a 16 B group may straddle two images when n % VEC != 0, so the
// image and the logical index j are kept per element. CL: the buffer is
// [B, H*W, C] (channels_last) and position m = p*C + c has j = c*H*W + p.
template <bool CL> struct rng_pos {
  long img;
  unsigned m, c, p;
  unsigned n, C, HW;
  __device__ __forceinline__ rng_pos(long start, unsigned n_, unsigned C_,
                                     unsigned HW_)
      : n(n_), C(C_), HW(HW_) {
    img = start / (long)n_;
    m = (unsigned)(start - img * (long)n_);
    if (CL) {
      p = m / C_;
      c = m - p * C_;
    }
  }
  __device__ __forceinline__ unsigned j() const {
    return CL ? c * HW + p : m;
  }
  __device__ __forceinline__ void next() {
    if (++m == n) {
      m = 0;
      ++img;
      if (CL) c = p = 0;
    } else if (CL && ++c == C) {
      c = 0;
      ++p;
    }
  }
};

// out[b, j] = randn(seeds[b], offset, j); out contiguous [B, n], n < 2^32
template <typename T>
__global__ void philox_randn_kernel(const long long *__restrict__ seeds,
                                    T *__restrict__ out, unsigned off_lo,
                                    unsigned off_hi, unsigned n, long n_vec,
                                    long n_total) {
  typedef rng_io<T> io;
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x;
  for (long i = tid; i < n_vec; i += stride) {
    rng_pos<false> pos(i * io::VEC, n, 1u, n);
    typename io::vec o;
#pragma unroll
    for (int e = 0; e < io::VEC; ++e) {
      o[e] = (typename io::elt)philox_normal(
          (unsigned long long)seeds[pos.img], off_lo, off_hi, pos.j());
      pos.next();
    }
    ((typename io::vec *)out)[i] = o;
  }
  for (long i = n_vec * io::VEC + tid; i < n_total; i += stride) {
    rng_pos<false> pos(i, n, 1u, n);
    io::st(out + i, philox_normal((unsigned long long)seeds[pos.img], off_lo,
                                  off_hi, pos.j()));
  }
}

// out = a*x + b*randn(seeds[img], offset, j), fp32 math; x/out share one
// memory format ([B, n] rows, CL as above), 16 B per lane, grid-stride
template <typename T, bool CL>
__global__ void axpby_philox_kernel(const T *__restrict__ x,
                                    const long long *__restrict__ seeds,
                                    T *__restrict__ out, float a, float b,
                                    unsigned off_lo, unsigned off_hi,
                                    unsigned n, unsigned C, unsigned HW,
                                    long n_vec, long n_total) {
  typedef rng_io<T> io;
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x;
  for (long i = tid; i < n_vec; i += stride) {
    rng_pos<CL> pos(i * io::VEC, n, C, HW);
    const typename io::vec vx = ((const typename io::vec *)x)[i];
    typename io::vec o;
#pragma unroll
    for (int e = 0; e < io::VEC; ++e) {
      const float r = philox_normal((unsigned long long)seeds[pos.img],
                                    off_lo, off_hi, pos.j());
      o[e] = (typename io::elt)(a * (float)vx[e] + b * r);
      pos.next();
    }
    ((typename io::vec *)out)[i] = o;
  }
  for (long i = n_vec * io::VEC + tid; i < n_total; i += stride) {
    rng_pos<CL> pos(i, n, C, HW);
    const float r = philox_normal((unsigned long long)seeds[pos.img], off_lo,
                                  off_hi, pos.j());
    io::st(out + i, a * io::ld(x + i) + b * r);
  }
}
