// Common device helpers for the msbn gfx950 (CDNA4) BatchNorm kernels.
//
// Design notes (MI355X-first, per /opt/skills/guides/cdna_hip_programming.md):
//  * wave64 is the scheduling quantum: all shuffle reductions are width-64.
//  * memory-bound kernels vectorize loads to 16 B/lane (Pack<T,V>).
//  * statistics reduce deterministically (no atomics) through a two-stage
//    (partial -> finalize) pipeline.  Each thread sums short fp32 chunks and
//    flushes them into fp64 totals (AccPair below).  fp64 totals alone do not
//    cure E[x^2]-E[x]^2 cancellation — raw squares are rounded in fp32 before
//    they reach them — so an ill-conditioned chunk is summed a second time
//    around its own mean (needs_recentre / unshift_pair below).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#define MSBN_WAVE 64
#define MSBN_BLOCK 256

namespace msbn {

// ---------------------------------------------------------------- vector pack
template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
  T v[V];
};

// ------------------------------------------------------------- dtype convert
__device__ __forceinline__ float to_f(float x) { return x; }
__device__ __forceinline__ float to_f(__hip_bfloat16 x) {
  return __bfloat162float(x);
}
__device__ __forceinline__ float to_f(__half x) { return __half2float(x); }

template <typename T>
__device__ __forceinline__ T from_f(float x);
template <>
__device__ __forceinline__ float from_f<float>(float x) {
  return x;
}
template <>
__device__ __forceinline__ __hip_bfloat16 from_f<__hip_bfloat16>(float x) {
  return __float2bfloat16(x);
}
template <>
__device__ __forceinline__ __half from_f<__half>(float x) {
  return __float2half(x);
}

// --------------------------------------------------- fused epilogue activation
// Compile-time activation mode of the fused BN(+add)+act epilogue.  kActNone
// is 0 so kernels can test `if (ACT)` for "there is a gate to recompute".
// The leaky slope is a runtime kernel argument, consulted by kActLeaky only.
constexpr int kActNone = 0;
constexpr int kActRelu = 1;
constexpr int kActLeaky = 2;

// forward: y = act(z)
template <int ACT>
__device__ __forceinline__ float act_fwd(float z, float slope) {
  if (ACT == kActRelu) return fmaxf(z, 0.f);
  if (ACT == kActLeaky) return z > 0.f ? z : slope * z;
  return z;
}

// backward: g = dy * act'(z); z == 0 takes the negative branch in both modes
// (stock threshold_backward / leaky_relu_backward convention).
//
// The branch is ONE predicate, act_pass: the forward may store it as a bit
// per element (gate bits, docs/KERNEL_DESIGN.md) and the backward then
// applies act_gate_bit to the stored bit instead of recomputing z, so the two
// cannot disagree.  A NaN z passes the gradient under relu (`z <= 0` is
// false) and takes the slope branch under leaky (`z > 0` is false).
template <int ACT>
__device__ __forceinline__ bool act_pass(float z) {
  if (ACT == kActRelu) return !(z <= 0.f);
  if (ACT == kActLeaky) return z > 0.f;
  return true;
}

template <int ACT>
__device__ __forceinline__ float act_gate_bit(bool pass, float g,
                                              float slope) {
  if (ACT == kActRelu) {
    if (!pass) g = 0.f;
  }
  if (ACT == kActLeaky) g = pass ? g : slope * g;
  return g;
}

template <int ACT>
__device__ __forceinline__ float act_gate(float z, float g, float slope) {
  return act_gate_bit<ACT>(act_pass<ACT>(z), g, slope);
}

// ------------------------------------------------------------------ gate bits
// One bit per element of a dense activation tensor: bit (e & 7) of byte
// (e >> 3) is act_pass<ACT>(z) of the element at storage offset e.  A V = 8
// forward thread owns one whole byte; a backward thread of any V <= 8 loads
// the byte its pack lies in (V divides 8 and e is a multiple of V, so a pack
// never straddles two bytes).  MSBN_GATE_STORE_NT / MSBN_GATE_LOAD_NT pick
// nontemporal byte accesses (A/B knobs; the defaults are what measured
// fastest, profiles/r08_gate_bits.md).
#ifndef MSBN_GATE_STORE_NT
#define MSBN_GATE_STORE_NT 0
#endif
#ifndef MSBN_GATE_LOAD_NT
#define MSBN_GATE_LOAD_NT 0
#endif

__device__ __forceinline__ void gate_store(unsigned char* gate, int64_t e,
                                           unsigned bits) {
#if MSBN_GATE_STORE_NT && !defined(MSBN_DISABLE_NT)
  __builtin_nontemporal_store((unsigned char)bits, &gate[e >> 3]);
#else
  gate[e >> 3] = (unsigned char)bits;
#endif
}

// the bits of the pack that starts at element e, bit k = element e + k
__device__ __forceinline__ unsigned gate_load(const unsigned char* gate,
                                              int64_t e) {
#if MSBN_GATE_LOAD_NT && !defined(MSBN_DISABLE_NT)
  const unsigned b = __builtin_nontemporal_load(&gate[e >> 3]);
#else
  const unsigned b = gate[e >> 3];
#endif
  return b >> (unsigned)(e & 7);
}

// ------------------------------------------------ nontemporal pack load/store
// Streaming tensors (activations / gradients: read or written exactly once
// per launch and far larger than L2) use nontemporal accesses — the nt cache
// bit keeps them from evicting the hot small data (per-channel coefs, fp64
// workspace) and measured slightly ahead of cached loads at BN shapes.
// Per-channel coefficient loads stay CACHED (reused by every block).
template <int BYTES>
struct NTVec;
template <>
struct NTVec<32> {  // 2x dwordx4 (e.g. fp32 V=8)
  using type = int __attribute__((vector_size(32)));
};
template <>
struct NTVec<16> {
  using type = int __attribute__((vector_size(16)));
};
template <>
struct NTVec<8> {
  using type = int __attribute__((vector_size(8)));
};
template <>
struct NTVec<4> {
  using type = int;
};
template <>
struct NTVec<2> {
  using type = short;
};
template <>
struct NTVec<1> {  // one pool window code (scalar path)
  using type = char;
};

template <typename T, int V>
__device__ __forceinline__ Pack<T, V> nt_load(const T* p) {
#ifdef MSBN_DISABLE_NT  // cached-access A/B build (tools/kernel_bench.py)
  return *reinterpret_cast<const Pack<T, V>*>(p);
#else
  using VT = typename NTVec<(int)sizeof(T) * V>::type;
  union {
    VT v;
    Pack<T, V> pk;
  } u;
  u.v = __builtin_nontemporal_load(reinterpret_cast<const VT*>(p));
  return u.pk;
#endif
}

template <typename T, int V>
__device__ __forceinline__ void nt_store(T* p, const Pack<T, V>& val) {
#ifdef MSBN_DISABLE_NT
  *reinterpret_cast<Pack<T, V>*>(p) = val;
#else
  using VT = typename NTVec<(int)sizeof(T) * V>::type;
  union {
    VT v;
    Pack<T, V> pk;
  } u;
  u.pk = val;
  __builtin_nontemporal_store(u.v, reinterpret_cast<VT*>(p));
#endif
}

template <typename T>
__device__ __forceinline__ T nt_load1(const T* p) {
  return nt_load<T, 1>(p).v[0];
}

template <typename T>
__device__ __forceinline__ void nt_store1(T* p, T val) {
  Pack<T, 1> pk;
  pk.v[0] = val;
  nt_store<T, 1>(p, pk);
}

// --------------------------------------------------------- wave64 reductions
__device__ __forceinline__ void wave_reduce_pair(double& a, double& b) {
#pragma unroll
  for (int off = MSBN_WAVE / 2; off > 0; off >>= 1) {
    a += __shfl_down(a, off, MSBN_WAVE);
    b += __shfl_down(b, off, MSBN_WAVE);
  }
}

// Block-level {sum, sumsq} reduction: wave64 shuffle tree, then LDS partials
// (one double2 per wave), wave 0 combines.  Result valid on thread 0 only.
// lds must hold 2 * (blockDim.x/64) doubles.
__device__ __forceinline__ void block_reduce_pair(double& a, double& b,
                                                  double* lds) {
  wave_reduce_pair(a, b);
  const int lane = threadIdx.x & (MSBN_WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int nw = blockDim.x >> 6;
  if (lane == 0) {
    lds[2 * wid] = a;
    lds[2 * wid + 1] = b;
  }
  __syncthreads();
  if (wid == 0) {
    a = (lane < nw) ? lds[2 * lane] : 0.0;
    b = (lane < nw) ? lds[2 * lane + 1] : 0.0;
    wave_reduce_pair(a, b);
  }
}

__device__ __forceinline__ int64_t i64min(int64_t a, int64_t b) {
  return a < b ? a : b;
}

// -------------------------------------------- chunked fp32->fp64 accumulator
// The streaming reduction loops are VALU-bound on MI355X when they
// accumulate every element in fp64 (f64 vector ops run at half rate: 16
// half-rate f64 ops per 16 B load caps the stats kernels at ~4.8 TB/s of
// the 6.3 TB/s ceiling).  Accumulate a short fp32 chunk (<= kAccFlush loop
// iterations) and FLUSH into the fp64 totals periodically: full-rate inner
// loop.
//
// What the fp64 totals do NOT do is protect {sum v, sum v*v} of raw values:
// each v*v and each chunk add is rounded in fp32 (relative 2^-24 of v^2), so
// var = E[x^2]-E[x]^2 loses mean^2/var of its digits before fp64 sees it
// (mean 1000, std 1: invstd off by 1e-3..1e-2).  Hence:
//   * the stats kernels sum raw values first — exact enough while
//     mean^2/var <= MSBN_RAW_COND_MAX, which is what activations look like —
//     and a block whose chunk fails that test (needs_recentre) reads the
//     chunk again, sums d = x - pivot with pivot = the chunk's mean, and
//     undoes the shift in fp64 (unshift_pair).  fp32 chunk error is then
//     ~sqrt(n)*2^-24 relative to sum d^2 ~ n*var, i.e. of the variance;
//   * the backward kernels add g and g*(x - mean) (add2), centred already.
// Either way the workspace holds plain fp64 {sum x, sum x^2}; the finalize
// kernels' E[x^2]-E[x]^2 then costs 2^-53 * mean^2/var, which is the
// conditioning of the problem in fp64.
#define MSBN_ACC_FLUSH 64

struct AccPair {
  double a = 0.0, b = 0.0;  // fp64 totals
  float fa = 0.f, fb = 0.f;  // fp32 chunk

  __device__ __forceinline__ void add(float v) {
    fa += v;
    fb += v * v;
  }
  __device__ __forceinline__ void add2(float s, float sq) {
    fa += s;
    fb += sq;
  }
  __device__ __forceinline__ void flush() {
    a += (double)fa;
    b += (double)fb;
    fa = fb = 0.f;
  }
};

// mean^2/var above which a chunk's raw {sum x, sum x^2} are not trusted and
// the stats kernels re-read the chunk with shifted values.  The raw sums'
// relative error in the variance is ~(1 + cond) * 2^-24; at 64 that is
// still several times inside the 1e-5 the statistics are held to.  The raw
// sums themselves decide: their variance is off by at most ~mean^2 * 1e-6,
// so an ill-conditioned chunk cannot look well-conditioned.
#define MSBN_RAW_COND_MAX 64.0

__device__ __forceinline__ bool needs_recentre(double sum, double sumsq,
                                               double cnt) {
  // mean^2 <= K*var with mean = sum/cnt, var = sumsq/cnt - mean^2, cleared
  // of its divisions: (K+1)*sum^2 <= K*cnt*sumsq.  False for var <= 0 (unless
  // all is zero) and for NaN: re-centre.
  return !((MSBN_RAW_COND_MAX + 1.0) * sum * sum <=
           MSBN_RAW_COND_MAX * cnt * sumsq);
}

// {sum d, sum d^2} over cnt elements with d = x - pivot  ->  {sum x, sum x^2}
__device__ __forceinline__ void unshift_pair(double& a, double& b,
                                             float pivot, double cnt) {
  const double p = (double)pivot;
  b += p * (2.0 * a + cnt * p);
  a += cnt * p;
}

}  // namespace msbn
