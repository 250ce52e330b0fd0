// Grouped (multi-tensor) training BatchNorm for MI355X (gfx950, CDNA4).
//
// One BatchNorm module applied to S tensors ("segments") that share C and
// dtype but not N*H*W -- the levels of a feature pyramid under a shared
// detection head -- each normalised with its OWN batch statistics.  Run one
// tensor at a time that is S statistics launches, S finalizes, S elementwise
// launches (and S all_gathers / all_reduces when synced), most of them far
// too small to fill 256 CUs.  Here every stage is ONE launch for the group:
//
//  * SegTable, a by-value kernel argument, holds per segment the base
//    pointers, the row count and two prefix sums: the first block of the
//    segment in the grid and its first chunk in the workspace.  A block finds
//    its segment by comparing its index with the at most 8 prefix entries
//    (wave-uniform, scalar registers): no per-segment launch, no table in
//    global memory.
//  * reductions: grid (channel tile, every segment's row chunks end to end).
//    The chunk height is chosen ONCE from the group's total row count, so a
//    large level gets proportionally many blocks and a tiny level is one
//    partial chunk.  Thread mapping, 16-byte nontemporal packs, fp32-chunked
//    fp64 accumulation and the re-centred second pass are those of
//    bn_stats_partial_nhwc / bn_bwd_reduce_partial_nhwc (bn_kernels.hip).
//    Workspace: fp64 {sum, sumsq}, [segment][channel][chunk of the segment],
//    i.e. segment s starts at first_chunk[s] * C pairs.
//  * finalize: one wave per channel walks the segments IN ORDER, so the
//    running statistics receive S successive momentum updates, each rounded
//    to fp32 as a module call would store it.
//  * elementwise: a 1-D grid, each segment owning a run of blocks sized by
//    its share of the packs, grid-stride inside the run.
//
// Deterministic: no atomics anywhere.  Channels-last only, full 16-byte
// packs only (C a multiple of V); the host declines the rest.
#include "bn_ops.hpp"
#include "common.hpp"
#include "launch_common.hpp"

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <climits>
#include <map>
#include <string>
#include <vector>

// Scalar fp32 arithmetic only in this file's device code (as in
// conv_stats_kernels.hip): the per-element loops over a pack are what the
// vectorizer turns into packed fp32 instructions.  Functions from outside
// the attribute inline only when they are always_inline (common.hpp's
// helpers are); the runtime header's barriers and AccPair's implicit
// constructor are not and would be CALLED (a stack frame, i.e. scratch), so
// the block barrier is spelled out below and AccPair is aggregate-initialised.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace msbn {

namespace {

constexpr int kMaxSeg = 8;

__device__ __forceinline__ void gbn_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct SegTable {
  const void* x[kMaxSeg];    // input of the segment
  const void* dy[kMaxSeg];   // incoming gradient (backward kernels)
  void* out[kMaxSeg];        // y (forward) or dx (backward)
  int64_t rows[kMaxSeg];     // N*H*W of the segment
  int first_block[kMaxSeg + 1];  // prefix sum over the grid
  int first_chunk[kMaxSeg + 1];  // prefix sum over the workspace chunks
  int nseg;
};

// The segment that owns grid block `block`: the number of prefix entries at
// or below it.  An empty segment shares its entry with its successor and is
// stepped over.  Uniform across the block.
__device__ __forceinline__ int find_segment(const SegTable& t, int block) {
  int s = 0;
#pragma unroll
  for (int i = 1; i < kMaxSeg; ++i)
    s += (i < t.nseg && block >= t.first_block[i]) ? 1 : 0;
  return s;
}

// LDS tree over the thread rows of a block (bn_stats_partial_nhwc's): the
// totals of column `lane` end up in the slots of thread `lane` (rowoff 0).
// Layout [k][tid], separate sum / sumsq planes: bank-conflict free.
template <int V>
__device__ __forceinline__ void reduce_thread_rows(double* sdata,
                                                   const double* a,
                                                   const double* b, int lpr,
                                                   int rpi, int rowoff) {
#pragma unroll
  for (int k = 0; k < V; ++k) {
    sdata[k * MSBN_BLOCK + threadIdx.x] = a[k];
    sdata[(V + k) * MSBN_BLOCK + threadIdx.x] = b[k];
  }
  for (int st = 1; st < rpi; st <<= 1) {
    gbn_sync();
    if ((rowoff & ((st << 1) - 1)) == 0 && rowoff + st < rpi) {
      const int other = threadIdx.x + st * lpr;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        sdata[k * MSBN_BLOCK + threadIdx.x] += sdata[k * MSBN_BLOCK + other];
        sdata[(V + k) * MSBN_BLOCK + threadIdx.x] +=
            sdata[(V + k) * MSBN_BLOCK + other];
      }
    }
  }
  gbn_sync();
}

// =====================================================================
// grouped statistics partial: grid(ctiles, total chunks) block 256
// lpr divides 256, so every thread row is whole (rpi * lpr == 256).
// =====================================================================
template <typename T, int V>
__global__ void gbn_stats_partial(SegTable tab, double* __restrict__ ws,
                                  int64_t C, int64_t chunk_rows, int lpr) {
  const int s = find_segment(tab, blockIdx.y);
  const int chunk = blockIdx.y - tab.first_block[s];
  const int nch = tab.first_block[s + 1] - tab.first_block[s];
  const T* __restrict__ x = static_cast<const T*>(tab.x[s]);
  const int64_t rows = tab.rows[s];
  double* wseg = ws + (int64_t)tab.first_chunk[s] * C * 2;

  const int rpi = blockDim.x / lpr;  // rows in flight per iteration
  const int lane = threadIdx.x % lpr;
  const int rowoff = threadIdx.x / lpr;
  const int64_t c = (int64_t)blockIdx.x * lpr * V + (int64_t)lane * V;
  const bool inb = c + V <= C;
  const int64_t r0 = (int64_t)chunk * chunk_rows;
  const int64_t r1 = i64min(r0 + chunk_rows, rows);

  __shared__ double sdata[MSBN_BLOCK * V * 2];
  __shared__ int recentre_any;  // some channel of the block wants pass 2
  if (threadIdx.x == 0) recentre_any = 0;  // barriers follow before its use

  float pivot[V];
  bool re[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    pivot[k] = 0.f;
    re[k] = false;
  }

  for (int pass = 0; pass < 2; ++pass) {
    AccPair acc[V] = {};
    if (inb) {
      int since_flush = 0;
      for (int64_t r = r0 + rowoff; r < r1; r += rpi) {
        Pack<T, V> pk = nt_load<T, V>(&x[r * C + c]);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k].add(to_f(pk.v[k]) - pivot[k]);
        if (++since_flush == MSBN_ACC_FLUSH) {
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k].flush();
          since_flush = 0;
        }
      }
    }
    double a[V], b[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      acc[k].flush();
      a[k] = acc[k].a;
      b[k] = acc[k].b;
    }
    // second pass: undo the shift per thread, over the rows it summed
    if (pass && inb && r0 + rowoff < r1) {
      const double cnt = (double)((r1 - r0 - rowoff + rpi - 1) / rpi);
#pragma unroll
      for (int k = 0; k < V; ++k) unshift_pair(a[k], b[k], pivot[k], cnt);
    }
    if (pass) gbn_sync();  // sdata is reused
    reduce_thread_rows<V>(sdata, a, b, lpr, rpi, rowoff);

    int any = 0;
    if (rowoff == 0 && inb) {
      const double cnt = (double)(r1 - r0);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const double sa = sdata[k * MSBN_BLOCK + threadIdx.x];
        const double sb = sdata[(V + k) * MSBN_BLOCK + threadIdx.x];
        bool want = false;
        if (!pass) {
          want = needs_recentre(sa, sb, cnt);
          // publish {recentre?, pivot} in this thread's own slots
          // (threadIdx.x == lane here); read back after the barrier below
          sdata[k * MSBN_BLOCK + threadIdx.x] = want ? 1.0 : 0.0;
          sdata[(V + k) * MSBN_BLOCK + threadIdx.x] = want ? sa / cnt : 0.0;
          any |= want ? 1 : 0;
        }
        // first pass: the channels that are fine as they are; second pass:
        // the re-centred ones
        if (pass ? re[k] : !want) {
          double* out = wseg + ((c + k) * nch + chunk) * 2;
          out[0] = sa;
          out[1] = sb;
        }
      }
    }
    if (pass) break;
    if (any) recentre_any = 1;
    gbn_sync();  // publishes sdata and the flag
    if (!recentre_any) break;  // block-uniform
    if (inb) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        re[k] = sdata[k * MSBN_BLOCK + lane] != 0.0;
        pivot[k] = re[k] ? (float)sdata[(V + k) * MSBN_BLOCK + lane] : 0.f;
      }
    }
  }
}

// =====================================================================
// grouped statistics finalize: one wave per channel, segments in order.
// Local form: mean / invstd [S, C] (stat_stride = C), count [S]
// (count_stride = 1), the running update and coefs [S, 2C].  Packed form:
// the three pointers aim into out[S][2C+1] (both strides 2C+1) and the
// running statistics / coefs are null.
// =====================================================================
__global__ void gbn_stats_finalize(SegTable tab, const double* __restrict__ ws,
                                   int64_t C, float eps,
                                   float* __restrict__ mean,
                                   float* __restrict__ invstd,
                                   int64_t stat_stride,
                                   float* __restrict__ count_out,
                                   int64_t count_stride,
                                   float* __restrict__ rmean,
                                   float* __restrict__ rvar, float momentum,
                                   const float* __restrict__ w,
                                   const float* __restrict__ bws,
                                   float* __restrict__ coefs) {
  const int lane = threadIdx.x & (MSBN_WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + wid;
  if (c >= C) return;  // whole waves only
  float rm = 0.f, rv = 0.f;
  if (rmean != nullptr && lane == 0) {
    rm = rmean[c];
    rv = rvar[c];
  }
  for (int s = 0; s < tab.nseg; ++s) {
    const int nch = tab.first_block[s + 1] - tab.first_block[s];
    const double* wseg =
        ws + ((int64_t)tab.first_chunk[s] * C + c * (int64_t)nch) * 2;
    double a = 0.0, b = 0.0;
    for (int ch = lane; ch < nch; ch += MSBN_WAVE) {
      a += wseg[ch * 2];
      b += wseg[ch * 2 + 1];
    }
    wave_reduce_pair(a, b);
    if (lane != 0) continue;
    const double count = (double)tab.rows[s];
    float m = 0.f, istd = 0.f;
    if (count > 0.0) {
      const double md = a / count;
      double var = b / count - md * md;
      var = var > 0.0 ? var : 0.0;
      m = (float)md;
      istd = (float)rsqrt(var + (double)eps);
      if (rmean != nullptr) {
        const double unbiased =
            count > 1.0 ? var * (count / (count - 1.0)) : var;
        rm = (1.f - momentum) * rm + momentum * m;
        rv = (1.f - momentum) * rv + momentum * (float)unbiased;
      }
    }
    mean[s * stat_stride + c] = m;
    invstd[s * stat_stride + c] = istd;
    if (c == 0) count_out[s * count_stride] = (float)count;
    if (coefs != nullptr) {
      const float sc = istd * (w != nullptr ? w[c] : 1.f);
      coefs[s * 2 * C + c] = sc;
      coefs[s * 2 * C + C + c] = -m * sc + (bws != nullptr ? bws[c] : 0.f);
    }
  }
  if (rmean != nullptr && lane == 0) {
    rmean[c] = rm;
    rvar[c] = rv;
  }
}

// =====================================================================
// grouped gather: packed_all[W][S][2C+1] -> per segment the count-weighted
// combine of bn_gather_stats (zero-count ranks masked here), the running
// update in segment order, the coefs.  One thread per channel.
// =====================================================================
__global__ void gbn_gather_stats(const float* __restrict__ packed_all, int W,
                                 int S, int64_t C, float eps, float momentum,
                                 float* __restrict__ mean,
                                 float* __restrict__ invstd,
                                 float* __restrict__ count_out,
                                 float* __restrict__ rmean,
                                 float* __restrict__ rvar,
                                 const float* __restrict__ wpar,
                                 const float* __restrict__ bpar,
                                 float* __restrict__ coefs) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const int64_t row = 2 * C + 1;
  float rm = 0.f, rv = 0.f;
  if (rmean != nullptr) {
    rm = rmean[c];
    rv = rvar[c];
  }
  for (int s = 0; s < S; ++s) {
    double n_tot = 0.0, m_acc = 0.0, ex2 = 0.0;
    for (int w = 0; w < W; ++w) {
      const float* p = packed_all + ((int64_t)w * S + s) * row;
      const float cnt = p[2 * C];
      if (cnt > 0.f) {
        const double m = p[c];
        const double istd = p[C + c];
        const double var = 1.0 / (istd * istd) - (double)eps;
        n_tot += cnt;
        m_acc += cnt * m;
        ex2 += cnt * (var + m * m);
      }
    }
    float m_out = 0.f, istd_out = 0.f;
    if (n_tot > 0.0) {
      const double m_g = m_acc / n_tot;
      double var_g = ex2 / n_tot - m_g * m_g;
      var_g = var_g > 0.0 ? var_g : 0.0;
      m_out = (float)m_g;
      istd_out = (float)rsqrt(var_g + (double)eps);
      if (rmean != nullptr) {
        const double unbiased =
            n_tot > 1.0 ? var_g * (n_tot / (n_tot - 1.0)) : var_g;
        rm = (1.f - momentum) * rm + momentum * m_out;
        rv = (1.f - momentum) * rv + momentum * (float)unbiased;
      }
    }
    mean[s * C + c] = m_out;
    invstd[s * C + c] = istd_out;
    if (c == 0) count_out[s] = (float)n_tot;
    const float sc = istd_out * (wpar != nullptr ? wpar[c] : 1.f);
    coefs[s * 2 * C + c] = sc;
    coefs[s * 2 * C + C + c] =
        -m_out * sc + (bpar != nullptr ? bpar[c] : 0.f);
  }
  if (rmean != nullptr) {
    rmean[c] = rm;
    rvar[c] = rv;
  }
}

// =====================================================================
// grouped elementwise forward: y_s = act(x_s * scale_s + shift_s)
// 1-D grid; segment s owns blocks [first_block[s], first_block[s+1]) and
// walks its packs grid-stride inside that run.
// =====================================================================
template <typename T, int V, int ACT>
__global__ void gbn_elemt(SegTable tab, const float* __restrict__ coefs,
                          int64_t C) {
  const int s = find_segment(tab, blockIdx.x);
  const int nb = tab.first_block[s + 1] - tab.first_block[s];
  const T* __restrict__ x = static_cast<const T*>(tab.x[s]);
  T* __restrict__ y = static_cast<T*>(tab.out[s]);
  const float* __restrict__ scale = coefs + (int64_t)s * 2 * C;
  const float* __restrict__ shift = scale + C;
  const int64_t packs = tab.rows[s] * C / V;
  const int64_t stride = (int64_t)nb * blockDim.x;
  for (int64_t i = (int64_t)(blockIdx.x - tab.first_block[s]) * blockDim.x +
                   threadIdx.x;
       i < packs; i += stride) {
    const int64_t e = i * V;
    const int64_t c = e % C;
    Pack<T, V> px = nt_load<T, V>(&x[e]);
    Pack<float, V> ps = *reinterpret_cast<const Pack<float, V>*>(&scale[c]);
    Pack<float, V> pb = *reinterpret_cast<const Pack<float, V>*>(&shift[c]);
    Pack<T, V> py;
#pragma unroll
    for (int k = 0; k < V; ++k)
      py.v[k] = from_f<T>(
          act_fwd<ACT>(to_f(px.v[k]) * ps.v[k] + pb.v[k], 0.f));
    nt_store<T, V>(&y[e], py);
  }
}

// =====================================================================
// grouped backward reduce partial: per (segment, channel, chunk)
// {sum g, sum g*(x - mean_s)}, g = dy through the ReLU gate recomputed from
// z = scale_s * x + shift_s.  Grid and workspace of gbn_stats_partial.
// =====================================================================
template <typename T, int V, int ACT>
__global__ void gbn_bwd_reduce_partial(SegTable tab,
                                       const float* __restrict__ mean,
                                       const float* __restrict__ coefs,
                                       double* __restrict__ ws, int64_t C,
                                       int64_t chunk_rows, int lpr) {
  const int s = find_segment(tab, blockIdx.y);
  const int chunk = blockIdx.y - tab.first_block[s];
  const int nch = tab.first_block[s + 1] - tab.first_block[s];
  const T* __restrict__ x = static_cast<const T*>(tab.x[s]);
  const T* __restrict__ dy = static_cast<const T*>(tab.dy[s]);
  const int64_t rows = tab.rows[s];
  double* wseg = ws + (int64_t)tab.first_chunk[s] * C * 2;

  const int rpi = blockDim.x / lpr;
  const int lane = threadIdx.x % lpr;
  const int rowoff = threadIdx.x / lpr;
  const int64_t c = (int64_t)blockIdx.x * lpr * V + (int64_t)lane * V;
  const bool inb = c + V <= C;

  AccPair acc[V] = {};
  if (inb) {
    float m[V], scv[V], shv[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      m[k] = mean[(int64_t)s * C + c + k];
      scv[k] = ACT ? coefs[(int64_t)s * 2 * C + c + k] : 0.f;
      shv[k] = ACT ? coefs[(int64_t)s * 2 * C + C + c + k] : 0.f;
    }
    const int64_t r0 = (int64_t)chunk * chunk_rows;
    const int64_t r1 = i64min(r0 + chunk_rows, rows);
    int since_flush = 0;
    for (int64_t r = r0 + rowoff; r < r1; r += rpi) {
      Pack<T, V> pg = nt_load<T, V>(&dy[r * C + c]);
      Pack<T, V> px = nt_load<T, V>(&x[r * C + c]);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float g = to_f(pg.v[k]);
        const float xv = to_f(px.v[k]);
        if (ACT) g = act_gate<ACT>(scv[k] * xv + shv[k], g, 0.f);
        acc[k].add2(g, g * (xv - m[k]));
      }
      if (++since_flush == MSBN_ACC_FLUSH) {
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k].flush();
        since_flush = 0;
      }
    }
  }
  double a[V], b[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    acc[k].flush();
    a[k] = acc[k].a;
    b[k] = acc[k].b;
  }
  __shared__ double sdata[MSBN_BLOCK * V * 2];
  reduce_thread_rows<V>(sdata, a, b, lpr, rpi, rowoff);
  if (rowoff == 0 && inb) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      double* out = wseg + ((c + k) * nch + chunk) * 2;
      out[0] = sdata[k * MSBN_BLOCK + threadIdx.x];
      out[1] = sdata[(V + k) * MSBN_BLOCK + threadIdx.x];
    }
  }
}

// one wave per channel; sums[S][2C] = per segment [sum_dy | sum_dy_xmu],
// grad_weight / grad_bias accumulated over the segments in ascending order,
// each segment's term rounded to fp32 first (what S calls would hand
// autograd to add up).
__global__ void gbn_bwd_reduce_finalize(SegTable tab,
                                        const double* __restrict__ ws,
                                        int64_t C,
                                        const float* __restrict__ invstd,
                                        float* __restrict__ sums,
                                        float* __restrict__ grad_weight,
                                        float* __restrict__ grad_bias) {
  const int lane = threadIdx.x & (MSBN_WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + wid;
  if (c >= C) return;  // whole waves only
  float gw = 0.f, gb = 0.f;
  for (int s = 0; s < tab.nseg; ++s) {
    const int nch = tab.first_block[s + 1] - tab.first_block[s];
    const double* wseg =
        ws + ((int64_t)tab.first_chunk[s] * C + c * (int64_t)nch) * 2;
    double a = 0.0, b = 0.0;
    for (int ch = lane; ch < nch; ch += MSBN_WAVE) {
      a += wseg[ch * 2];
      b += wseg[ch * 2 + 1];
    }
    wave_reduce_pair(a, b);
    if (lane != 0) continue;
    sums[(int64_t)s * 2 * C + c] = (float)a;
    sums[(int64_t)s * 2 * C + C + c] = (float)b;
    gw += (float)(b * invstd[(int64_t)s * C + c]);
    gb += (float)a;
  }
  if (lane != 0) return;
  if (grad_weight != nullptr) grad_weight[c] = gw;
  if (grad_bias != nullptr) grad_bias[c] = gb;
}

// =====================================================================
// grouped backward elementwise: dx_s = a*g + b*x + d with, per (segment,
// channel), n = count[s] and
//   f1 = invstd*gamma, f2 = sum_dy/n, f3 = invstd^2*sum_dy_xmu/n
//   a = f1, b = -f1*f3, d = f1*(f3*mean - f2)
// (bn_affine_bwd's expressions) formed in the kernel from the per-channel
// vectors, which stay in cache: no coefficient launch of its own.  A segment
// whose total count is zero has no rows on any rank.
// =====================================================================
template <typename T, int V, int ACT>
__global__ void gbn_bwd_elemt(SegTable tab, const float* __restrict__ mean,
                              const float* __restrict__ invstd,
                              const float* __restrict__ coefs,
                              const float* __restrict__ sums,
                              const float* __restrict__ count, int64_t C) {
  const int s = find_segment(tab, blockIdx.x);
  const int nb = tab.first_block[s + 1] - tab.first_block[s];
  const T* __restrict__ x = static_cast<const T*>(tab.x[s]);
  const T* __restrict__ dy = static_cast<const T*>(tab.dy[s]);
  T* __restrict__ dx = static_cast<T*>(tab.out[s]);
  const float* __restrict__ ms = mean + (int64_t)s * C;
  const float* __restrict__ is = invstd + (int64_t)s * C;
  const float* __restrict__ scale = coefs + (int64_t)s * 2 * C;
  const float* __restrict__ shift = scale + C;
  const float* __restrict__ sdy = sums + (int64_t)s * 2 * C;
  const float* __restrict__ sdx = sdy + C;
  const float n = count[s];
  const int64_t packs = tab.rows[s] * C / V;
  const int64_t stride = (int64_t)nb * blockDim.x;
  using PF = Pack<float, V>;
  for (int64_t i = (int64_t)(blockIdx.x - tab.first_block[s]) * blockDim.x +
                   threadIdx.x;
       i < packs; i += stride) {
    const int64_t e = i * V;
    const int64_t c = e % C;
    Pack<T, V> pg = nt_load<T, V>(&dy[e]);
    Pack<T, V> px = nt_load<T, V>(&x[e]);
    const PF pm = *reinterpret_cast<const PF*>(&ms[c]);
    const PF pi = *reinterpret_cast<const PF*>(&is[c]);
    const PF p1 = *reinterpret_cast<const PF*>(&sdy[c]);
    const PF p2 = *reinterpret_cast<const PF*>(&sdx[c]);
    // scale_s is invstd_s * gamma, the f1 of the formula, bit for bit
    const PF psc = *reinterpret_cast<const PF*>(&scale[c]);
    PF psh;
    if (ACT) psh = *reinterpret_cast<const PF*>(&shift[c]);
    Pack<T, V> po;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float g = to_f(pg.v[k]);
      const float xv = to_f(px.v[k]);
      if (ACT) g = act_gate<ACT>(psc.v[k] * xv + psh.v[k], g, 0.f);
      const float istd = pi.v[k];
      const float f1 = psc.v[k];
      const float f2 = p1.v[k] / n;
      const float f3 = istd * istd * p2.v[k] / n;
      po.v[k] = from_f<T>(f1 * g + (-f1 * f3) * xv +
                          f1 * (f3 * pm.v[k] - f2));
    }
    nt_store<T, V>(&dx[e], po);
  }
}

// =====================================================================
// host side
// =====================================================================

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// most blocks of a grouped elementwise launch, before the at most one extra
// block per segment that rounding up adds (elemt_grid's cap in bn_kernels)
constexpr int kElemtBlockCap = 2 * kTargetBlocks;

// The one place a grouped launch is decided; launch_plan_grouped reports it.
struct GroupPlan {
  bool ok = false;
  int S = 0;
  int64_t C = 0;
  int v = 0;
  at::ScalarType dtype = at::kFloat;
  int64_t rows[kMaxSeg] = {};
  int64_t total_rows = 0;
  // reductions
  int lpr = 0, ctiles = 0;
  int64_t chunk_rows = 0;
  int nchunks[kMaxSeg] = {};
  int first_chunk[kMaxSeg + 1] = {};
  int64_t red_trips = 0;
  // elementwise
  int eblocks[kMaxSeg] = {};
  int first_eblock[kMaxSeg + 1] = {};
  int64_t packs = 0;
  int64_t elemt_trips = 0;
};

bool pack_type(at::ScalarType t) {
  return t == at::kFloat || t == at::kBFloat16 || t == at::kHalf;
}

// `lists`: the tensor lists the kernels read with 16-byte packs (inputs,
// then gradients); every list has S entries shaped like lists[0].  The
// device is not looked at (the plan of a CPU tensor is that of its GPU copy).
GroupPlan plan_group(const std::vector<const std::vector<at::Tensor>*>& lists) {
  GroupPlan p;
  const auto& xs = *lists[0];
  const int64_t S = (int64_t)xs.size();
  if (S < 1 || S > kMaxSeg) return p;
  const at::Tensor& x0 = xs[0];
  if (x0.dim() != 4 || !pack_type(x0.scalar_type())) return p;
  const int64_t C = x0.size(1);
  const int v = 16 / (int)x0.element_size();
  if (C <= 0 || C % v != 0) return p;
  for (const auto* l : lists) {
    if ((int64_t)l->size() != S) return p;
    for (int64_t s = 0; s < S; ++s) {
      const at::Tensor& t = (*l)[s];
      if (!t.defined() || t.dim() != 4 || t.sizes() != xs[s].sizes() ||
          t.size(1) != C || t.scalar_type() != x0.scalar_type() ||
          t.device() != x0.device())
        return p;
      if (t.numel() == 0) continue;
      if (!t.is_contiguous(at::MemoryFormat::ChannelsLast) ||
          ((uintptr_t)t.data_ptr() % 16) != 0)
        return p;
    }
  }
  p.S = (int)S;
  p.C = C;
  p.v = v;
  p.dtype = x0.scalar_type();
  for (int s = 0; s < p.S; ++s) {
    p.rows[s] = xs[s].numel() / C;
    p.total_rows += p.rows[s];
  }
  // reductions: bn_kernels' channel tiling; ONE chunk height for the group,
  // from its total rows (nhwc_grid's rule applied to the concatenation)
  p.lpr = nhwc_lanes_per_row(C, v);
  p.ctiles = (int)cdiv(C, (int64_t)p.lpr * v);
  const int rpi = MSBN_BLOCK / p.lpr;
  const int64_t per_tile =
      std::max<int64_t>(1, kTargetBlocks / std::max(p.ctiles, 1));
  const int64_t max_chunks =
      cdiv(p.total_rows, std::max<int64_t>(4 * rpi, 16));
  const int64_t want =
      std::max<int64_t>(1, std::min(per_tile, std::max<int64_t>(max_chunks, 1)));
  p.chunk_rows = std::max<int64_t>(1, cdiv(p.total_rows, want));
  int64_t longest = 0;
  for (int s = 0; s < p.S; ++s) {
    const int64_t n = cdiv(p.rows[s], p.chunk_rows);
    if (n > INT_MAX / 2 || p.first_chunk[s] + n > INT_MAX / 2) return p;
    p.nchunks[s] = (int)n;
    p.first_chunk[s + 1] = p.first_chunk[s] + (int)n;
    longest = std::max(longest, std::min(p.rows[s], p.chunk_rows));
  }
  p.red_trips = cdiv(longest, rpi);
  // elementwise: blocks in proportion to the packs; past the cap every
  // thread takes the same number of extra trips
  int64_t full = 0;
  int64_t pblocks[kMaxSeg];
  for (int s = 0; s < p.S; ++s) {
    pblocks[s] = cdiv(p.rows[s] * C / v, MSBN_BLOCK);
    full += pblocks[s];
    p.packs += p.rows[s] * C / v;
  }
  const int64_t share = std::max<int64_t>(1, cdiv(full, kElemtBlockCap));
  for (int s = 0; s < p.S; ++s) {
    p.eblocks[s] = (int)cdiv(pblocks[s], share);
    p.first_eblock[s + 1] = p.first_eblock[s] + p.eblocks[s];
    if (p.eblocks[s] > 0)
      p.elemt_trips = std::max(
          p.elemt_trips,
          cdiv(p.rows[s] * C / v, (int64_t)p.eblocks[s] * MSBN_BLOCK));
  }
  p.ok = true;
  return p;
}

// the table of a launch: pointers from the lists, prefix sums from the plan
SegTable make_table(const GroupPlan& p, const std::vector<at::Tensor>& xs,
                    const std::vector<at::Tensor>* dys,
                    const std::vector<at::Tensor>* outs, bool elemt) {
  SegTable t{};
  t.nseg = p.S;
  for (int s = 0; s < p.S; ++s) {
    t.x[s] = xs[s].data_ptr();
    t.dy[s] = dys ? (*dys)[s].data_ptr() : nullptr;
    t.out[s] = outs ? (*outs)[s].data_ptr() : nullptr;
    t.rows[s] = p.rows[s];
  }
  for (int s = 0; s <= p.S; ++s) {
    t.first_block[s] = elemt ? p.first_eblock[s] : p.first_chunk[s];
    t.first_chunk[s] = p.first_chunk[s];
  }
  return t;
}

template <typename T, int V>
struct TV {
  using type = T;
  static constexpr int v = V;
};

template <typename F>
void dispatch_pack(at::ScalarType t, F&& f) {
  switch (t) {
    case at::kFloat:
      return f(TV<float, 4>{});
    case at::kBFloat16:
      return f(TV<__hip_bfloat16, 8>{});
    default:
      return f(TV<__half, 8>{});
  }
}

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

GroupPlan checked_plan(const std::vector<at::Tensor>& xs,
                       const std::vector<at::Tensor>* dys, const char* op) {
  std::vector<const std::vector<at::Tensor>*> lists{&xs};
  if (dys) lists.push_back(dys);
  const GroupPlan p = plan_group(lists);
  TORCH_CHECK(p.ok && xs[0].is_cuda(), op,
              ": takes 1..8 dense channels-last 4-D GPU tensors of one dtype "
              "and C, C a multiple of the 16-byte pack, 16-byte aligned "
              "(ask launch_plan first)");
  return p;
}

// fp32 [C] on the inputs' device, or absent
const float* vec_ptr(const c10::optional<at::Tensor>& t, int64_t C,
                     const at::Tensor& like, const char* op) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous() &&
                  t->numel() == C && t->device() == like.device(),
              op, ": weight / bias / running statistics must be contiguous "
                  "fp32 [C] on the inputs' device");
  return t->data_ptr<float>();
}

void check_f32(const at::Tensor& t, int64_t numel, const at::Tensor& like,
               const char* what) {
  TORCH_CHECK(t.defined() && t.scalar_type() == at::kFloat &&
                  t.is_contiguous() && t.numel() == numel &&
                  t.device() == like.device(),
              what, " must be contiguous fp32 of ", numel, " elements on the "
              "inputs' device");
}

// partial launch into a fresh workspace; an all-empty group launches nothing
at::Tensor stats_partials_grouped(const GroupPlan& p,
                                  const std::vector<at::Tensor>& xs) {
  const int total = p.first_chunk[p.S];
  at::Tensor ws = at::empty({(int64_t)std::max(total, 1) * p.C * 2},
                            xs[0].options().dtype(at::kDouble));
  if (total == 0) return ws;
  const SegTable tab = make_table(p, xs, nullptr, nullptr, false);
  dispatch_pack(p.dtype, [&](auto tv) {
    using T = typename decltype(tv)::type;
    constexpr int V = decltype(tv)::v;
    hipLaunchKernelGGL((gbn_stats_partial<T, V>),
                       dim3((unsigned)p.ctiles, (unsigned)total),
                       dim3(MSBN_BLOCK), 0, cur_stream(), tab,
                       ws.data_ptr<double>(), p.C, p.chunk_rows, p.lpr);
  });
  return ws;
}

constexpr int kWavesPerBlock = MSBN_BLOCK / MSBN_WAVE;

std::vector<at::Tensor> alloc_like_group(const GroupPlan& p,
                                         const std::vector<at::Tensor>& xs) {
  // one allocation; every segment's bytes are a multiple of 16
  at::Tensor flat = at::empty({p.total_rows * p.C}, xs[0].options());
  std::vector<at::Tensor> outs;
  int64_t off = 0;
  for (int s = 0; s < p.S; ++s) {
    const auto sz = xs[s].sizes();
    outs.push_back(flat.narrow(0, off, p.rows[s] * p.C)
                       .view({sz[0], sz[2], sz[3], sz[1]})
                       .permute({0, 3, 1, 2}));
    off += p.rows[s] * p.C;
  }
  return outs;
}

}  // namespace

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_stats_local_grouped(const std::vector<at::Tensor>& inputs,
                               double eps,
                               const c10::optional<at::Tensor>& running_mean,
                               const c10::optional<at::Tensor>& running_var,
                               double momentum,
                               const c10::optional<at::Tensor>& weight,
                               const c10::optional<at::Tensor>& bias) {
  const char* op = "batch_norm_stats_local_grouped";
  const GroupPlan p = checked_plan(inputs, nullptr, op);
  const at::Tensor& x0 = inputs[0];
  float* rm = const_cast<float*>(vec_ptr(running_mean, p.C, x0, op));
  float* rv = const_cast<float*>(vec_ptr(running_var, p.C, x0, op));
  TORCH_CHECK((rm == nullptr) == (rv == nullptr), op,
              ": running_mean and running_var come together");
  const float* w = vec_ptr(weight, p.C, x0, op);
  const float* b = vec_ptr(bias, p.C, x0, op);
  auto f32 = x0.options().dtype(at::kFloat);
  auto mean = at::empty({p.S, p.C}, f32);
  auto invstd = at::empty({p.S, p.C}, f32);
  auto count = at::empty({p.S}, f32);
  auto coefs = at::empty({p.S, 2 * p.C}, f32);
  const at::Tensor ws = stats_partials_grouped(p, inputs);
  const SegTable tab = make_table(p, inputs, nullptr, nullptr, false);
  hipLaunchKernelGGL(gbn_stats_finalize,
                     dim3((unsigned)cdiv(p.C, kWavesPerBlock)),
                     dim3(MSBN_BLOCK), 0, cur_stream(), tab,
                     ws.data_ptr<double>(), p.C, (float)eps,
                     mean.data_ptr<float>(), invstd.data_ptr<float>(), p.C,
                     count.data_ptr<float>(), (int64_t)1, rm, rv,
                     (float)momentum, w, b, coefs.data_ptr<float>());
  return {mean, invstd, count, coefs};
}

void batch_norm_stats_packed_grouped(const std::vector<at::Tensor>& inputs,
                                     double eps, at::Tensor& out) {
  const char* op = "batch_norm_stats_packed_grouped";
  const GroupPlan p = checked_plan(inputs, nullptr, op);
  const int64_t row = 2 * p.C + 1;
  check_f32(out, p.S * row, inputs[0], "packed stats buffer [S, 2C+1]");
  if (p.total_rows == 0) {  // the join() shadow step: nothing to read
    out.zero_();
    return;
  }
  const at::Tensor ws = stats_partials_grouped(p, inputs);
  const SegTable tab = make_table(p, inputs, nullptr, nullptr, false);
  float* o = out.data_ptr<float>();
  hipLaunchKernelGGL(gbn_stats_finalize,
                     dim3((unsigned)cdiv(p.C, kWavesPerBlock)),
                     dim3(MSBN_BLOCK), 0, cur_stream(), tab,
                     ws.data_ptr<double>(), p.C, (float)eps, o, o + p.C, row,
                     o + 2 * p.C, row, (float*)nullptr, (float*)nullptr, 0.f,
                     (const float*)nullptr, (const float*)nullptr,
                     (float*)nullptr);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_gather_stats_packed_grouped(
    const at::Tensor& packed_all, const c10::optional<at::Tensor>& running_mean,
    const c10::optional<at::Tensor>& running_var, double momentum, double eps,
    const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias) {
  const char* op = "batch_norm_gather_stats_packed_grouped";
  TORCH_CHECK(packed_all.dim() == 3 && packed_all.is_contiguous() &&
                  packed_all.scalar_type() == at::kFloat &&
                  packed_all.is_cuda() && packed_all.size(1) >= 1 &&
                  packed_all.size(1) <= kMaxSeg && packed_all.size(2) >= 3 &&
                  packed_all.size(2) % 2 == 1 && packed_all.size(0) >= 1,
              op, ": packed_all must be contiguous fp32 [W, S <= 8, 2C+1] on "
                  "the GPU");
  const int W = (int)packed_all.size(0);
  const int S = (int)packed_all.size(1);
  const int64_t C = (packed_all.size(2) - 1) / 2;
  float* rm = const_cast<float*>(vec_ptr(running_mean, C, packed_all, op));
  float* rv = const_cast<float*>(vec_ptr(running_var, C, packed_all, op));
  TORCH_CHECK((rm == nullptr) == (rv == nullptr), op,
              ": running_mean and running_var come together");
  const float* w = vec_ptr(weight, C, packed_all, op);
  const float* b = vec_ptr(bias, C, packed_all, op);
  auto f32 = packed_all.options();
  auto mean = at::empty({S, C}, f32);
  auto invstd = at::empty({S, C}, f32);
  auto count = at::empty({S}, f32);
  auto coefs = at::empty({S, 2 * C}, f32);
  hipLaunchKernelGGL(gbn_gather_stats, dim3((unsigned)cdiv(C, MSBN_BLOCK)),
                     dim3(MSBN_BLOCK), 0, cur_stream(),
                     packed_all.data_ptr<float>(), W, S, C, (float)eps,
                     (float)momentum, mean.data_ptr<float>(),
                     invstd.data_ptr<float>(), count.data_ptr<float>(), rm, rv,
                     w, b, coefs.data_ptr<float>());
  return {mean, invstd, count, coefs};
}

std::vector<at::Tensor> batch_norm_elemt_act_grouped(
    const std::vector<at::Tensor>& inputs, const at::Tensor& coefs,
    bool relu) {
  const GroupPlan p =
      checked_plan(inputs, nullptr, "batch_norm_elemt_act_grouped");
  check_f32(coefs, p.S * 2 * p.C, inputs[0], "coefs [S, 2C]");
  std::vector<at::Tensor> ys = alloc_like_group(p, inputs);
  const int grid = p.first_eblock[p.S];
  if (grid == 0) return ys;
  const SegTable tab = make_table(p, inputs, nullptr, &ys, true);
  dispatch_pack(p.dtype, [&](auto tv) {
    using T = typename decltype(tv)::type;
    constexpr int V = decltype(tv)::v;
    if (relu)
      hipLaunchKernelGGL((gbn_elemt<T, V, kActRelu>), dim3((unsigned)grid),
                         dim3(MSBN_BLOCK), 0, cur_stream(), tab,
                         coefs.data_ptr<float>(), p.C);
    else
      hipLaunchKernelGGL((gbn_elemt<T, V, kActNone>), dim3((unsigned)grid),
                         dim3(MSBN_BLOCK), 0, cur_stream(), tab,
                         coefs.data_ptr<float>(), p.C);
  });
  return ys;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor>
batch_norm_backward_reduce_act_grouped(
    const std::vector<at::Tensor>& grad_outs,
    const std::vector<at::Tensor>& inputs, const at::Tensor& mean,
    const at::Tensor& invstd, const at::Tensor& coefs, bool relu,
    bool weight_g, bool bias_g) {
  const GroupPlan p = checked_plan(inputs, &grad_outs,
                                   "batch_norm_backward_reduce_act_grouped");
  const at::Tensor& x0 = inputs[0];
  check_f32(mean, p.S * p.C, x0, "mean [S, C]");
  check_f32(invstd, p.S * p.C, x0, "invstd [S, C]");
  check_f32(coefs, p.S * 2 * p.C, x0, "coefs [S, 2C]");
  auto f32 = x0.options().dtype(at::kFloat);
  auto sums = at::empty({p.S, 2 * p.C}, f32);
  at::Tensor gw, gb;
  if (weight_g) gw = at::empty({p.C}, f32);
  if (bias_g) gb = at::empty({p.C}, f32);
  const int total = p.first_chunk[p.S];
  at::Tensor ws = at::empty({(int64_t)std::max(total, 1) * p.C * 2},
                            x0.options().dtype(at::kDouble));
  const SegTable tab = make_table(p, inputs, &grad_outs, nullptr, false);
  if (total > 0) {
    dispatch_pack(p.dtype, [&](auto tv) {
      using T = typename decltype(tv)::type;
      constexpr int V = decltype(tv)::v;
      const dim3 grid((unsigned)p.ctiles, (unsigned)total);
      if (relu)
        hipLaunchKernelGGL((gbn_bwd_reduce_partial<T, V, kActRelu>), grid,
                           dim3(MSBN_BLOCK), 0, cur_stream(), tab,
                           mean.data_ptr<float>(), coefs.data_ptr<float>(),
                           ws.data_ptr<double>(), p.C, p.chunk_rows, p.lpr);
      else
        hipLaunchKernelGGL((gbn_bwd_reduce_partial<T, V, kActNone>), grid,
                           dim3(MSBN_BLOCK), 0, cur_stream(), tab,
                           mean.data_ptr<float>(), coefs.data_ptr<float>(),
                           ws.data_ptr<double>(), p.C, p.chunk_rows, p.lpr);
    });
  }
  hipLaunchKernelGGL(gbn_bwd_reduce_finalize,
                     dim3((unsigned)cdiv(p.C, kWavesPerBlock)),
                     dim3(MSBN_BLOCK), 0, cur_stream(), tab,
                     ws.data_ptr<double>(), p.C, invstd.data_ptr<float>(),
                     sums.data_ptr<float>(),
                     weight_g ? gw.data_ptr<float>() : nullptr,
                     bias_g ? gb.data_ptr<float>() : nullptr);
  return {sums, gw, gb};
}

std::vector<at::Tensor> batch_norm_backward_elemt_act_grouped(
    const std::vector<at::Tensor>& grad_outs,
    const std::vector<at::Tensor>& inputs, const at::Tensor& mean,
    const at::Tensor& invstd, const at::Tensor& coefs, const at::Tensor& sums,
    const at::Tensor& count, bool relu) {
  const GroupPlan p = checked_plan(inputs, &grad_outs,
                                   "batch_norm_backward_elemt_act_grouped");
  const at::Tensor& x0 = inputs[0];
  check_f32(mean, p.S * p.C, x0, "mean [S, C]");
  check_f32(invstd, p.S * p.C, x0, "invstd [S, C]");
  check_f32(coefs, p.S * 2 * p.C, x0, "coefs [S, 2C]");
  check_f32(sums, p.S * 2 * p.C, x0, "sums [S, 2C]");
  check_f32(count, p.S, x0, "count [S]");
  std::vector<at::Tensor> dxs = alloc_like_group(p, inputs);
  const int grid = p.first_eblock[p.S];
  if (grid == 0) return dxs;
  const SegTable tab = make_table(p, inputs, &grad_outs, &dxs, true);
  dispatch_pack(p.dtype, [&](auto tv) {
    using T = typename decltype(tv)::type;
    constexpr int V = decltype(tv)::v;
    if (relu)
      hipLaunchKernelGGL((gbn_bwd_elemt<T, V, kActRelu>), dim3((unsigned)grid),
                         dim3(MSBN_BLOCK), 0, cur_stream(), tab,
                         mean.data_ptr<float>(), invstd.data_ptr<float>(),
                         coefs.data_ptr<float>(), sums.data_ptr<float>(),
                         count.data_ptr<float>(), p.C);
    else
      hipLaunchKernelGGL((gbn_bwd_elemt<T, V, kActNone>), dim3((unsigned)grid),
                         dim3(MSBN_BLOCK), 0, cur_stream(), tab,
                         mean.data_ptr<float>(), invstd.data_ptr<float>(),
                         coefs.data_ptr<float>(), sums.data_ptr<float>(),
                         count.data_ptr<float>(), p.C);
  });
  return dxs;
}

// The reduction kinds report the chunk height of the group, each segment's
// chunk count and first block (= first workspace chunk) as nchunks_<s> /
// first_block_<s>; the elementwise kinds each segment's run of blocks as
// blocks_<s> / first_block_<s>.  The backward kinds take the gradients after
// the inputs: others = {x_1 .. x_{S-1}, dy_0 .. dy_{S-1}}.
std::tuple<std::string, std::map<std::string, int64_t>> launch_plan_grouped(
    const std::string& kind, const at::Tensor& input,
    const std::vector<c10::optional<at::Tensor>>& others) {
  std::map<std::string, int64_t> d;
  const bool bwd = kind == "bwd_reduce_grouped" || kind == "bwd_elemt_grouped";
  const bool red = kind == "stats_grouped" || kind == "bwd_reduce_grouped";
  std::vector<at::Tensor> all{input};
  for (const auto& t : others) {
    if (!t.has_value() || !t->defined()) return {"ineligible", d};
    all.push_back(*t);
  }
  if (bwd && all.size() % 2 != 0) return {"ineligible", d};
  const size_t S = bwd ? all.size() / 2 : all.size();
  const std::vector<at::Tensor> xs(all.begin(), all.begin() + S);
  const std::vector<at::Tensor> dys(all.begin() + S, all.end());
  std::vector<const std::vector<at::Tensor>*> lists{&xs};
  if (bwd) lists.push_back(&dys);
  const GroupPlan p = plan_group(lists);
  if (!p.ok) return {"ineligible", d};
  d["S"] = p.S;
  d["V"] = p.v;
  if (red) {
    d["chunk_rows"] = p.chunk_rows;
    d["lpr"] = p.lpr;
    d["ctiles"] = p.ctiles;
    d["total_chunks"] = p.first_chunk[p.S];
    d["trips"] = p.red_trips;
    d["flush_every"] = MSBN_ACC_FLUSH;
    int most = 0;
    for (int s = 0; s < p.S; ++s) {
      d["nchunks_" + std::to_string(s)] = p.nchunks[s];
      d["first_block_" + std::to_string(s)] = p.first_chunk[s];
      most = std::max(most, p.nchunks[s]);
    }
    d["finalize_trips"] = cdiv(most, MSBN_WAVE);
  } else {
    d["grid"] = p.first_eblock[p.S];
    d["packs"] = p.packs;
    d["trips"] = p.elemt_trips;
    d["multi_trip"] = p.elemt_trips > 1 ? 1 : 0;
    for (int s = 0; s < p.S; ++s) {
      d["blocks_" + std::to_string(s)] = p.eblocks[s];
      d["first_block_" + std::to_string(s)] = p.first_eblock[s];
    }
  }
  return {"nhwc", d};
}

}  // namespace msbn

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
