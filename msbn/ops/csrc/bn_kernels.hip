// msbn BatchNorm kernels for MI355X (gfx950, CDNA4).
//
// Replaces the stock SyncBatchNorm kernel family K1-K10 with
// an MI355X-first design:
//
//  * Reductions are TWO-STAGE: a `partial` kernel with a grid sized for the
//    256-CU chip (the stock one-block-per-channel shape leaves 3/4 of the chip
//    idle at C=64) writes per-chunk fp64 {sum, sumsq} pairs to a workspace; a
//    tiny `finalize` kernel combines them.  Deterministic (no atomics).  The
//    stats partials sum short fp32 chunks into fp64; a chunk whose raw sums
//    are ill-conditioned (mean^2/var > 64) is summed again around its own
//    mean and un-shifted in fp64 (common.hpp), so the error of
//    E[x^2]-E[x]^2 stays near the fp64 conditioning of the data.
//  * wave64 shuffle reductions + LDS partials inside each block.
//  * 16 B/lane vectorized loads (Pack<T,V>) for bf16/fp16/fp32, NCHW and
//    channels-last (NHWC) layouts both first-class.
//  * The sync path's cross-rank message is built IN the finalize kernel
//    ([mean | invstd | count] packed fp32), and the combine kernel masks
//    zero-count ranks in-device: no cat(), no GPU->CPU sync, hipGraph-safe.
//  * Elementwise kernels apply per-channel affine coefficients precomputed by
//    tiny kernels: y = x*scale+shift, dx = a*dy + b*x + d  (grid-stride,
//    capped grid, fused multiply-add form).
#include "bn_ops.hpp"
#include "common.hpp"

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace msbn {

namespace {

// =====================================================================
// stats partial: NCHW   grid(C, nchunkN, nchunkS) block 256
// ws layout: [C][nchunk][2] fp64, chunk = by*gridDim.z + bz
//
// Each block first sums raw {x, x^2} (AccPair, common.hpp).  If its chunk
// turns out ill-conditioned (needs_recentre) it reads the chunk a second
// time and sums d = x - pivot with pivot = the chunk's own mean, then
// un-shifts in fp64; the workspace holds plain {sum x, sum x^2} either way.
// =====================================================================
template <typename T, int V>
__global__ void bn_stats_partial_nchw(const T* __restrict__ x,
                                      double* __restrict__ ws, int64_t N,
                                      int64_t C, int64_t S, int64_t chunkN,
                                      int64_t chunkS) {
  const int64_t c = blockIdx.x;
  const int64_t n0 = blockIdx.y * chunkN;
  const int64_t n1 = i64min(n0 + chunkN, N);
  const int64_t s0 = blockIdx.z * chunkS;
  const int64_t s1 = i64min(s0 + chunkS, S);
  __shared__ double lds[2 * (MSBN_BLOCK / MSBN_WAVE)];
  __shared__ float pivot_s[2];  // {recentre?, pivot}
  float pivot = 0.f;
  double a = 0.0, b = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    AccPair acc;
    int since_flush = 0;
    for (int64_t n = n0; n < n1; ++n) {
      const T* row = x + (n * C + c) * S;
      if (V == 1) {
        for (int64_t s = s0 + threadIdx.x; s < s1; s += blockDim.x) {
          acc.add(to_f(nt_load1(&row[s])) - pivot);
          if (++since_flush == MSBN_ACC_FLUSH) {
            acc.flush();
            since_flush = 0;
          }
        }
      } else {
        for (int64_t s = s0 + (int64_t)threadIdx.x * V; s < s1;
             s += (int64_t)blockDim.x * V) {
          Pack<T, V> pk = nt_load<T, V>(&row[s]);
#pragma unroll
          for (int k = 0; k < V; ++k) acc.add(to_f(pk.v[k]) - pivot);
          if (++since_flush == MSBN_ACC_FLUSH / V) {
            acc.flush();
            since_flush = 0;
          }
        }
      }
    }
    acc.flush();
    a = acc.a;
    b = acc.b;
    if (pass) __syncthreads();  // lds is reused
    block_reduce_pair(a, b, lds);
    const double cnt = (double)((n1 - n0) * (s1 - s0));
    if (pass) {
      if (threadIdx.x == 0) unshift_pair(a, b, pivot, cnt);
      break;
    }
    if (threadIdx.x == 0) {
      const bool re = needs_recentre(a, b, cnt);
      pivot_s[0] = re ? 1.f : 0.f;
      pivot_s[1] = re ? (float)(a / cnt) : 0.f;
    }
    __syncthreads();
    if (pivot_s[0] == 0.f) break;
    pivot = pivot_s[1];
  }
  if (threadIdx.x == 0) {
    const int64_t chunk = (int64_t)blockIdx.y * gridDim.z + blockIdx.z;
    double* out = ws + (c * gridDim.y * gridDim.z + chunk) * 2;
    out[0] = a;
    out[1] = b;
  }
}

// V==1 fallback for layouts where the spatial extent is small or odd
// (e.g. S=49 at C=2048): flat index over the whole (n, s) chunk keeps every
// lane busy (the row-loop form idles blockDim-S threads per row).
template <typename T>
__global__ void bn_stats_partial_nchw_flat(const T* __restrict__ x,
                                           double* __restrict__ ws, int64_t N,
                                           int64_t C, int64_t S,
                                           int64_t chunk_len) {
  const int64_t c = blockIdx.x;
  const int64_t NS = N * S;
  const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
  const int64_t p1 = i64min(p0 + chunk_len, NS);
  __shared__ double lds[2 * (MSBN_BLOCK / MSBN_WAVE)];
  __shared__ float pivot_s[2];  // {recentre?, pivot}
  float pivot = 0.f;
  double a = 0.0, b = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    AccPair acc;
    int since_flush = 0;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
      const int64_t n = p / S, s = p - n * S;
      acc.add(to_f(nt_load1(&x[(n * C + c) * S + s])) - pivot);
      if (++since_flush == MSBN_ACC_FLUSH) {
        acc.flush();
        since_flush = 0;
      }
    }
    acc.flush();
    a = acc.a;
    b = acc.b;
    if (pass) __syncthreads();  // lds is reused
    block_reduce_pair(a, b, lds);
    const double cnt = (double)(p1 - p0);
    if (pass) {
      if (threadIdx.x == 0) unshift_pair(a, b, pivot, cnt);
      break;
    }
    if (threadIdx.x == 0) {
      const bool re = needs_recentre(a, b, cnt);
      pivot_s[0] = re ? 1.f : 0.f;
      pivot_s[1] = re ? (float)(a / cnt) : 0.f;
    }
    __syncthreads();
    if (pivot_s[0] == 0.f) break;
    pivot = pivot_s[1];
  }
  if (threadIdx.x == 0) {
    double* out = ws + (c * gridDim.y + blockIdx.y) * 2;
    out[0] = a;
    out[1] = b;
  }
}

// =====================================================================
// stats partial: NHWC   grid(ctiles, nchunk) block 256
// Each block covers channels [tile*lpr*V, ...) and a chunk of rows; thread
// (lane, rowoff) owns V consecutive channels.  LDS tree-reduce over rowoff.
// Same two passes as the NCHW kernel, decided per (block, channel); the
// second pass runs only if some channel of the block needs it.
// =====================================================================
template <typename T, int V>
__global__ void bn_stats_partial_nhwc(const T* __restrict__ x,
                                      double* __restrict__ ws, int64_t rows,
                                      int64_t C, int64_t chunk_rows, int lpr) {
  const int rpi = blockDim.x / lpr;  // rows in flight per iteration
  const int lane = threadIdx.x % lpr;
  const int rowoff = threadIdx.x / lpr;
  const bool active = rowoff < rpi;
  const int64_t c = (int64_t)blockIdx.x * lpr * V + (int64_t)lane * V;
  const bool inb = active && (c + V <= C);
  const int64_t r0 = (int64_t)blockIdx.y * chunk_rows;
  const int64_t r1 = i64min(r0 + chunk_rows, rows);

  // LDS layout [k][tid] with separate sum/sumsq planes: lane l of a wave
  // lands on bank (2*l) mod 64 for ds_*_b64 -> conflict-free (the [tid][k]
  // layout measured ~20 extra LDS cycles/instr via SQ_LDS_BANK_CONFLICT).
  __shared__ double sdata[MSBN_BLOCK * V * 2];

  float pivot[V];
  bool re[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    pivot[k] = 0.f;
    re[k] = false;
  }

  for (int pass = 0; pass < 2; ++pass) {
    AccPair acc[V];
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

    // LDS tree-reduce across the rowoff dimension (generic, non-pow2 safe).
    if (pass) __syncthreads();  // sdata is reused
#pragma unroll
    for (int k = 0; k < V; ++k) {
      sdata[k * MSBN_BLOCK + threadIdx.x] = a[k];
      sdata[(V + k) * MSBN_BLOCK + threadIdx.x] = b[k];
    }
    for (int st = 1; st < rpi; st <<= 1) {
      __syncthreads();
      if (active && (rowoff & ((st << 1) - 1)) == 0 && rowoff + st < rpi) {
        const int other = threadIdx.x + st * lpr;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          sdata[k * MSBN_BLOCK + threadIdx.x] += sdata[k * MSBN_BLOCK + other];
          sdata[(V + k) * MSBN_BLOCK + threadIdx.x] +=
              sdata[(V + k) * MSBN_BLOCK + other];
        }
      }
    }
    __syncthreads();
    int any = 0;
    if (rowoff == 0 && c < C) {
      const int64_t chunk = blockIdx.y;
      const double cnt = (double)(r1 - r0);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (c + k < C) {
          const double sa = sdata[k * MSBN_BLOCK + threadIdx.x];
          const double sb = sdata[(V + k) * MSBN_BLOCK + threadIdx.x];
          bool want = false;
          if (!pass) {
            want = needs_recentre(sa, sb, cnt);
            // publish {recentre?, pivot} in this thread's own sdata slots
            // (threadIdx.x == lane here); read back after the barrier below
            sdata[k * MSBN_BLOCK + threadIdx.x] = want ? 1.0 : 0.0;
            sdata[(V + k) * MSBN_BLOCK + threadIdx.x] = want ? sa / cnt : 0.0;
            any |= want ? 1 : 0;
          }
          // first pass: every channel that is fine as it is; second pass:
          // the re-centred ones
          if (pass ? re[k] : !want) {
            double* out = ws + ((c + k) * gridDim.y + chunk) * 2;
            out[0] = sa;
            out[1] = sb;
          }
        }
      }
    }
    if (pass) break;
    if (!__syncthreads_or(any)) break;  // block-uniform; publishes sdata
    if (inb) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        re[k] = sdata[k * MSBN_BLOCK + lane] != 0.0;
        // channels that were fine keep pivot 0: their second-pass sums are
        // simply not stored
        pivot[k] = re[k] ? (float)sdata[(V + k) * MSBN_BLOCK + lane] : 0.f;
      }
    }
  }
}

// =====================================================================
// stats finalize: combine chunk partials -> mean/invstd (+count, +running).
// ONE WAVE per channel (ws is channel-major [C][nchunks][2] -> coalesced
// lane-strided loads + wave64 shuffle reduce); nchunks may be in the
// thousands for small-C layers without serializing.
// =====================================================================
template <typename RT, typename WT>
__global__ void bn_stats_finalize(const double* __restrict__ ws, int nchunks,
                                  int64_t C, double count, float eps,
                                  float* __restrict__ mean,
                                  float* __restrict__ invstd,
                                  float* __restrict__ count_out,
                                  RT* __restrict__ rmean, RT* __restrict__ rvar,
                                  float momentum, const WT* __restrict__ w,
                                  const WT* __restrict__ bws,
                                  float* __restrict__ scale_out,
                                  float* __restrict__ shift_out) {
  const int lane = threadIdx.x & (MSBN_WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + wid;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int ch = lane; ch < nchunks; ch += MSBN_WAVE) {
    a += ws[(c * nchunks + ch) * 2];
    b += ws[(c * nchunks + ch) * 2 + 1];
  }
  wave_reduce_pair(a, b);
  if (lane != 0) return;
  const double m = a / count;
  double var = b / count - m * m;
  var = var > 0.0 ? var : 0.0;
  const float istd = (float)rsqrt(var + (double)eps);
  mean[c] = (float)m;
  invstd[c] = istd;
  if (c == 0 && count_out != nullptr) count_out[0] = (float)count;
  if (rmean != nullptr) {
    const double unbiased = count > 1.0 ? var * (count / (count - 1.0)) : var;
    rmean[c] = from_f<RT>((1.f - momentum) * to_f(rmean[c]) + momentum * (float)m);
    rvar[c] =
        from_f<RT>((1.f - momentum) * to_f(rvar[c]) + momentum * (float)unbiased);
  }
  if (scale_out != nullptr) {
    const float sc = istd * (w != nullptr ? to_f(w[c]) : 1.f);
    scale_out[c] = sc;
    shift_out[c] = -(float)m * sc + (bws != nullptr ? to_f(bws[c]) : 0.f);
  }
}

// =====================================================================
// gather: combine W ranks' packed [mean | invstd | count] rows.
// Zero-count ranks masked HERE (device-side; no host sync).
// =====================================================================
template <typename RT, typename WT>
__global__ void bn_gather_stats(const float* __restrict__ packed_all, int W,
                                int64_t C, float eps, float momentum,
                                float* __restrict__ mean,
                                float* __restrict__ invstd,
                                float* __restrict__ count_out,
                                RT* __restrict__ rmean, RT* __restrict__ rvar,
                                const WT* __restrict__ wpar,
                                const WT* __restrict__ bpar,
                                float* __restrict__ scale_out,
                                float* __restrict__ shift_out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const int64_t row = 2 * C + 1;
  double n_tot = 0.0, m_acc = 0.0, ex2 = 0.0;
  for (int w = 0; w < W; ++w) {
    const float cnt = packed_all[w * row + 2 * C];
    if (cnt > 0.f) {
      const double m = packed_all[w * row + c];
      const double istd = packed_all[w * row + C + c];
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
      rmean[c] =
          from_f<RT>((1.f - momentum) * to_f(rmean[c]) + momentum * (float)m_g);
      rvar[c] = from_f<RT>((1.f - momentum) * to_f(rvar[c]) +
                           momentum * (float)unbiased);
    }
  }
  mean[c] = m_out;
  invstd[c] = istd_out;
  if (c == 0 && count_out != nullptr) count_out[0] = (float)n_tot;
  if (scale_out != nullptr) {
    const float sc = istd_out * (wpar != nullptr ? to_f(wpar[c]) : 1.f);
    scale_out[c] = sc;
    shift_out[c] = -m_out * sc + (bpar != nullptr ? to_f(bpar[c]) : 0.f);
  }
}

// =====================================================================
// per-channel affine coefficient kernels (tiny)
// =====================================================================
template <typename WT>
__global__ void bn_affine_fwd(const float* __restrict__ mean,
                              const float* __restrict__ invstd,
                              const WT* __restrict__ w,
                              const WT* __restrict__ b, int64_t C,
                              float* __restrict__ scale,
                              float* __restrict__ shift) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sc = invstd[c] * (w != nullptr ? to_f(w[c]) : 1.f);
  scale[c] = sc;
  shift[c] = -mean[c] * sc + (b != nullptr ? to_f(b[c]) : 0.f);
}

// dx = a*dy + b*x + d with
//   f1 = invstd*gamma, f2 = sum_dy/n, f3 = invstd^2*sum_dy_xmu/n
//   a = f1, b = -f1*f3, d = f1*(f3*mean - f2)
template <typename WT>
__global__ void bn_affine_bwd(const float* __restrict__ mean,
                              const float* __restrict__ invstd,
                              const WT* __restrict__ w,
                              const float* __restrict__ sum_dy,
                              const float* __restrict__ sum_dy_xmu,
                              const float* __restrict__ count, int64_t C,
                              float* __restrict__ coef_a,
                              float* __restrict__ coef_b,
                              float* __restrict__ coef_d) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float n = count[0];
  if (n <= 0.f) {
    coef_a[c] = coef_b[c] = coef_d[c] = 0.f;
    return;
  }
  const float istd = invstd[c];
  const float f1 = istd * (w != nullptr ? to_f(w[c]) : 1.f);
  const float f2 = sum_dy[c] / n;
  const float f3 = istd * istd * sum_dy_xmu[c] / n;
  coef_a[c] = f1;
  coef_b[c] = -f1 * f3;
  coef_d[c] = f1 * (f3 * mean[c] - f2);
}

// =====================================================================
// elementwise: y = act(x*scale[c] + shift[c] [+ res])
// ACT / RES are compile-time: the fused BN(+add)+ReLU/LeakyReLU epilogue
// replaces the eager clamp / add kernels and their full-tensor round trips
// (guide G13: fuse into the producing kernel).  ACT is kActNone / kActRelu /
// kActLeaky (common.hpp); `slope` is only read by the kActLeaky
// instantiations, so none / relu keep their arithmetic.
//
// GATE(V = 8, RES, an activation): the thread also stores the byte of gate
// bits of its pack (common.hpp), taken from the z it already holds, so the
// backward reduce can take its branch from the bit and skip the res read.
// =====================================================================
template <typename T, int V, int ACT, bool RES, bool GATE>
__global__ void bn_elemt_nchw(const T* __restrict__ x,
                              const T* __restrict__ res, T* __restrict__ y,
                              const float* __restrict__ scale,
                              const float* __restrict__ shift, int64_t total,
                              int64_t C, int64_t S, float slope,
                              unsigned char* __restrict__ gate_out) {
  static_assert(!GATE || (V == 8 && RES && ACT != kActNone),
                "gate bits: one byte per 8-pack of a bn+add+act layer");
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const int64_t c = (e / S) % C;
    const float sc = scale[c], sh = shift[c];
    if (V == 1) {
      float z = to_f(nt_load1(&x[e])) * sc + sh;
      if (RES) z += to_f(nt_load1(&res[e]));
      z = act_fwd<ACT>(z, slope);
      nt_store1(&y[e], from_f<T>(z));
    } else {
      Pack<T, V> px = nt_load<T, V>(&x[e]);
      Pack<T, V> pr;
      if (RES) pr = nt_load<T, V>(&res[e]);
      Pack<T, V> py;
      unsigned bits = 0;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float z = to_f(px.v[k]) * sc + sh;
        if (RES) z += to_f(pr.v[k]);
        if (GATE) bits |= (unsigned)act_pass<ACT>(z) << k;
        z = act_fwd<ACT>(z, slope);
        py.v[k] = from_f<T>(z);
      }
      nt_store<T, V>(&y[e], py);
      if (GATE) gate_store(gate_out, e, bits);
    }
  }
}

template <typename T, int V, int ACT, bool RES, bool GATE>
__global__ void bn_elemt_nhwc(const T* __restrict__ x,
                              const T* __restrict__ res, T* __restrict__ y,
                              const float* __restrict__ scale,
                              const float* __restrict__ shift, int64_t total,
                              int64_t C, float slope,
                              unsigned char* __restrict__ gate_out) {
  static_assert(!GATE || (V == 8 && RES && ACT != kActNone),
                "gate bits: one byte per 8-pack of a bn+add+act layer");
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const int64_t c = e % C;
    if (V == 1) {
      float z = to_f(nt_load1(&x[e])) * scale[c] + shift[c];
      if (RES) z += to_f(nt_load1(&res[e]));
      z = act_fwd<ACT>(z, slope);
      nt_store1(&y[e], from_f<T>(z));
    } else {
      Pack<T, V> px = nt_load<T, V>(&x[e]);
      Pack<float, V> ps = *reinterpret_cast<const Pack<float, V>*>(&scale[c]);
      Pack<float, V> pb = *reinterpret_cast<const Pack<float, V>*>(&shift[c]);
      Pack<T, V> pr;
      if (RES) pr = nt_load<T, V>(&res[e]);
      Pack<T, V> py;
      unsigned bits = 0;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float z = to_f(px.v[k]) * ps.v[k] + pb.v[k];
        if (RES) z += to_f(pr.v[k]);
        if (GATE) bits |= (unsigned)act_pass<ACT>(z) << k;
        z = act_fwd<ACT>(z, slope);
        py.v[k] = from_f<T>(z);
      }
      nt_store<T, V>(&y[e], py);
      if (GATE) gate_store(gate_out, e, bits);
    }
  }
}

// =====================================================================
// backward reduce partial: {sum_g, sum_g*(x-mean)} per channel, where
// g = dy through the fused activation's gate when ACT (relu: z>0 ? dy : 0,
// leaky: z>0 ? dy : slope*dy): the pre-activation
// z = scale[c]*x + shift[c] (+ res) is recomputed in-kernel, so the fused
// forward never has to store a mask or the pre-activation tensor.
//
// DY2: the layer's output forked (residual block: conv1 and the skip path)
// and the two gradients arrive unsummed; the kernel reads both and folds
// autograd's `dy + dy2` pass (read 2A, write 1A) into its own dy read.  The
// fp32 sum is rounded to T ONCE before the gate, exactly what the eager
// add<T> kernel stored (fp32 opmath, round-to-nearest-even), so gm, the
// sums and everything downstream keep their bits.  Only instantiated with
// GMOUT: the second pass then reads gm and never needs dy / dy2 again.
//
// GATE: the forward stored act_pass(z) as one bit per element (gate bits,
// common.hpp) and the kernel takes its branch from that bit: it loads the
// byte its pack lies in instead of the res pack, and neither scale nor
// shift.  Excludes RES; only instantiated with GMOUT.  Everything after the
// gate is the code of the recomputing kernels, in their order.
// =====================================================================
template <typename T>
__device__ __forceinline__ float fork_grad(T g1, T g2) {
  return to_f(from_f<T>(to_f(g1) + to_f(g2)));
}

template <typename T, int V, int ACT, bool RES, bool GMOUT, bool DY2,
          bool GATE>
__global__ void bn_bwd_reduce_partial_nchw(const T* __restrict__ dy,
                                           const T* __restrict__ dy2,
                                           const T* __restrict__ x,
                                           const T* __restrict__ res,
                                           T* __restrict__ gm_out,
                                           const float* __restrict__ mean,
                                           const float* __restrict__ scale,
                                           const float* __restrict__ shift,
                                           double* __restrict__ ws, int64_t N,
                                           int64_t C, int64_t S, int64_t chunkN,
                                           int64_t chunkS, float slope,
                                           const unsigned char* __restrict__ gate) {
  static_assert(!GATE || (ACT != kActNone && !RES && GMOUT && V <= 8),
                "gate bits replace the res read of a gm-writing reduce");
  const int64_t c = blockIdx.x;
  const float m = mean[c];
  const float sc = (ACT && !GATE) ? scale[c] : 0.f;
  const float sh = (ACT && !GATE) ? shift[c] : 0.f;
  const int64_t n0 = blockIdx.y * chunkN;
  const int64_t n1 = i64min(n0 + chunkN, N);
  const int64_t s0 = blockIdx.z * chunkS;
  const int64_t s1 = i64min(s0 + chunkS, S);
  AccPair acc;
  int since_flush = 0;
  for (int64_t n = n0; n < n1; ++n) {
    const int64_t base = (n * C + c) * S;
    if (V == 1) {
      for (int64_t s = s0 + threadIdx.x; s < s1; s += blockDim.x) {
        float g = DY2 ? fork_grad(nt_load1(&dy[base + s]),
                                  nt_load1(&dy2[base + s]))
                      : to_f(nt_load1(&dy[base + s]));
        const float xv = to_f(nt_load1(&x[base + s]));
        if (GATE) {
          g = act_gate_bit<ACT>(gate_load(gate, base + s) & 1u, g, slope);
        } else if (ACT) {
          float z = sc * xv + sh;
          if (RES) z += to_f(nt_load1(&res[base + s]));
          g = act_gate<ACT>(z, g, slope);
        }
        if (GMOUT) nt_store1(&gm_out[base + s], from_f<T>(g));
        acc.add2(g, g * (xv - m));
        if (++since_flush == MSBN_ACC_FLUSH) {
          acc.flush();
          since_flush = 0;
        }
      }
    } else {
      for (int64_t s = s0 + (int64_t)threadIdx.x * V; s < s1;
           s += (int64_t)blockDim.x * V) {
        Pack<T, V> pg = nt_load<T, V>(&dy[base + s]);
        Pack<T, V> px = nt_load<T, V>(&x[base + s]);
        Pack<T, V> pg2, pr, pm;
        if (DY2) pg2 = nt_load<T, V>(&dy2[base + s]);
        if (RES) pr = nt_load<T, V>(&res[base + s]);
        unsigned bits = 0;
        if (GATE) bits = gate_load(gate, base + s);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          float g = DY2 ? fork_grad(pg.v[k], pg2.v[k]) : to_f(pg.v[k]);
          const float xv = to_f(px.v[k]);
          if (GATE) {
            g = act_gate_bit<ACT>((bits >> k) & 1u, g, slope);
          } else if (ACT) {
            float z = sc * xv + sh;
            if (RES) z += to_f(pr.v[k]);
            g = act_gate<ACT>(z, g, slope);
          }
          if (GMOUT) pm.v[k] = from_f<T>(g);
          acc.add2(g, g * (xv - m));
        }
        if (GMOUT) nt_store<T, V>(&gm_out[base + s], pm);
        if (++since_flush == MSBN_ACC_FLUSH / V) {
          acc.flush();
          since_flush = 0;
        }
      }
    }
  }
  acc.flush();
  double a = acc.a, b = acc.b;
  __shared__ double lds[2 * (MSBN_BLOCK / MSBN_WAVE)];
  block_reduce_pair(a, b, lds);
  if (threadIdx.x == 0) {
    const int64_t chunk = (int64_t)blockIdx.y * gridDim.z + blockIdx.z;
    double* out = ws + (c * gridDim.y * gridDim.z + chunk) * 2;
    out[0] = a;
    out[1] = b;
  }
}

template <typename T, int ACT, bool RES, bool GMOUT, bool DY2, bool GATE>
__global__ void bn_bwd_reduce_partial_nchw_flat(
    const T* __restrict__ dy, const T* __restrict__ dy2,
    const T* __restrict__ x,
    const T* __restrict__ res, T* __restrict__ gm_out,
    const float* __restrict__ mean,
    const float* __restrict__ scale, const float* __restrict__ shift,
    double* __restrict__ ws, int64_t N, int64_t C, int64_t S,
    int64_t chunk_len, float slope, const unsigned char* __restrict__ gate) {
  static_assert(!GATE || (ACT != kActNone && !RES && GMOUT),
                "gate bits replace the res read of a gm-writing reduce");
  const int64_t c = blockIdx.x;
  const float m = mean[c];
  const float sc = (ACT && !GATE) ? scale[c] : 0.f;
  const float sh = (ACT && !GATE) ? shift[c] : 0.f;
  const int64_t NS = N * S;
  const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
  const int64_t p1 = i64min(p0 + chunk_len, NS);
  AccPair acc;
  int since_flush = 0;
  for (int64_t p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
    const int64_t n = p / S, s = p - n * S;
    const int64_t e = (n * C + c) * S + s;
    float g = DY2 ? fork_grad(nt_load1(&dy[e]), nt_load1(&dy2[e]))
                  : to_f(nt_load1(&dy[e]));
    const float xv = to_f(nt_load1(&x[e]));
    if (GATE) {
      g = act_gate_bit<ACT>(gate_load(gate, e) & 1u, g, slope);
    } else if (ACT) {
      float z = sc * xv + sh;
      if (RES) z += to_f(nt_load1(&res[e]));
      g = act_gate<ACT>(z, g, slope);
    }
    if (GMOUT) nt_store1(&gm_out[e], from_f<T>(g));
    acc.add2(g, g * (xv - m));
    if (++since_flush == MSBN_ACC_FLUSH) {
      acc.flush();
      since_flush = 0;
    }
  }
  acc.flush();
  double a = acc.a, b = acc.b;
  __shared__ double lds[2 * (MSBN_BLOCK / MSBN_WAVE)];
  block_reduce_pair(a, b, lds);
  if (threadIdx.x == 0) {
    double* out = ws + (c * gridDim.y + blockIdx.y) * 2;
    out[0] = a;
    out[1] = b;
  }
}

template <typename T, int V, int ACT, bool RES, bool GMOUT, bool DY2,
          bool GATE>
__global__ void bn_bwd_reduce_partial_nhwc(const T* __restrict__ dy,
                                           const T* __restrict__ dy2,
                                           const T* __restrict__ x,
                                           const T* __restrict__ res,
                                           T* __restrict__ gm_out,
                                           const float* __restrict__ mean,
                                           const float* __restrict__ scale,
                                           const float* __restrict__ shift,
                                           double* __restrict__ ws,
                                           int64_t rows, int64_t C,
                                           int64_t chunk_rows, int lpr,
                                           float slope,
                                           const unsigned char* __restrict__ gate) {
  static_assert(!GATE || (ACT != kActNone && !RES && GMOUT && V <= 8),
                "gate bits replace the res read of a gm-writing reduce");
  const int rpi = blockDim.x / lpr;
  const int lane = threadIdx.x % lpr;
  const int rowoff = threadIdx.x / lpr;
  const bool active = rowoff < rpi;
  const int64_t c = (int64_t)blockIdx.x * lpr * V + (int64_t)lane * V;
  const bool inb = active && (c + V <= C);

  AccPair acc[V];
  float m[V], scv[V], shv[V];
#pragma unroll
  for (int k = 0; k < V; ++k) m[k] = scv[k] = shv[k] = 0.f;
  if (inb) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      m[k] = mean[c + k];
      if (ACT && !GATE) {
        scv[k] = scale[c + k];
        shv[k] = shift[c + k];
      }
    }
    const int64_t r0 = (int64_t)blockIdx.y * chunk_rows;
    const int64_t r1 = i64min(r0 + chunk_rows, rows);
    int since_flush = 0;
    for (int64_t r = r0 + rowoff; r < r1; r += rpi) {
      Pack<T, V> pg = nt_load<T, V>(&dy[r * C + c]);
      Pack<T, V> px = nt_load<T, V>(&x[r * C + c]);
      Pack<T, V> pg2, pr, pm;
      if (DY2) pg2 = nt_load<T, V>(&dy2[r * C + c]);
      if (RES) pr = nt_load<T, V>(&res[r * C + c]);
      unsigned bits = 0;
      if (GATE) bits = gate_load(gate, r * C + c);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float g = DY2 ? fork_grad(pg.v[k], pg2.v[k]) : to_f(pg.v[k]);
        const float xv = to_f(px.v[k]);
        if (GATE) {
          g = act_gate_bit<ACT>((bits >> k) & 1u, g, slope);
        } else if (ACT) {
          float z = scv[k] * xv + shv[k];
          if (RES) z += to_f(pr.v[k]);
          g = act_gate<ACT>(z, g, slope);
        }
        if (GMOUT) pm.v[k] = from_f<T>(g);
        acc[k].add2(g, g * (xv - m[k]));
      }
      if (GMOUT) nt_store<T, V>(&gm_out[r * C + c], pm);
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
  // LDS layout [k][tid] with separate sum/sumsq planes: lane l of a wave
  // lands on bank (2*l) mod 64 for ds_*_b64 -> conflict-free (the [tid][k]
  // layout measured ~20 extra LDS cycles/instr via SQ_LDS_BANK_CONFLICT).
  __shared__ double sdata[MSBN_BLOCK * V * 2];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    sdata[k * MSBN_BLOCK + threadIdx.x] = a[k];
    sdata[(V + k) * MSBN_BLOCK + threadIdx.x] = b[k];
  }
  for (int st = 1; st < rpi; st <<= 1) {
    __syncthreads();
    if (active && (rowoff & ((st << 1) - 1)) == 0 && rowoff + st < rpi) {
      const int other = threadIdx.x + st * lpr;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        sdata[k * MSBN_BLOCK + threadIdx.x] += sdata[k * MSBN_BLOCK + other];
        sdata[(V + k) * MSBN_BLOCK + threadIdx.x] +=
            sdata[(V + k) * MSBN_BLOCK + other];
      }
    }
  }
  __syncthreads();
  if (rowoff == 0 && c < C) {
    const int64_t chunk = blockIdx.y;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (c + k < C) {
        double* out = ws + ((c + k) * gridDim.y + chunk) * 2;
        out[0] = sdata[k * MSBN_BLOCK + threadIdx.x];
        out[1] = sdata[(V + k) * MSBN_BLOCK + threadIdx.x];
      }
    }
  }
}

// one wave per channel (see bn_stats_finalize)
template <typename WT>
__global__ void bn_bwd_reduce_finalize(const double* __restrict__ ws,
                                       int nchunks, int64_t C,
                                       const float* __restrict__ invstd,
                                       float* __restrict__ sum_dy,
                                       float* __restrict__ sum_dy_xmu,
                                       WT* __restrict__ grad_weight,
                                       WT* __restrict__ grad_bias) {
  const int lane = threadIdx.x & (MSBN_WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + wid;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int ch = lane; ch < nchunks; ch += MSBN_WAVE) {
    a += ws[(c * nchunks + ch) * 2];
    b += ws[(c * nchunks + ch) * 2 + 1];
  }
  wave_reduce_pair(a, b);
  if (lane != 0) return;
  if (sum_dy != nullptr) sum_dy[c] = (float)a;
  if (sum_dy_xmu != nullptr) sum_dy_xmu[c] = (float)b;
  if (grad_weight != nullptr) grad_weight[c] = from_f<WT>((float)(b * invstd[c]));
  if (grad_bias != nullptr) grad_bias[c] = from_f<WT>((float)a);
}

// =====================================================================
// backward elementwise: dx = a[c]*g + b[c]*x + d[c], with the activation
// gate recomputed in-kernel when ACT (g = z>0 ? dy : 0 or slope*dy); RESG
// additionally writes the residual-branch gradient dres = g (the add node's
// pass-through).
// =====================================================================
template <typename T, int V, int ACT, bool RES, bool RESG>
__global__ void bn_bwd_elemt_nchw(const T* __restrict__ dy,
                                  const T* __restrict__ x,
                                  const T* __restrict__ res,
                                  T* __restrict__ dx, T* __restrict__ dres,
                                  const float* __restrict__ ca,
                                  const float* __restrict__ cb,
                                  const float* __restrict__ cd,
                                  const float* __restrict__ scale,
                                  const float* __restrict__ shift,
                                  int64_t total, int64_t C, int64_t S,
                                  float slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const int64_t c = (e / S) % C;
    const float A = ca[c], B = cb[c], D = cd[c];
    const float sc = ACT ? scale[c] : 0.f;
    const float sh = ACT ? shift[c] : 0.f;
    if (V == 1) {
      float g = to_f(nt_load1(&dy[e]));
      const float xv = to_f(nt_load1(&x[e]));
      if (ACT) {
        float z = sc * xv + sh;
        if (RES) z += to_f(nt_load1(&res[e]));
        g = act_gate<ACT>(z, g, slope);
      }
      nt_store1(&dx[e], from_f<T>(A * g + B * xv + D));
      if (RESG) nt_store1(&dres[e], from_f<T>(g));
    } else {
      Pack<T, V> pg = nt_load<T, V>(&dy[e]);
      Pack<T, V> px = nt_load<T, V>(&x[e]);
      Pack<T, V> pr;
      if (RES) pr = nt_load<T, V>(&res[e]);
      Pack<T, V> po, pq;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float g = to_f(pg.v[k]);
        const float xv = to_f(px.v[k]);
        if (ACT) {
          float z = sc * xv + sh;
          if (RES) z += to_f(pr.v[k]);
          g = act_gate<ACT>(z, g, slope);
        }
        po.v[k] = from_f<T>(A * g + B * xv + D);
        if (RESG) pq.v[k] = from_f<T>(g);
      }
      nt_store<T, V>(&dx[e], po);
      if (RESG) nt_store<T, V>(&dres[e], pq);
    }
  }
}

template <typename T, int V, int ACT, bool RES, bool RESG>
__global__ void bn_bwd_elemt_nhwc(const T* __restrict__ dy,
                                  const T* __restrict__ x,
                                  const T* __restrict__ res,
                                  T* __restrict__ dx, T* __restrict__ dres,
                                  const float* __restrict__ ca,
                                  const float* __restrict__ cb,
                                  const float* __restrict__ cd,
                                  const float* __restrict__ scale,
                                  const float* __restrict__ shift,
                                  int64_t total, int64_t C, float slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const int64_t c = e % C;
    if (V == 1) {
      float g = to_f(nt_load1(&dy[e]));
      const float xv = to_f(nt_load1(&x[e]));
      if (ACT) {
        float z = scale[c] * xv + shift[c];
        if (RES) z += to_f(nt_load1(&res[e]));
        g = act_gate<ACT>(z, g, slope);
      }
      nt_store1(&dx[e], from_f<T>(ca[c] * g + cb[c] * xv + cd[c]));
      if (RESG) nt_store1(&dres[e], from_f<T>(g));
    } else {
      Pack<T, V> pg = nt_load<T, V>(&dy[e]);
      Pack<T, V> px = nt_load<T, V>(&x[e]);
      Pack<float, V> pa = *reinterpret_cast<const Pack<float, V>*>(&ca[c]);
      Pack<float, V> pb = *reinterpret_cast<const Pack<float, V>*>(&cb[c]);
      Pack<float, V> pd = *reinterpret_cast<const Pack<float, V>*>(&cd[c]);
      Pack<float, V> psc, psh;
      if (ACT) {
        psc = *reinterpret_cast<const Pack<float, V>*>(&scale[c]);
        psh = *reinterpret_cast<const Pack<float, V>*>(&shift[c]);
      }
      Pack<T, V> pr;
      if (RES) pr = nt_load<T, V>(&res[e]);
      Pack<T, V> po, pq;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float g = to_f(pg.v[k]);
        const float xv = to_f(px.v[k]);
        if (ACT) {
          float z = psc.v[k] * xv + psh.v[k];
          if (RES) z += to_f(pr.v[k]);
          g = act_gate<ACT>(z, g, slope);
        }
        po.v[k] = from_f<T>(pa.v[k] * g + pb.v[k] * xv + pd.v[k]);
        if (RESG) pq.v[k] = from_f<T>(g);
      }
      nt_store<T, V>(&dx[e], po);
      if (RESG) nt_store<T, V>(&dres[e], pq);
    }
  }
}

// =====================================================================
// dual BN: relu(bn(x) + bn_d(x_d)), the first block of a ResNet stage, whose
// skip path has a BatchNorm of its own (docs/KERNEL_DESIGN.md "Dual BN").
// Three kernels stand in for the five of the composition
//   bn_elemt_nhwc<none>(x_d) -> r,  bn_elemt_nhwc<relu, RES, GATE>(x, r)
//   bn_bwd_reduce_partial_nhwc<relu, GM, DY2?, GATE>, then <none> on (gm, x_d)
//   bn_bwd_elemt_nhwc<none> on (gm, x) and on (gm, x_d)
// so r is never stored and gm is read once per pass for both layers.
// Channels-last, 8 elements per thread, bf16 / half, ReLU, gate bits; the
// host declines everything else and the composition runs.  Every expression
// is the one the single kernels use, in their order, and the reduce runs on
// the single reduce's launch plan: the results are the composition's bits.
// =====================================================================
template <typename T>
__global__ void bn_elemt_dual_nhwc(const T* __restrict__ x,
                                   const T* __restrict__ x2,
                                   T* __restrict__ y,
                                   const float* __restrict__ scale,
                                   const float* __restrict__ shift,
                                   const float* __restrict__ scale2,
                                   const float* __restrict__ shift2,
                                   int64_t total, int64_t C,
                                   unsigned char* __restrict__ gate_out) {
  constexpr int V = 8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const int64_t c = e % C;
    Pack<T, V> px = nt_load<T, V>(&x[e]);
    Pack<T, V> px2 = nt_load<T, V>(&x2[e]);
    Pack<float, V> ps = *reinterpret_cast<const Pack<float, V>*>(&scale[c]);
    Pack<float, V> pb = *reinterpret_cast<const Pack<float, V>*>(&shift[c]);
    Pack<float, V> ps2 = *reinterpret_cast<const Pack<float, V>*>(&scale2[c]);
    Pack<float, V> pb2 = *reinterpret_cast<const Pack<float, V>*>(&shift2[c]);
    Pack<T, V> py;
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      // the skip BN's output, rounded to T as its own kernel stores it
      const T r = from_f<T>(to_f(px2.v[k]) * ps2.v[k] + pb2.v[k]);
      float z = to_f(px.v[k]) * ps.v[k] + pb.v[k];
      z += to_f(r);
      bits |= (unsigned)act_pass<kActRelu>(z) << k;
      z = act_fwd<kActRelu>(z, 0.f);
      py.v[k] = from_f<T>(z);
    }
    nt_store<T, V>(&y[e], py);
    gate_store(gate_out, e, bits);
  }
}

// Block tree reduction of one layer's per-thread fp64 pairs over sdata and
// the store of the block's partials (the tail of bn_bwd_reduce_partial_nhwc).
template <int V>
__device__ __forceinline__ void nhwc_tree_reduce_store(
    const double (&a)[V], const double (&b)[V], double* sdata,
    double* __restrict__ ws, int64_t c, int64_t C, int lpr, int rpi,
    int rowoff, bool active) {
#pragma unroll
  for (int k = 0; k < V; ++k) {
    sdata[k * MSBN_BLOCK + threadIdx.x] = a[k];
    sdata[(V + k) * MSBN_BLOCK + threadIdx.x] = b[k];
  }
  for (int st = 1; st < rpi; st <<= 1) {
    __syncthreads();
    if (active && (rowoff & ((st << 1) - 1)) == 0 && rowoff + st < rpi) {
      const int other = threadIdx.x + st * lpr;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        sdata[k * MSBN_BLOCK + threadIdx.x] += sdata[k * MSBN_BLOCK + other];
        sdata[(V + k) * MSBN_BLOCK + threadIdx.x] +=
            sdata[(V + k) * MSBN_BLOCK + other];
      }
    }
  }
  __syncthreads();
  if (rowoff == 0 && c < C) {
    const int64_t chunk = blockIdx.y;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (c + k < C) {
        double* out = ws + ((c + k) * gridDim.y + chunk) * 2;
        out[0] = sdata[k * MSBN_BLOCK + threadIdx.x];
        out[1] = sdata[(V + k) * MSBN_BLOCK + threadIdx.x];
      }
    }
  }
}

// g*(x - mean) rounded on its own, never fused into the add that follows:
// what the single V = 8 reduce kernels compile to, for both layers.  The
// compiler is otherwise free to contract each kernel differently (it fused
// the skip layer's product here and not in the single kernel), and one fused
// product moves the last bit of a sum.
__device__ __forceinline__ float mul_unfused(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// Traversal, gate and flush interval of
// bn_bwd_reduce_partial_nhwc<T, 8, relu, false, true, DY2, true>.  The gated
// gradient g is a value of T (the relu gate passes or zeroes one), so the
// skip layer's plain reduce over gm would add the very g in the very order:
// its sum of g IS this layer's, and only sum g*(x_d - mean_d) needs
// accumulators of its own.  The two layers' pairs go through the tree one
// after the other over the same 32 KiB of LDS.
template <typename T, bool DY2>
__global__ void bn_bwd_reduce_dual_partial_nhwc(
    const T* __restrict__ dy, const T* __restrict__ dy2,
    const T* __restrict__ x, const T* __restrict__ x2,
    T* __restrict__ gm_out, const float* __restrict__ mean,
    const float* __restrict__ mean2, double* __restrict__ ws,
    double* __restrict__ ws2, int64_t rows, int64_t C, int64_t chunk_rows,
    int lpr, const unsigned char* __restrict__ gate) {
  constexpr int V = 8;
  const int rpi = blockDim.x / lpr;
  const int lane = threadIdx.x % lpr;
  const int rowoff = threadIdx.x / lpr;
  const bool active = rowoff < rpi;
  const int64_t c = (int64_t)blockIdx.x * lpr * V + (int64_t)lane * V;
  const bool inb = active && (c + V <= C);

  // acc2: only its second component is read; the first is this layer's
  AccPair acc[V], acc2[V];
  float m[V], m2[V];
#pragma unroll
  for (int k = 0; k < V; ++k) m[k] = m2[k] = 0.f;
  if (inb) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      m[k] = mean[c + k];
      m2[k] = mean2[c + k];
    }
    const int64_t r0 = (int64_t)blockIdx.y * chunk_rows;
    const int64_t r1 = i64min(r0 + chunk_rows, rows);
    int since_flush = 0;
    for (int64_t r = r0 + rowoff; r < r1; r += rpi) {
      Pack<T, V> pg = nt_load<T, V>(&dy[r * C + c]);
      Pack<T, V> px = nt_load<T, V>(&x[r * C + c]);
      Pack<T, V> px2 = nt_load<T, V>(&x2[r * C + c]);
      Pack<T, V> pg2, pm;
      if (DY2) pg2 = nt_load<T, V>(&dy2[r * C + c]);
      const unsigned bits = gate_load(gate, r * C + c);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float g = DY2 ? fork_grad(pg.v[k], pg2.v[k]) : to_f(pg.v[k]);
        const float xv = to_f(px.v[k]);
        const float xv2 = to_f(px2.v[k]);
        g = act_gate_bit<kActRelu>((bits >> k) & 1u, g, 0.f);
        pm.v[k] = from_f<T>(g);
        acc[k].add2(g, mul_unfused(g, xv - m[k]));
        acc2[k].add2(g, mul_unfused(g, xv2 - m2[k]));
      }
      nt_store<T, V>(&gm_out[r * C + c], pm);
      if (++since_flush == MSBN_ACC_FLUSH) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          acc[k].flush();
          acc2[k].flush();
        }
        since_flush = 0;
      }
    }
  }
  double a[V], b[V], b2[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    acc[k].flush();
    acc2[k].flush();
    a[k] = acc[k].a;
    b[k] = acc[k].b;
    b2[k] = acc2[k].b;
  }
  // [k][tid] planes as in bn_bwd_reduce_partial_nhwc (conflict-free)
  __shared__ double sdata[MSBN_BLOCK * V * 2];
  nhwc_tree_reduce_store<V>(a, b, sdata, ws, c, C, lpr, rpi, rowoff, active);
  __syncthreads();
  nhwc_tree_reduce_store<V>(a, b2, sdata, ws2, c, C, lpr, rpi, rowoff, active);
}

// dx = a*gm + b*x + d and dx2 = a2*gm + b2*x2 + d2 from one read of gm: the
// expressions of bn_bwd_elemt_nhwc<T, 8, none, false, false>.  co / co2 are
// the packed [a | b | d] rows bn_affine_bwd wrote.
template <typename T>
__global__ void bn_bwd_elemt_dual_nhwc(const T* __restrict__ gm,
                                       const T* __restrict__ x,
                                       const T* __restrict__ x2,
                                       T* __restrict__ dx,
                                       T* __restrict__ dx2,
                                       const float* __restrict__ co,
                                       const float* __restrict__ co2,
                                       int64_t total, int64_t C) {
  constexpr int V = 8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const int64_t c = e % C;
    Pack<T, V> pg = nt_load<T, V>(&gm[e]);
    Pack<T, V> px = nt_load<T, V>(&x[e]);
    Pack<T, V> px2 = nt_load<T, V>(&x2[e]);
    Pack<float, V> pa = *reinterpret_cast<const Pack<float, V>*>(&co[c]);
    Pack<float, V> pb = *reinterpret_cast<const Pack<float, V>*>(&co[C + c]);
    Pack<float, V> pd =
        *reinterpret_cast<const Pack<float, V>*>(&co[2 * C + c]);
    Pack<float, V> pa2 = *reinterpret_cast<const Pack<float, V>*>(&co2[c]);
    Pack<float, V> pb2 = *reinterpret_cast<const Pack<float, V>*>(&co2[C + c]);
    Pack<float, V> pd2 =
        *reinterpret_cast<const Pack<float, V>*>(&co2[2 * C + c]);
    Pack<T, V> po, po2;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float g = to_f(pg.v[k]);
      const float xv = to_f(px.v[k]);
      const float xv2 = to_f(px2.v[k]);
      po.v[k] = from_f<T>(pa.v[k] * g + pb.v[k] * xv + pd.v[k]);
      po2.v[k] = from_f<T>(pa2.v[k] * g + pb2.v[k] * xv2 + pd2.v[k]);
    }
    nt_store<T, V>(&dx[e], po);
    nt_store<T, V>(&dx2[e], po2);
  }
}

// =====================================================================
// frozen path: the statistics are the (fixed) running stats, so there is no
// batch reduction anywhere.  One tiny kernel folds (running_mean,
// running_var, eps, weight, bias) into the packed [scale | shift] buffer the
// forward elemt kernels consume; backward is ONE elementwise pass
//   dx = scale[c]*g,  dres = g,  g = dy * 1[z > 0]  (leaky: slope*dy else)
// with the activation gate recomputed from (x, scale, shift[, res]) exactly
// as bn_bwd_elemt_* does.  Without the gate (kActNone) x is never read, so
// the layer does not have to keep its input alive.
// =====================================================================
template <typename RT, typename WT>
__global__ void bn_frozen_coefs(const RT* __restrict__ rmean,
                                const RT* __restrict__ rvar, float eps,
                                const WT* __restrict__ w,
                                const WT* __restrict__ b, int64_t C,
                                float* __restrict__ scale,
                                float* __restrict__ shift) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float istd = (float)rsqrt((double)to_f(rvar[c]) + (double)eps);
  const float sc = istd * (w != nullptr ? to_f(w[c]) : 1.f);
  scale[c] = sc;
  shift[c] = -to_f(rmean[c]) * sc + (b != nullptr ? to_f(b[c]) : 0.f);
}

// x / res are only dereferenced when ACT (the host passes nullptr
// otherwise); dx may be nullptr when only the residual branch needs its
// gradient (wave-uniform branch).
template <typename T, int V, int ACT, bool RES, bool RESG>
__global__ void bn_frozen_bwd_elemt_nchw(const T* __restrict__ dy,
                                         const T* __restrict__ x,
                                         const T* __restrict__ res,
                                         T* __restrict__ dx,
                                         T* __restrict__ dres,
                                         const float* __restrict__ scale,
                                         const float* __restrict__ shift,
                                         int64_t total, int64_t C, int64_t S,
                                         float slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const int64_t c = (e / S) % C;
    const float sc = scale[c];
    const float sh = ACT ? shift[c] : 0.f;
    if (V == 1) {
      float g = to_f(nt_load1(&dy[e]));
      if (ACT) {
        float z = sc * to_f(nt_load1(&x[e])) + sh;
        if (RES) z += to_f(nt_load1(&res[e]));
        g = act_gate<ACT>(z, g, slope);
      }
      if (dx != nullptr) nt_store1(&dx[e], from_f<T>(sc * g));
      if (RESG) nt_store1(&dres[e], from_f<T>(g));
    } else {
      Pack<T, V> pg = nt_load<T, V>(&dy[e]);
      Pack<T, V> px, pr;
      if (ACT) px = nt_load<T, V>(&x[e]);
      if (ACT && RES) pr = nt_load<T, V>(&res[e]);
      Pack<T, V> po, pq;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float g = to_f(pg.v[k]);
        if (ACT) {
          float z = sc * to_f(px.v[k]) + sh;
          if (RES) z += to_f(pr.v[k]);
          g = act_gate<ACT>(z, g, slope);
        }
        po.v[k] = from_f<T>(sc * g);
        if (RESG) pq.v[k] = from_f<T>(g);
      }
      if (dx != nullptr) nt_store<T, V>(&dx[e], po);
      if (RESG) nt_store<T, V>(&dres[e], pq);
    }
  }
}

template <typename T, int V, int ACT, bool RES, bool RESG>
__global__ void bn_frozen_bwd_elemt_nhwc(const T* __restrict__ dy,
                                         const T* __restrict__ x,
                                         const T* __restrict__ res,
                                         T* __restrict__ dx,
                                         T* __restrict__ dres,
                                         const float* __restrict__ scale,
                                         const float* __restrict__ shift,
                                         int64_t total, int64_t C,
                                         float slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const int64_t c = e % C;
    if (V == 1) {
      float g = to_f(nt_load1(&dy[e]));
      const float sc = scale[c];
      if (ACT) {
        float z = sc * to_f(nt_load1(&x[e])) + shift[c];
        if (RES) z += to_f(nt_load1(&res[e]));
        g = act_gate<ACT>(z, g, slope);
      }
      if (dx != nullptr) nt_store1(&dx[e], from_f<T>(sc * g));
      if (RESG) nt_store1(&dres[e], from_f<T>(g));
    } else {
      Pack<T, V> pg = nt_load<T, V>(&dy[e]);
      Pack<float, V> psc = *reinterpret_cast<const Pack<float, V>*>(&scale[c]);
      Pack<float, V> psh;
      Pack<T, V> px, pr;
      if (ACT) {
        psh = *reinterpret_cast<const Pack<float, V>*>(&shift[c]);
        px = nt_load<T, V>(&x[e]);
      }
      if (ACT && RES) pr = nt_load<T, V>(&res[e]);
      Pack<T, V> po, pq;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float g = to_f(pg.v[k]);
        if (ACT) {
          float z = psc.v[k] * to_f(px.v[k]) + psh.v[k];
          if (RES) z += to_f(pr.v[k]);
          g = act_gate<ACT>(z, g, slope);
        }
        po.v[k] = from_f<T>(psc.v[k] * g);
        if (RESG) pq.v[k] = from_f<T>(g);
      }
      if (dx != nullptr) nt_store<T, V>(&dx[e], po);
      if (RESG) nt_store<T, V>(&dres[e], pq);
    }
  }
}

// =====================================================================
// small-plane world-1 fused kernels (the stock K10-style single-launch
// family, MI355X-gated): block-per-channel, TWO passes over an L2-resident
// plane.  Used when plane = N*S is small (GAN / small-per-GPU-batch
// regime): there the per-launch ramp of the 3-kernel
// two-stage pipeline dominates and the plane fits cache, so the second
// pass re-reads from L2 (plain cached accesses on purpose — no nt).
// NCHW only; fp32 running stats / fp32 affine (host gates eligibility).
// =====================================================================
// V-wide flat indexing: pack pp covers elements [pp*V, pp*V+V) of the
// channel plane; S % V == 0 (host-gated) keeps every pack inside one row.
// int32 arithmetic throughout (plane <= 32K elems by gate).
template <typename T, int V, int ACT, bool RES>
__global__ void bn_fwd_fused_small_nchw(
    const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
    int N, int64_t C, int S, float eps, float momentum,
    float* __restrict__ mean_out, float* __restrict__ invstd_out,
    float* __restrict__ count_out, float* __restrict__ rmean,
    float* __restrict__ rvar, const float* __restrict__ w,
    const float* __restrict__ b, float* __restrict__ scale_out,
    float* __restrict__ shift_out, float slope) {
  const int64_t c = blockIdx.x;
  const int plane = N * S;
  const int packs = plane / V;
  double a = 0.0, bb = 0.0;
  for (int pp = threadIdx.x; pp < packs; pp += blockDim.x) {
    const int e = pp * V;
    const int n = e / S, s = e - n * S;
    const T* row = x + ((int64_t)n * C + c) * S + s;
    Pack<T, V> pk = *reinterpret_cast<const Pack<T, V>*>(row);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float v = to_f(pk.v[k]);
      a += v;
      bb += (double)v * v;
    }
  }
  __shared__ double lds[2 * (MSBN_BLOCK / MSBN_WAVE)];
  block_reduce_pair(a, bb, lds);
  __shared__ float sc_sh[2];
  if (threadIdx.x == 0) {
    const double cnt = (double)plane;
    const double m = a / cnt;
    double var = bb / cnt - m * m;
    var = var > 0.0 ? var : 0.0;
    const float istd = (float)rsqrt(var + (double)eps);
    mean_out[c] = (float)m;
    invstd_out[c] = istd;
    if (c == 0 && count_out != nullptr) count_out[0] = (float)cnt;
    if (rmean != nullptr) {
      const double unbiased = cnt > 1.0 ? var * (cnt / (cnt - 1.0)) : var;
      rmean[c] = (1.f - momentum) * rmean[c] + momentum * (float)m;
      rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unbiased;
    }
    const float sc = istd * (w != nullptr ? w[c] : 1.f);
    const float sh = -(float)m * sc + (b != nullptr ? b[c] : 0.f);
    scale_out[c] = sc;
    shift_out[c] = sh;
    sc_sh[0] = sc;
    sc_sh[1] = sh;
  }
  __syncthreads();
  const float sc = sc_sh[0], sh = sc_sh[1];
  for (int pp = threadIdx.x; pp < packs; pp += blockDim.x) {
    const int e = pp * V;
    const int n = e / S, s = e - n * S;
    const int64_t base = ((int64_t)n * C + c) * S + s;
    Pack<T, V> px = *reinterpret_cast<const Pack<T, V>*>(&x[base]);
    Pack<T, V> pr, py;
    if (RES) pr = *reinterpret_cast<const Pack<T, V>*>(&res[base]);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float z = to_f(px.v[k]) * sc + sh;
      if (RES) z += to_f(pr.v[k]);
      z = act_fwd<ACT>(z, slope);
      py.v[k] = from_f<T>(z);
    }
    *reinterpret_cast<Pack<T, V>*>(&y[base]) = py;
  }
}

template <typename T, int V, int ACT, bool RES, bool RESG>
__global__ void bn_bwd_fused_small_nchw(
    const T* __restrict__ dy, const T* __restrict__ x,
    const T* __restrict__ res, T* __restrict__ dx, T* __restrict__ dres,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ w, float* __restrict__ gw,
    float* __restrict__ gb, int N, int64_t C, int S, float slope) {
  const int64_t c = blockIdx.x;
  const int plane = N * S;
  const int packs = plane / V;
  const float m = mean[c];
  const float sc = ACT ? scale[c] : 0.f;
  const float sh = ACT ? shift[c] : 0.f;
  double a = 0.0, bb = 0.0;
  for (int pp = threadIdx.x; pp < packs; pp += blockDim.x) {
    const int e = pp * V;
    const int n = e / S, s = e - n * S;
    const int64_t base = ((int64_t)n * C + c) * S + s;
    Pack<T, V> pg = *reinterpret_cast<const Pack<T, V>*>(&dy[base]);
    Pack<T, V> px = *reinterpret_cast<const Pack<T, V>*>(&x[base]);
    Pack<T, V> pr;
    if (ACT && RES) pr = *reinterpret_cast<const Pack<T, V>*>(&res[base]);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float g = to_f(pg.v[k]);
      const float xv = to_f(px.v[k]);
      if (ACT) {
        float z = sc * xv + sh;
        if (RES) z += to_f(pr.v[k]);
        g = act_gate<ACT>(z, g, slope);
      }
      a += g;
      bb += (double)g * (xv - m);
    }
  }
  __shared__ double lds[2 * (MSBN_BLOCK / MSBN_WAVE)];
  block_reduce_pair(a, bb, lds);
  __shared__ float abd[3];
  if (threadIdx.x == 0) {
    const float istd = invstd[c];
    const float n_inv = 1.f / (float)plane;
    if (gw != nullptr) gw[c] = (float)(bb * istd);
    if (gb != nullptr) gb[c] = (float)a;
    const float f1 = istd * (w != nullptr ? w[c] : 1.f);
    const float f2 = (float)a * n_inv;
    const float f3 = istd * istd * (float)bb * n_inv;
    abd[0] = f1;
    abd[1] = -f1 * f3;
    abd[2] = f1 * (f3 * m - f2);
  }
  __syncthreads();
  const float A = abd[0], B = abd[1], D = abd[2];
  for (int pp = threadIdx.x; pp < packs; pp += blockDim.x) {
    const int e = pp * V;
    const int n = e / S, s = e - n * S;
    const int64_t base = ((int64_t)n * C + c) * S + s;
    Pack<T, V> pg = *reinterpret_cast<const Pack<T, V>*>(&dy[base]);
    Pack<T, V> px = *reinterpret_cast<const Pack<T, V>*>(&x[base]);
    Pack<T, V> pr, po, pq;
    if (ACT && RES) pr = *reinterpret_cast<const Pack<T, V>*>(&res[base]);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float g = to_f(pg.v[k]);
      const float xv = to_f(px.v[k]);
      if (ACT) {
        float z = sc * xv + sh;
        if (RES) z += to_f(pr.v[k]);
        g = act_gate<ACT>(z, g, slope);
      }
      po.v[k] = from_f<T>(A * g + B * xv + D);
      if (RESG) pq.v[k] = from_f<T>(g);
    }
    *reinterpret_cast<Pack<T, V>*>(&dx[base]) = po;
    if (RESG) *reinterpret_cast<Pack<T, V>*>(&dres[base]) = pq;
  }
}

// =====================================================================
// in-place activated BN (Rota Bulo et al., 2018): the forward writes
// y = act(scale*x + shift) OVER x, and the backward works from the stored y
// alone.  The activation must be invertible: identity (kActNone) or
// LeakyReLU with slope > 0 (kActLeaky), where sign(y) == sign(z):
//   gate            g = y > 0 ? dy : slope*dy
//   pre-activation  z = y > 0 ? y  : y*(1/slope)
//   x - mean        = (z - bias) * (1/scale)
// so {sum g, sum g*(x - mean)} mean what bn_bwd_reduce_partial_* emit (same
// fp64 workspace, same finalize, same all-reduce), and with
// x = (z - shift)/scale the usual dx = a*g + b*x + d is affine in (g, z):
//   dx = a*g + (b/scale)*z + (d - b*shift/scale).
// Needs scale != 0 in every channel (a zero scale gives 1/scale := 0: finite,
// but that channel's gradients are wrong).
// =====================================================================
template <int ACT>
__device__ __forceinline__ void inv_act(float yv, float& g, float& z,
                                        float slope, float inv_slope) {
  z = yv;
  if (ACT == kActLeaky) {
    const bool pos = yv > 0.f;
    g = pos ? g : slope * g;
    z = pos ? yv : yv * inv_slope;
  }
}

// packed [1/scale | bias] for the reduce-from-y kernels
template <typename WT>
__global__ void bn_inplace_aux(const float* __restrict__ invstd,
                               const WT* __restrict__ w,
                               const WT* __restrict__ b, int64_t C,
                               float* __restrict__ rscale,
                               float* __restrict__ bias_out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sc = invstd[c] * (w != nullptr ? to_f(w[c]) : 1.f);
  rscale[c] = sc != 0.f ? 1.f / sc : 0.f;
  bias_out[c] = b != nullptr ? to_f(b[c]) : 0.f;
}

// (a, b, d) of bn_affine_bwd -> the coefficients of dx in (g, z), in place:
//   b' = b/scale,  d' = d - b*shift/scale = -a*sum_dy/n - b'*bias
// (the second form has no mean in it, hence no cancellation off-centre).
template <typename WT>
__global__ void bn_inplace_bwd_coefs(const float* __restrict__ invstd,
                                     const WT* __restrict__ w,
                                     const WT* __restrict__ b,
                                     const float* __restrict__ sum_dy,
                                     const float* __restrict__ count,
                                     int64_t C,
                                     const float* __restrict__ coef_a,
                                     float* __restrict__ coef_b,
                                     float* __restrict__ coef_d) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float n = count[0];
  if (n <= 0.f) return;  // bn_affine_bwd wrote zeros
  const float sc = invstd[c] * (w != nullptr ? to_f(w[c]) : 1.f);
  const float rs = sc != 0.f ? 1.f / sc : 0.f;
  const float bz = coef_b[c] * rs;
  coef_b[c] = bz;
  coef_d[c] = -(coef_a[c] * (sum_dy[c] / n)) -
              bz * (b != nullptr ? to_f(b[c]) : 0.f);
}

// Alias-safe forward: ONE pointer, not __restrict__; every thread reads its
// pack and writes the same pack, so no element is read after another thread
// wrote it.  Arithmetic is bn_elemt_*'s, to the bit.
template <typename T, int V, int ACT>
__global__ void bn_elemt_inplace_nchw(T* xy, const float* __restrict__ scale,
                                      const float* __restrict__ shift,
                                      int64_t total, int64_t C, int64_t S,
                                      float slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const int64_t c = (e / S) % C;
    const float sc = scale[c], sh = shift[c];
    if (V == 1) {
      float z = to_f(nt_load1(&xy[e])) * sc + sh;
      z = act_fwd<ACT>(z, slope);
      nt_store1(&xy[e], from_f<T>(z));
    } else {
      Pack<T, V> px = nt_load<T, V>(&xy[e]);
      Pack<T, V> py;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float z = to_f(px.v[k]) * sc + sh;
        z = act_fwd<ACT>(z, slope);
        py.v[k] = from_f<T>(z);
      }
      nt_store<T, V>(&xy[e], py);
    }
  }
}

template <typename T, int V, int ACT>
__global__ void bn_elemt_inplace_nhwc(T* xy, const float* __restrict__ scale,
                                      const float* __restrict__ shift,
                                      int64_t total, int64_t C, float slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const int64_t c = e % C;
    if (V == 1) {
      float z = to_f(nt_load1(&xy[e])) * scale[c] + shift[c];
      z = act_fwd<ACT>(z, slope);
      nt_store1(&xy[e], from_f<T>(z));
    } else {
      Pack<T, V> px = nt_load<T, V>(&xy[e]);
      Pack<float, V> ps = *reinterpret_cast<const Pack<float, V>*>(&scale[c]);
      Pack<float, V> pb = *reinterpret_cast<const Pack<float, V>*>(&shift[c]);
      Pack<T, V> py;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float z = to_f(px.v[k]) * ps.v[k] + pb.v[k];
        z = act_fwd<ACT>(z, slope);
        py.v[k] = from_f<T>(z);
      }
      nt_store<T, V>(&xy[e], py);
    }
  }
}

// backward reduce partial from y: grids, chunking, AccPair flushes and the
// workspace layout are bn_bwd_reduce_partial_*'s.
template <typename T, int V, int ACT>
__global__ void bn_bwd_reduce_inplace_partial_nchw(
    const T* __restrict__ dy, const T* __restrict__ y,
    const float* __restrict__ rscale, const float* __restrict__ bias,
    double* __restrict__ ws, int64_t N, int64_t C, int64_t S, int64_t chunkN,
    int64_t chunkS, float slope, float inv_slope) {
  const int64_t c = blockIdx.x;
  const float rs = rscale[c], bi = bias[c];
  const int64_t n0 = blockIdx.y * chunkN;
  const int64_t n1 = i64min(n0 + chunkN, N);
  const int64_t s0 = blockIdx.z * chunkS;
  const int64_t s1 = i64min(s0 + chunkS, S);
  AccPair acc;
  int since_flush = 0;
  for (int64_t n = n0; n < n1; ++n) {
    const int64_t base = (n * C + c) * S;
    if (V == 1) {
      for (int64_t s = s0 + threadIdx.x; s < s1; s += blockDim.x) {
        float g = to_f(nt_load1(&dy[base + s])), z;
        inv_act<ACT>(to_f(nt_load1(&y[base + s])), g, z, slope, inv_slope);
        acc.add2(g, g * ((z - bi) * rs));
        if (++since_flush == MSBN_ACC_FLUSH) {
          acc.flush();
          since_flush = 0;
        }
      }
    } else {
      for (int64_t s = s0 + (int64_t)threadIdx.x * V; s < s1;
           s += (int64_t)blockDim.x * V) {
        Pack<T, V> pg = nt_load<T, V>(&dy[base + s]);
        Pack<T, V> py = nt_load<T, V>(&y[base + s]);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          float g = to_f(pg.v[k]), z;
          inv_act<ACT>(to_f(py.v[k]), g, z, slope, inv_slope);
          acc.add2(g, g * ((z - bi) * rs));
        }
        if (++since_flush == MSBN_ACC_FLUSH / V) {
          acc.flush();
          since_flush = 0;
        }
      }
    }
  }
  acc.flush();
  double a = acc.a, b = acc.b;
  __shared__ double lds[2 * (MSBN_BLOCK / MSBN_WAVE)];
  block_reduce_pair(a, b, lds);
  if (threadIdx.x == 0) {
    const int64_t chunk = (int64_t)blockIdx.y * gridDim.z + blockIdx.z;
    double* out = ws + (c * gridDim.y * gridDim.z + chunk) * 2;
    out[0] = a;
    out[1] = b;
  }
}

template <typename T, int ACT>
__global__ void bn_bwd_reduce_inplace_partial_nchw_flat(
    const T* __restrict__ dy, const T* __restrict__ y,
    const float* __restrict__ rscale, const float* __restrict__ bias,
    double* __restrict__ ws, int64_t N, int64_t C, int64_t S,
    int64_t chunk_len, float slope, float inv_slope) {
  const int64_t c = blockIdx.x;
  const float rs = rscale[c], bi = bias[c];
  const int64_t NS = N * S;
  const int64_t p0 = (int64_t)blockIdx.y * chunk_len;
  const int64_t p1 = i64min(p0 + chunk_len, NS);
  AccPair acc;
  int since_flush = 0;
  for (int64_t p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
    const int64_t n = p / S, s = p - n * S;
    const int64_t e = (n * C + c) * S + s;
    float g = to_f(nt_load1(&dy[e])), z;
    inv_act<ACT>(to_f(nt_load1(&y[e])), g, z, slope, inv_slope);
    acc.add2(g, g * ((z - bi) * rs));
    if (++since_flush == MSBN_ACC_FLUSH) {
      acc.flush();
      since_flush = 0;
    }
  }
  acc.flush();
  double a = acc.a, b = acc.b;
  __shared__ double lds[2 * (MSBN_BLOCK / MSBN_WAVE)];
  block_reduce_pair(a, b, lds);
  if (threadIdx.x == 0) {
    double* out = ws + (c * gridDim.y + blockIdx.y) * 2;
    out[0] = a;
    out[1] = b;
  }
}

template <typename T, int V, int ACT>
__global__ void bn_bwd_reduce_inplace_partial_nhwc(
    const T* __restrict__ dy, const T* __restrict__ y,
    const float* __restrict__ rscale, const float* __restrict__ bias,
    double* __restrict__ ws, int64_t rows, int64_t C, int64_t chunk_rows,
    int lpr, float slope, float inv_slope) {
  const int rpi = blockDim.x / lpr;
  const int lane = threadIdx.x % lpr;
  const int rowoff = threadIdx.x / lpr;
  const bool active = rowoff < rpi;
  const int64_t c = (int64_t)blockIdx.x * lpr * V + (int64_t)lane * V;
  const bool inb = active && (c + V <= C);

  AccPair acc[V];
  if (inb) {
    float rs[V], bi[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      rs[k] = rscale[c + k];
      bi[k] = bias[c + k];
    }
    const int64_t r0 = (int64_t)blockIdx.y * chunk_rows;
    const int64_t r1 = i64min(r0 + chunk_rows, rows);
    int since_flush = 0;
    for (int64_t r = r0 + rowoff; r < r1; r += rpi) {
      Pack<T, V> pg = nt_load<T, V>(&dy[r * C + c]);
      Pack<T, V> py = nt_load<T, V>(&y[r * C + c]);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float g = to_f(pg.v[k]), z;
        inv_act<ACT>(to_f(py.v[k]), g, z, slope, inv_slope);
        acc[k].add2(g, g * ((z - bi[k]) * rs[k]));
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
  // LDS layout and tree as in bn_bwd_reduce_partial_nhwc
  __shared__ double sdata[MSBN_BLOCK * V * 2];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    sdata[k * MSBN_BLOCK + threadIdx.x] = a[k];
    sdata[(V + k) * MSBN_BLOCK + threadIdx.x] = b[k];
  }
  for (int st = 1; st < rpi; st <<= 1) {
    __syncthreads();
    if (active && (rowoff & ((st << 1) - 1)) == 0 && rowoff + st < rpi) {
      const int other = threadIdx.x + st * lpr;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        sdata[k * MSBN_BLOCK + threadIdx.x] += sdata[k * MSBN_BLOCK + other];
        sdata[(V + k) * MSBN_BLOCK + threadIdx.x] +=
            sdata[(V + k) * MSBN_BLOCK + other];
      }
    }
  }
  __syncthreads();
  if (rowoff == 0 && c < C) {
    const int64_t chunk = blockIdx.y;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (c + k < C) {
        double* out = ws + ((c + k) * gridDim.y + chunk) * 2;
        out[0] = sdata[k * MSBN_BLOCK + threadIdx.x];
        out[1] = sdata[(V + k) * MSBN_BLOCK + threadIdx.x];
      }
    }
  }
}

// backward elementwise from y: dx = a[c]*g + bz[c]*z + dz[c], gate and
// pre-activation recovered from y (inv_act); cb / cd hold bz / dz
// (bn_inplace_bwd_coefs).
template <typename T, int V, int ACT>
__global__ void bn_bwd_elemt_inplace_nchw(const T* __restrict__ dy,
                                          const T* __restrict__ y,
                                          T* __restrict__ dx,
                                          const float* __restrict__ ca,
                                          const float* __restrict__ cb,
                                          const float* __restrict__ cd,
                                          int64_t total, int64_t C, int64_t S,
                                          float slope, float inv_slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const int64_t c = (e / S) % C;
    const float A = ca[c], B = cb[c], D = cd[c];
    if (V == 1) {
      float g = to_f(nt_load1(&dy[e])), z;
      inv_act<ACT>(to_f(nt_load1(&y[e])), g, z, slope, inv_slope);
      nt_store1(&dx[e], from_f<T>(A * g + B * z + D));
    } else {
      Pack<T, V> pg = nt_load<T, V>(&dy[e]);
      Pack<T, V> py = nt_load<T, V>(&y[e]);
      Pack<T, V> po;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float g = to_f(pg.v[k]), z;
        inv_act<ACT>(to_f(py.v[k]), g, z, slope, inv_slope);
        po.v[k] = from_f<T>(A * g + B * z + D);
      }
      nt_store<T, V>(&dx[e], po);
    }
  }
}

template <typename T, int V, int ACT>
__global__ void bn_bwd_elemt_inplace_nhwc(const T* __restrict__ dy,
                                          const T* __restrict__ y,
                                          T* __restrict__ dx,
                                          const float* __restrict__ ca,
                                          const float* __restrict__ cb,
                                          const float* __restrict__ cd,
                                          int64_t total, int64_t C,
                                          float slope, float inv_slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const int64_t c = e % C;
    if (V == 1) {
      float g = to_f(nt_load1(&dy[e])), z;
      inv_act<ACT>(to_f(nt_load1(&y[e])), g, z, slope, inv_slope);
      nt_store1(&dx[e], from_f<T>(ca[c] * g + cb[c] * z + cd[c]));
    } else {
      Pack<T, V> pg = nt_load<T, V>(&dy[e]);
      Pack<T, V> py = nt_load<T, V>(&y[e]);
      Pack<float, V> pa = *reinterpret_cast<const Pack<float, V>*>(&ca[c]);
      Pack<float, V> pb = *reinterpret_cast<const Pack<float, V>*>(&cb[c]);
      Pack<float, V> pd = *reinterpret_cast<const Pack<float, V>*>(&cd[c]);
      Pack<T, V> po;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float g = to_f(pg.v[k]), z;
        inv_act<ACT>(to_f(py.v[k]), g, z, slope, inv_slope);
        po.v[k] = from_f<T>(pa.v[k] * g + pb.v[k] * z + pd.v[k]);
      }
      nt_store<T, V>(&dx[e], po);
    }
  }
}

// =====================================================================
// stem pool fusion: bn + act + MaxPool2d(3, 2, 1) without the full-size
// activation (docs/KERNEL_DESIGN.md "Stem pool fusion").  Channels-last only.
//
// Forward: one thread per pooled (n, oh, ow, channel pack) forms
// y = from_f<T>(act(scale*x + shift)) for the up to nine x packs of its
// window (rows / columns outside the image are skipped, not read as zero),
// takes the maximum over the T-ROUNDED y with the stock rule
// `val > max || isnan(val)` scanning kh then kw ascending (first maximum
// wins), and stores the pooled pack plus one byte per element, the window
// code kh*3 + kw.  y itself is never written.
//
// Backward: the full-size gradient the stock pool backward would have stored
// is re-formed per x element by a gather (pool_gather): an element lies in
// 1, 2 or 4 windows (even h / w: one window row / column, odd: two); each
// candidate window in ascending (oh, ow) order whose code names this element
// adds its pooled gradient in fp32, and the sum is rounded to T once -- what
// max_pool_backward_nhwc<T, float> stored.  With DY2 a window's gradient is
// fork_grad(dy, dy2), the eager add's result.  The reduce kernel keeps
// bn_bwd_reduce_partial_nhwc's traversal of x's rows, accumulators, flush
// period, LDS tree and workspace layout, so its sums are that kernel's sums
// bit for bit; the elementwise kernel gathers again rather than paying a gm
// round trip (0.6A of mostly cached reads against 2A).
// =====================================================================
// Window / gather reads are shared by neighbouring threads (a pooled window
// overlaps its neighbours; a pooled gradient is wanted by up to nine x
// elements).  nt loads skip L1 and are served from L2, plain loads may hit
// L1.  Measured both ways (profiles/r07_stem_pool.md): plain loads are the
// faster ones for the forward's window reads and, once the second window
// column is only read where it exists, for the backward's gather reads.
// The streamed tensors (x in the backward kernels, every store) stay nt.
#ifndef MSBN_POOL_FWD_NT
#define MSBN_POOL_FWD_NT 0
#endif
#ifndef MSBN_POOL_GATHER_NT
#define MSBN_POOL_GATHER_NT 0
#endif

template <typename T, int V, bool NT>
__device__ __forceinline__ Pack<T, V> pool_load(const T* p) {
  if (NT) return nt_load<T, V>(p);
  return *reinterpret_cast<const Pack<T, V>*>(p);
}

template <typename T, int V, int ACT>
__global__ void bn_elemt_pool_nhwc(const T* __restrict__ x,
                                   T* __restrict__ y,
                                   uint8_t* __restrict__ codes,
                                   const float* __restrict__ scale,
                                   const float* __restrict__ shift,
                                   int64_t total, int64_t C, int H, int W,
                                   int OH, int OW, float slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const uint32_t pix = (uint32_t)(e / C);
    const int64_t c = e - (int64_t)pix * C;
    const uint32_t t = pix / (uint32_t)OW;
    const int ow = (int)(pix - t * (uint32_t)OW);
    const int n = (int)(t / (uint32_t)OH);
    const int oh = (int)(t - (uint32_t)n * (uint32_t)OH);
    const int h0 = 2 * oh - 1, w0 = 2 * ow - 1;
    Pack<float, V> ps, pb;
    if (V == 1) {
      ps.v[0] = scale[c];
      pb.v[0] = shift[c];
    } else {
      ps = *reinterpret_cast<const Pack<float, V>*>(&scale[c]);
      pb = *reinterpret_cast<const Pack<float, V>*>(&shift[c]);
    }
    float best[V];
    uint8_t code[V];
    // first window position inside the image: what an all -inf window keeps
    const uint8_t first = (uint8_t)((h0 < 0 ? 3 : 0) + (w0 < 0 ? 1 : 0));
#pragma unroll
    for (int k = 0; k < V; ++k) {
      best[k] = -INFINITY;
      code[k] = first;
    }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int h = h0 + kh;
      if (h < 0 || h >= H) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int w = w0 + kw;
        if (w < 0 || w >= W) continue;
        const int64_t off = (((int64_t)n * H + h) * W + w) * C + c;
        const Pack<T, V> px = pool_load<T, V, MSBN_POOL_FWD_NT>(&x[off]);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          float z = to_f(px.v[k]) * ps.v[k] + pb.v[k];
          z = act_fwd<ACT>(z, slope);
          const float val = to_f(from_f<T>(z));
          if (val > best[k] || val != val) {
            best[k] = val;
            code[k] = (uint8_t)(kh * 3 + kw);
          }
        }
      }
    }
    Pack<T, V> py;
    Pack<uint8_t, V> pc;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      py.v[k] = from_f<T>(best[k]);
      pc.v[k] = code[k];
    }
    nt_store<T, V>(&y[e], py);
    nt_store<uint8_t, V>(&codes[e], pc);
  }
}

// The stock pool backward's gradient at x element (n, h, w, c..c+V), in fp32
// after its one rounding to T.
template <typename T, int V, bool DY2>
__device__ __forceinline__ void pool_gather(const T* __restrict__ dy,
                                            const T* __restrict__ dy2,
                                            const uint8_t* __restrict__ codes,
                                            int n, int h, int w, int64_t c,
                                            int64_t C, int OH, int OW,
                                            float (&g)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) g[k] = 0.f;
  const int oh0 = h >> 1, ow0 = w >> 1;
  // the window row loop branches (h is all but uniform across a wave); the
  // second window column is read only by the odd-w lanes that lie in it and
  // carries a code no window stores everywhere else
  const int noh = ((h & 1) && oh0 + 1 < OH) ? 2 : 1;
  const bool two_w = (w & 1) && ow0 + 1 < OW;
  const int ow1 = two_w ? ow0 + 1 : ow0;
  const int kw0 = w - (2 * ow0 - 1);
  for (int a = 0; a < noh; ++a) {
    const int oh = oh0 + a;
    const int kh3 = (h - (2 * oh - 1)) * 3;
    const uint8_t want0 = (uint8_t)(kh3 + kw0);
    const uint8_t want1 = two_w ? (uint8_t)kh3 : (uint8_t)0xff;  // kw = 0
    const int64_t row = ((int64_t)n * OH + oh) * OW;
    const int64_t off0 = (row + ow0) * C + c;
    const int64_t off1 = (row + ow1) * C + c;
    constexpr bool GNT = MSBN_POOL_GATHER_NT;
    const Pack<uint8_t, V> pc0 = pool_load<uint8_t, V, GNT>(&codes[off0]);
    const Pack<T, V> pg0 = pool_load<T, V, GNT>(&dy[off0]);
    Pack<T, V> ph0, ph1;
    if (DY2) ph0 = pool_load<T, V, GNT>(&dy2[off0]);
    Pack<uint8_t, V> pc1;
    Pack<T, V> pg1;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      pc1.v[k] = 0xff;
      pg1.v[k] = from_f<T>(0.f);
      if (DY2) ph1.v[k] = from_f<T>(0.f);
    }
    if (two_w) {
      pc1 = pool_load<uint8_t, V, GNT>(&codes[off1]);
      pg1 = pool_load<T, V, GNT>(&dy[off1]);
      if (DY2) ph1 = pool_load<T, V, GNT>(&dy2[off1]);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float g0 = DY2 ? fork_grad(pg0.v[k], ph0.v[k]) : to_f(pg0.v[k]);
      const float g1 = DY2 ? fork_grad(pg1.v[k], ph1.v[k]) : to_f(pg1.v[k]);
      if (pc0.v[k] == want0) g[k] += g0;
      if (pc1.v[k] == want1) g[k] += g1;
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) g[k] = to_f(from_f<T>(g[k]));
}

// bn_bwd_reduce_partial_nhwc<T, V, ACT, false, false, false> over x's rows
// with the dy load replaced by pool_gather.
template <typename T, int V, int ACT, bool DY2>
__global__ void bn_bwd_reduce_pool_partial_nhwc(
    const T* __restrict__ dy, const T* __restrict__ dy2,
    const uint8_t* __restrict__ codes, const T* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ scale,
    const float* __restrict__ shift, double* __restrict__ ws, int64_t rows,
    int64_t C, int64_t chunk_rows, int lpr, int H, int W, int OH, int OW,
    float slope) {
  const int rpi = blockDim.x / lpr;
  const int lane = threadIdx.x % lpr;
  const int rowoff = threadIdx.x / lpr;
  const bool active = rowoff < rpi;
  const int64_t c = (int64_t)blockIdx.x * lpr * V + (int64_t)lane * V;
  const bool inb = active && (c + V <= C);

  AccPair acc[V];
  float m[V], scv[V], shv[V];
#pragma unroll
  for (int k = 0; k < V; ++k) m[k] = scv[k] = shv[k] = 0.f;
  if (inb) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      m[k] = mean[c + k];
      if (ACT) {
        scv[k] = scale[c + k];
        shv[k] = shift[c + k];
      }
    }
    const int64_t r0 = (int64_t)blockIdx.y * chunk_rows;
    const int64_t r1 = i64min(r0 + chunk_rows, rows);
    // (n, h, w) of row r, stepped along with r (rows < 2^31, host-checked)
    int n = 0, h = 0, w = 0;
    if (r0 + rowoff < r1) {
      const uint32_t r = (uint32_t)(r0 + rowoff);
      const uint32_t t = r / (uint32_t)W;
      w = (int)(r - t * (uint32_t)W);
      n = (int)(t / (uint32_t)H);
      h = (int)(t - (uint32_t)n * (uint32_t)H);
    }
    int since_flush = 0;
    for (int64_t r = r0 + rowoff; r < r1; r += rpi) {
      float g[V];
      pool_gather<T, V, DY2>(dy, dy2, codes, n, h, w, c, C, OH, OW, g);
      Pack<T, V> px = nt_load<T, V>(&x[r * C + c]);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float xv = to_f(px.v[k]);
        if (ACT) {
          float z = scv[k] * xv + shv[k];
          g[k] = act_gate<ACT>(z, g[k], slope);
        }
        acc[k].add2(g[k], g[k] * (xv - m[k]));
      }
      if (++since_flush == MSBN_ACC_FLUSH) {
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k].flush();
        since_flush = 0;
      }
      w += rpi;
      while (w >= W) {
        w -= W;
        if (++h == H) {
          h = 0;
          ++n;
        }
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
  // LDS tree and workspace layout of bn_bwd_reduce_partial_nhwc
  __shared__ double sdata[MSBN_BLOCK * V * 2];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    sdata[k * MSBN_BLOCK + threadIdx.x] = a[k];
    sdata[(V + k) * MSBN_BLOCK + threadIdx.x] = b[k];
  }
  for (int st = 1; st < rpi; st <<= 1) {
    __syncthreads();
    if (active && (rowoff & ((st << 1) - 1)) == 0 && rowoff + st < rpi) {
      const int other = threadIdx.x + st * lpr;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        sdata[k * MSBN_BLOCK + threadIdx.x] += sdata[k * MSBN_BLOCK + other];
        sdata[(V + k) * MSBN_BLOCK + threadIdx.x] +=
            sdata[(V + k) * MSBN_BLOCK + other];
      }
    }
  }
  __syncthreads();
  if (rowoff == 0 && c < C) {
    const int64_t chunk = blockIdx.y;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (c + k < C) {
        double* out = ws + ((c + k) * gridDim.y + chunk) * 2;
        out[0] = sdata[k * MSBN_BLOCK + threadIdx.x];
        out[1] = sdata[(V + k) * MSBN_BLOCK + threadIdx.x];
      }
    }
  }
}

// bn_bwd_elemt_nhwc<T, V, ACT, false, false> with the dy load replaced by
// pool_gather: reads x, the pooled gradient(s) and the codes, writes dx.
template <typename T, int V, int ACT, bool DY2>
__global__ void bn_bwd_elemt_pool_nhwc(
    const T* __restrict__ dy, const T* __restrict__ dy2,
    const uint8_t* __restrict__ codes, const T* __restrict__ x,
    T* __restrict__ dx, const float* __restrict__ ca,
    const float* __restrict__ cb, const float* __restrict__ cd,
    const float* __restrict__ scale, const float* __restrict__ shift,
    int64_t total, int64_t C, int H, int W, int OH, int OW, float slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i * V < total; i += stride) {
    const int64_t e = i * V;
    const uint32_t pix = (uint32_t)(e / C);
    const int64_t c = e - (int64_t)pix * C;
    const uint32_t t = pix / (uint32_t)W;
    const int w = (int)(pix - t * (uint32_t)W);
    const int n = (int)(t / (uint32_t)H);
    const int h = (int)(t - (uint32_t)n * (uint32_t)H);
    float g[V];
    pool_gather<T, V, DY2>(dy, dy2, codes, n, h, w, c, C, OH, OW, g);
    if (V == 1) {
      const float xv = to_f(nt_load1(&x[e]));
      float gv = g[0];
      if (ACT) {
        float z = scale[c] * xv + shift[c];
        gv = act_gate<ACT>(z, gv, slope);
      }
      nt_store1(&dx[e], from_f<T>(ca[c] * gv + cb[c] * xv + cd[c]));
    } else {
      Pack<T, V> px = nt_load<T, V>(&x[e]);
      Pack<float, V> pa = *reinterpret_cast<const Pack<float, V>*>(&ca[c]);
      Pack<float, V> pb = *reinterpret_cast<const Pack<float, V>*>(&cb[c]);
      Pack<float, V> pd = *reinterpret_cast<const Pack<float, V>*>(&cd[c]);
      Pack<float, V> psc, psh;
      if (ACT) {
        psc = *reinterpret_cast<const Pack<float, V>*>(&scale[c]);
        psh = *reinterpret_cast<const Pack<float, V>*>(&shift[c]);
      }
      Pack<T, V> po;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float gv = g[k];
        const float xv = to_f(px.v[k]);
        if (ACT) {
          float z = psc.v[k] * xv + psh.v[k];
          gv = act_gate<ACT>(z, gv, slope);
        }
        po.v[k] = from_f<T>(pa.v[k] * gv + pb.v[k] * xv + pd.v[k]);
      }
      nt_store<T, V>(&dx[e], po);
    }
  }
}

// =====================================================================
// host-side helpers
// =====================================================================

struct Layout {
  bool nhwc;       // channels-last (rows x C contiguous)
  int64_t N, C, S; // NCHW view (S = spatial)
  int64_t rows;    // NHWC view (= N*S)
};

Layout get_layout(const at::Tensor& t) {
  Layout L{};
  L.C = t.size(1);
  L.N = t.size(0);
  L.S = t.numel() / std::max<int64_t>(L.N * L.C, 1);
  L.rows = L.N * L.S;
  const auto fmt = t.suggest_memory_format();
  if ((fmt == at::MemoryFormat::ChannelsLast && t.dim() == 4 &&
       t.is_contiguous(at::MemoryFormat::ChannelsLast)) ||
      (fmt == at::MemoryFormat::ChannelsLast3d && t.dim() == 5 &&
       t.is_contiguous(at::MemoryFormat::ChannelsLast3d))) {
    L.nhwc = true;
  } else {
    TORCH_CHECK(t.is_contiguous(), "msbn: input must be contiguous (NCHW) or "
                                   "channels-last");
    L.nhwc = false;
  }
  return L;
}

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t clamp64(int64_t v, int64_t lo, int64_t hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// channels per finalize block (one wave each)
constexpr int kFinalizeWavesPerBlock = MSBN_BLOCK / MSBN_WAVE;

struct FlatGrid {
  dim3 grid;
  int64_t chunk_len;
  int nchunks;
};

// grid for the V==1 flat NCHW partial kernels: (C, nchunks)
FlatGrid flat_grid(int64_t C, int64_t NS, int64_t target_blocks) {
  FlatGrid g{};
  int64_t nchunks =
      clamp64(target_blocks / std::max<int64_t>(C, 1), 1, cdiv(NS, 1024));
  g.chunk_len = cdiv(NS, nchunks);
  nchunks = cdiv(NS, g.chunk_len);
  g.grid = dim3((unsigned)C, (unsigned)nchunks);
  g.nchunks = (int)nchunks;
  return g;
}

// pick vector width: 16B/lane when layout & alignment allow
// `ptrs` is EVERY tensor pointer the launch dereferences with V-wide packs
// (absent ones nullptr); esize the element size in bytes.
int pick_v(int esize, c10::ArrayRef<const void*> ptrs, int64_t inner) {
  const int vmax = 16 / esize;
  auto ok = [&](int v) {
    const size_t bytes = (size_t)v * esize;
    if (inner % v != 0) return false;
    for (const void* p : ptrs)
      if (p != nullptr && ((uintptr_t)p % bytes) != 0) return false;
    return true;
  };
  if (ok(vmax)) return vmax;
  if (vmax >= 4 && ok(vmax / 2)) return vmax / 2;
  return 1;
}

constexpr int kTargetBlocks = 2048;  // 256 CUs x 8 blocks (guide G11)

struct NchwGrid {
  dim3 grid;
  int64_t chunkN, chunkS;
  int nchunks;
};

NchwGrid nchw_grid(int64_t N, int64_t C, int64_t S, int V) {
  NchwGrid g{};
  const int64_t perC = std::max<int64_t>(1, kTargetBlocks / std::max<int64_t>(C, 1));
  int64_t nchunkN = std::min<int64_t>(N, perC);
  nchunkN = std::max<int64_t>(nchunkN, 1);
  g.chunkN = cdiv(N, nchunkN);
  nchunkN = cdiv(N, g.chunkN);
  int64_t want_s = cdiv(perC, nchunkN);
  // each S-chunk should be a multiple of V and >= ~4096 elements of work
  int64_t max_s = cdiv(S, std::max<int64_t>((int64_t)MSBN_BLOCK * V, 1024));
  int64_t nchunkS = std::max<int64_t>(1, std::min(want_s, std::max<int64_t>(max_s, 1)));
  g.chunkS = cdiv(cdiv(S, nchunkS), V) * V;
  nchunkS = cdiv(S, g.chunkS);
  g.grid = dim3((unsigned)C, (unsigned)nchunkN, (unsigned)nchunkS);
  g.nchunks = (int)(nchunkN * nchunkS);
  return g;
}

struct NhwcGrid {
  dim3 grid;
  int64_t chunk_rows;
  int nchunks;
  int lpr;
};

NhwcGrid nhwc_grid(int64_t rows, int64_t C, int V) {
  NhwcGrid g{};
  const int64_t cv = cdiv(C, V);
  // Workspace traffic is C * nchunks * 16 B, written by the partial kernel
  // and read back by finalize.  The old lpr = min(cv, 256) choice made
  // ctiles = 1 for C >= 2048 (bf16), forcing nchunks ~ kTargetBlocks and a
  // workspace up to HALF the payload (measured 1.4 TB/s effective at
  // 512x2048x7x7 vs 6.3 TB/s ceiling).  Tile CHANNELS instead: pick lpr so
  // ~16 channel tiles exist, which caps nchunks near kTargetBlocks/16 and
  // keeps the workspace at a few % of the payload.  Lower bound lpr at 8
  // lanes so each row segment stays >= 128 B (one full memory granule).
  int64_t lpr = cdiv(cv, 16);
  // round up to a power of two that divides the block
  int64_t p2 = 8;
  while (p2 < lpr) p2 <<= 1;
  lpr = std::min<int64_t>(std::max<int64_t>(p2, 8), MSBN_BLOCK);
  lpr = std::min(lpr, [&] {  // never exceed what C needs
    int64_t q = 8;
    while (q < cv) q <<= 1;
    return std::min<int64_t>(q, MSBN_BLOCK);
  }());
  g.lpr = (int)lpr;
  const int64_t ctiles = cdiv(C, lpr * V);
  const int64_t per_tile =
      std::max<int64_t>(1, kTargetBlocks / std::max<int64_t>(ctiles, 1));
  const int rpi = MSBN_BLOCK / g.lpr;
  int64_t max_chunks = cdiv(rows, std::max<int64_t>(4 * rpi, 16));
  int64_t nchunks = std::max<int64_t>(1, std::min(per_tile, std::max<int64_t>(max_chunks, 1)));
  g.chunk_rows = cdiv(rows, nchunks);
  nchunks = cdiv(rows, g.chunk_rows);
  g.grid = dim3((unsigned)ctiles, (unsigned)nchunks);
  g.nchunks = (int)nchunks;
  return g;
}

int elemt_grid(int64_t total, int V) {
  return (int)std::min<int64_t>(cdiv(total, (int64_t)MSBN_BLOCK * V),
                                2 * kTargetBlocks);
}

// ---- launch plans -----------------------------------------------------
// The one place a launch's vector width and grid are decided: the ops below
// launch from these, and launch_plan() reports them to tests (so a test can
// prove which loop trips / branches its shape reaches).
enum class RedPath { NchwVec, NchwFlat, Nhwc };

struct ReducePlan {
  RedPath path;
  int v;
  int nchunks;        // partials per channel handed to the finalize kernel
  NchwGrid nchw;      // path == NchwVec
  FlatGrid flat;      // path == NchwFlat
  NhwcGrid nhwc;      // path == Nhwc
  int64_t trips;      // most iterations any thread's accumulation loop makes
  int flush_every;    // iterations between two AccPair flushes
};

ReducePlan plan_reduce(const Layout& L, int esize,
                       c10::ArrayRef<const void*> ptrs) {
  ReducePlan p{};
  if (!L.nhwc) {
    p.v = pick_v(esize, ptrs, L.S);
    if (p.v == 1) {
      p.path = RedPath::NchwFlat;
      p.flat = flat_grid(L.C, L.rows, kTargetBlocks);
      p.nchunks = p.flat.nchunks;
      p.trips = cdiv(p.flat.chunk_len, MSBN_BLOCK);
      p.flush_every = MSBN_ACC_FLUSH;
    } else {
      p.path = RedPath::NchwVec;
      p.nchw = nchw_grid(L.N, L.C, L.S, p.v);
      p.nchunks = p.nchw.nchunks;
      p.trips = p.nchw.chunkN *
                cdiv(std::min(p.nchw.chunkS, L.S), (int64_t)MSBN_BLOCK * p.v);
      p.flush_every = MSBN_ACC_FLUSH / p.v;
    }
  } else {
    p.path = RedPath::Nhwc;
    p.v = pick_v(esize, ptrs, L.C);
    p.nhwc = nhwc_grid(L.rows, L.C, p.v);
    p.nchunks = p.nhwc.nchunks;
    p.trips = cdiv(p.nhwc.chunk_rows, MSBN_BLOCK / p.nhwc.lpr);
    p.flush_every = MSBN_ACC_FLUSH;
  }
  return p;
}

struct ElemtPlan {
  int v;
  int grid;
  int64_t packs;  // V-wide packs in the tensor; one thread-trip handles one
};

// `coef` is the caller-visible per-channel fp32 buffer ([scale | shift]) the
// NHWC kernels load V floats at a time; nullptr when none is read.
ElemtPlan plan_elemt(const Layout& L, int64_t total, int esize,
                     c10::ArrayRef<const void*> ptrs, const float* coef) {
  ElemtPlan p{};
  p.v = pick_v(esize, ptrs, L.nhwc ? L.C : L.S);
  if (L.nhwc && coef != nullptr &&
      ((uintptr_t)coef % ((size_t)p.v * sizeof(float))) != 0)
    p.v = 1;
  p.grid = elemt_grid(total, p.v);
  p.packs = cdiv(total, p.v);
  return p;
}

#define MSBN_DISPATCH_FLOAT_TYPES(TYPE, NAME, ...)                          \
  [&] {                                                                     \
    switch (TYPE) {                                                         \
      case at::kFloat: {                                                    \
        using scalar_t = float;                                             \
        using native_t = float;                                             \
        return __VA_ARGS__();                                               \
      }                                                                     \
      case at::kBFloat16: {                                                 \
        using scalar_t = at::BFloat16;                                      \
        using native_t = __hip_bfloat16;                                    \
        return __VA_ARGS__();                                               \
      }                                                                     \
      case at::kHalf: {                                                     \
        using scalar_t = at::Half;                                          \
        using native_t = __half;                                            \
        return __VA_ARGS__();                                               \
      }                                                                     \
      default:                                                              \
        TORCH_CHECK(false, NAME, ": unsupported dtype ", TYPE);             \
    }                                                                       \
  }()

#define MSBN_DISPATCH_V(VSEL, VMAX, ...)                                    \
  [&] {                                                                     \
    if constexpr (VMAX == 8) {                                              \
      switch (VSEL) {                                                       \
        case 8: {                                                           \
          constexpr int VV = 8;                                             \
          return __VA_ARGS__();                                             \
        }                                                                   \
        case 4: {                                                           \
          constexpr int VV = 4;                                             \
          return __VA_ARGS__();                                             \
        }                                                                   \
        default: {                                                          \
          constexpr int VV = 1;                                             \
          return __VA_ARGS__();                                             \
        }                                                                   \
      }                                                                     \
    } else {                                                                \
      switch (VSEL) {                                                       \
        case 4: {                                                           \
          constexpr int VV = 4;                                             \
          return __VA_ARGS__();                                             \
        }                                                                   \
        case 2: {                                                           \
          constexpr int VV = 2;                                             \
          return __VA_ARGS__();                                             \
        }                                                                   \
        default: {                                                          \
          constexpr int VV = 1;                                             \
          return __VA_ARGS__();                                             \
        }                                                                   \
      }                                                                     \
    }                                                                       \
  }()

#define MSBN_DISPATCH_RSTAT(TYPE, NAME, ...)                                \
  [&] {                                                                     \
    switch (TYPE) {                                                         \
      case at::kFloat: {                                                    \
        using rstat_t = float;                                              \
        return __VA_ARGS__();                                               \
      }                                                                     \
      case at::kBFloat16: {                                                 \
        using rstat_t = __hip_bfloat16;                                     \
        return __VA_ARGS__();                                               \
      }                                                                     \
      case at::kHalf: {                                                     \
        using rstat_t = __half;                                             \
        return __VA_ARGS__();                                               \
      }                                                                     \
      default:                                                              \
        TORCH_CHECK(false, NAME, ": unsupported running-stat dtype ", TYPE); \
    }                                                                       \
  }()

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// Launch the two-stage stats reduction; writes mean/invstd/count into the
// given fp32 pointers (which may alias a packed buffer).
#define MSBN_DISPATCH_WTYPE(TYPE, NAME, ...)                                \
  [&] {                                                                     \
    switch (TYPE) {                                                         \
      case at::kFloat: {                                                    \
        using wt_t = float;                                                 \
        return __VA_ARGS__();                                               \
      }                                                                     \
      case at::kBFloat16: {                                                 \
        using wt_t = __hip_bfloat16;                                        \
        return __VA_ARGS__();                                               \
      }                                                                     \
      case at::kHalf: {                                                     \
        using wt_t = __half;                                                \
        return __VA_ARGS__();                                               \
      }                                                                     \
      default:                                                              \
        TORCH_CHECK(false, NAME, ": unsupported weight dtype ", TYPE);      \
    }                                                                       \
  }()

void stats_into(const at::Tensor& input, double eps, float* mean_p,
                float* invstd_p, float* count_p, const at::Tensor* rmean,
                const at::Tensor* rvar, double momentum,
                const at::Tensor* wpar = nullptr,
                const at::Tensor* bpar = nullptr, float* scale_p = nullptr,
                float* shift_p = nullptr) {
  const Layout L = get_layout(input);
  const int64_t count = L.rows;
  auto stream = cur_stream();
  const auto rstat_type = rmean ? rmean->scalar_type() : at::kFloat;
  const auto w_type = wpar ? wpar->scalar_type()
                     : bpar ? bpar->scalar_type()
                            : at::kFloat;

  MSBN_DISPATCH_FLOAT_TYPES(input.scalar_type(), "batch_norm_stats", [&] {
    const native_t* x =
        reinterpret_cast<const native_t*>(input.data_ptr<scalar_t>());
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    const ReducePlan plan = plan_reduce(L, (int)sizeof(native_t), {x});
    const int v = plan.v;
    const int nchunks = plan.nchunks;
    at::Tensor ws = at::empty({(int64_t)nchunks * L.C * 2},
                              input.options().dtype(at::kDouble));
    if (plan.path == RedPath::NchwFlat) {
      const auto& g = plan.flat;
      hipLaunchKernelGGL((bn_stats_partial_nchw_flat<native_t>), g.grid,
                         dim3(MSBN_BLOCK), 0, stream, x,
                         ws.data_ptr<double>(), L.N, L.C, L.S, g.chunk_len);
    } else if (plan.path == RedPath::NchwVec) {
      const auto& g = plan.nchw;
      MSBN_DISPATCH_V(v, VMAX, [&] {
        hipLaunchKernelGGL((bn_stats_partial_nchw<native_t, VV>), g.grid,
                           dim3(MSBN_BLOCK), 0, stream, x,
                           ws.data_ptr<double>(), L.N, L.C, L.S, g.chunkN,
                           g.chunkS);
      });
    } else {
      const auto& g = plan.nhwc;
      MSBN_DISPATCH_V(v, VMAX, [&] {
        hipLaunchKernelGGL((bn_stats_partial_nhwc<native_t, VV>), g.grid,
                           dim3(MSBN_BLOCK), 0, stream, x,
                           ws.data_ptr<double>(), L.rows, L.C, g.chunk_rows,
                           g.lpr);
      });
    }
    const int fgrid = (int)cdiv(L.C, kFinalizeWavesPerBlock);
    MSBN_DISPATCH_RSTAT(rstat_type, "batch_norm_stats", [&] {
      MSBN_DISPATCH_WTYPE(w_type, "batch_norm_stats", [&] {
        rstat_t* rm = rmean ? reinterpret_cast<rstat_t*>(rmean->data_ptr())
                            : nullptr;
        rstat_t* rv = rvar ? reinterpret_cast<rstat_t*>(rvar->data_ptr())
                           : nullptr;
        const wt_t* wp =
            wpar ? reinterpret_cast<const wt_t*>(wpar->data_ptr()) : nullptr;
        const wt_t* bp =
            bpar ? reinterpret_cast<const wt_t*>(bpar->data_ptr()) : nullptr;
        hipLaunchKernelGGL((bn_stats_finalize<rstat_t, wt_t>), dim3(fgrid),
                           dim3(MSBN_BLOCK), 0, stream, ws.data_ptr<double>(),
                           nchunks, L.C, (double)count, (float)eps, mean_p,
                           invstd_p, count_p, rm, rv, (float)momentum, wp, bp,
                           scale_p, shift_p);
      });
    });
  });
}

}  // namespace

// =====================================================================
// public ops
// =====================================================================

std::tuple<at::Tensor, at::Tensor> batch_norm_stats(const at::Tensor& input,
                                                    double eps) {
  const int64_t C = input.size(1);
  auto opts = input.options().dtype(at::kFloat);
  auto mean = at::empty({C}, opts);
  auto invstd = at::empty({C}, opts);
  if (input.numel() == 0) {
    mean.zero_();
    invstd.zero_();
    return {mean, invstd};
  }
  stats_into(input, eps, mean.data_ptr<float>(), invstd.data_ptr<float>(),
             nullptr, nullptr, nullptr, 0.0);
  return {mean, invstd};
}

void batch_norm_stats_packed(const at::Tensor& input, double eps,
                             at::Tensor& out) {
  const int64_t C = input.size(1);
  TORCH_CHECK(out.is_contiguous() && out.numel() == 2 * C + 1 &&
                  out.scalar_type() == at::kFloat,
              "packed stats buffer must be contiguous fp32 of size 2C+1");
  if (input.numel() == 0) {
    out.zero_();
    return;
  }
  float* p = out.data_ptr<float>();
  stats_into(input, eps, p, p + C, p + 2 * C, nullptr, nullptr, 0.0);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_gather_stats_packed_coefs(
    const at::Tensor& packed_all, const c10::optional<at::Tensor>& running_mean,
    const c10::optional<at::Tensor>& running_var, double momentum, double eps,
    const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, bool want_coefs) {
  TORCH_CHECK(packed_all.dim() == 2 && packed_all.is_contiguous() &&
                  packed_all.scalar_type() == at::kFloat,
              "packed_all must be contiguous fp32 [W, 2C+1]");
  const int W = (int)packed_all.size(0);
  const int64_t C = (packed_all.size(1) - 1) / 2;
  auto opts = packed_all.options();
  auto mean = at::empty({C}, opts);
  auto invstd = at::empty({C}, opts);
  auto count_sum = at::empty({1}, opts);
  at::Tensor coefs;
  float* scale_p = nullptr;
  float* shift_p = nullptr;
  if (want_coefs) {
    coefs = at::empty({2 * C}, opts);
    scale_p = coefs.data_ptr<float>();
    shift_p = scale_p + C;
  }
  auto stream = cur_stream();
  const auto rstat_type =
      running_mean.has_value() ? running_mean->scalar_type() : at::kFloat;
  const auto w_type = weight.has_value() ? weight->scalar_type()
                      : bias.has_value() ? bias->scalar_type()
                                         : at::kFloat;
  const int fgrid = (int)cdiv(C, MSBN_BLOCK);
  MSBN_DISPATCH_RSTAT(rstat_type, "gather_stats", [&] {
    MSBN_DISPATCH_WTYPE(w_type, "gather_stats", [&] {
      rstat_t* rm = running_mean.has_value()
                        ? reinterpret_cast<rstat_t*>(running_mean->data_ptr())
                        : nullptr;
      rstat_t* rv = running_var.has_value()
                        ? reinterpret_cast<rstat_t*>(running_var->data_ptr())
                        : nullptr;
      const wt_t* wp =
          weight.has_value()
              ? reinterpret_cast<const wt_t*>(weight->data_ptr())
              : nullptr;
      const wt_t* bp = bias.has_value()
                           ? reinterpret_cast<const wt_t*>(bias->data_ptr())
                           : nullptr;
      hipLaunchKernelGGL((bn_gather_stats<rstat_t, wt_t>), dim3(fgrid),
                         dim3(MSBN_BLOCK), 0, stream,
                         packed_all.data_ptr<float>(), W, C, (float)eps,
                         (float)momentum, mean.data_ptr<float>(),
                         invstd.data_ptr<float>(), count_sum.data_ptr<float>(),
                         rm, rv, wp, bp, scale_p, shift_p);
    });
  });
  return {mean, invstd, count_sum, coefs};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> batch_norm_gather_stats_packed(
    const at::Tensor& packed_all, const c10::optional<at::Tensor>& running_mean,
    const c10::optional<at::Tensor>& running_var, double momentum, double eps) {
  auto r = batch_norm_gather_stats_packed_coefs(
      packed_all, running_mean, running_var, momentum, eps, c10::nullopt,
      c10::nullopt, false);
  return {std::get<0>(r), std::get<1>(r), std::get<2>(r)};
}

// Fused local (world_size==1) stats: partial+finalize with running-stats
// update AND [scale|shift] coefs in ONE finalize launch.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_stats_local(const at::Tensor& input, double eps,
                       const c10::optional<at::Tensor>& running_mean,
                       const c10::optional<at::Tensor>& running_var,
                       double momentum,
                       const c10::optional<at::Tensor>& weight,
                       const c10::optional<at::Tensor>& bias,
                       bool want_coefs) {
  const int64_t C = input.size(1);
  auto opts = input.options().dtype(at::kFloat);
  auto mean = at::empty({C}, opts);
  auto invstd = at::empty({C}, opts);
  auto count_sum = at::empty({1}, opts);
  at::Tensor coefs;
  float* scale_p = nullptr;
  float* shift_p = nullptr;
  if (want_coefs) {
    coefs = at::empty({2 * C}, opts);
    scale_p = coefs.data_ptr<float>();
    shift_p = scale_p + C;
  }
  TORCH_CHECK(input.numel() > 0, "batch_norm_stats_local: empty input");
  const at::Tensor* rm =
      running_mean.has_value() ? &running_mean.value() : nullptr;
  const at::Tensor* rv =
      running_var.has_value() ? &running_var.value() : nullptr;
  const at::Tensor* wp = weight.has_value() ? &weight.value() : nullptr;
  const at::Tensor* bp = bias.has_value() ? &bias.value() : nullptr;
  stats_into(input, eps, mean.data_ptr<float>(), invstd.data_ptr<float>(),
             count_sum.data_ptr<float>(), rm, rv, momentum, wp, bp, scale_p,
             shift_p);
  return {mean, invstd, count_sum, coefs};
}

std::tuple<at::Tensor, at::Tensor> batch_norm_gather_stats_with_counts(
    const at::Tensor& mean_all, const at::Tensor& invstd_all,
    const c10::optional<at::Tensor>& running_mean,
    const c10::optional<at::Tensor>& running_var, double momentum, double eps,
    const at::Tensor& counts) {
  // API-parity wrapper: assemble the packed layout, then run the packed path.
  const int64_t W = mean_all.size(0);
  const int64_t C = mean_all.size(1);
  auto packed = at::empty({W, 2 * C + 1}, mean_all.options().dtype(at::kFloat));
  packed.narrow(1, 0, C).copy_(mean_all);
  packed.narrow(1, C, C).copy_(invstd_all);
  packed.narrow(1, 2 * C, 1).copy_(
      counts.to(at::kFloat).reshape({W, 1}));
  auto out = batch_norm_gather_stats_packed(packed, running_mean, running_var,
                                            momentum, eps);
  return {std::get<0>(out), std::get<1>(out)};
}

namespace {
// compute per-channel (scale, shift) into one [2C] fp32 buffer
at::Tensor make_fwd_coefs(const at::Tensor& mean, const at::Tensor& invstd,
                          const c10::optional<at::Tensor>& weight,
                          const c10::optional<at::Tensor>& bias, int64_t C) {
  auto coefs = at::empty({2 * C}, mean.options().dtype(at::kFloat));
  float* scale = coefs.data_ptr<float>();
  float* shift = scale + C;
  auto stream = cur_stream();
  const int cgrid = (int)cdiv(C, MSBN_BLOCK);
  const auto wtype = weight.has_value() ? weight->scalar_type()
                     : bias.has_value() ? bias->scalar_type()
                                        : at::kFloat;
  MSBN_DISPATCH_RSTAT(wtype, "bn_affine", [&] {
    const rstat_t* w =
        weight.has_value()
            ? reinterpret_cast<const rstat_t*>(weight->data_ptr())
            : nullptr;
    const rstat_t* b = bias.has_value()
                           ? reinterpret_cast<const rstat_t*>(bias->data_ptr())
                           : nullptr;
    hipLaunchKernelGGL((bn_affine_fwd<rstat_t>), dim3(cgrid), dim3(MSBN_BLOCK),
                       0, stream, mean.data_ptr<float>(),
                       invstd.data_ptr<float>(), w, b, C, scale, shift);
  });
  return coefs;
}

#define MSBN_DISPATCH_BOOL(FLAG, NAME, ...)                                  \
  [&] {                                                                      \
    if (FLAG) {                                                              \
      constexpr bool NAME = true;                                            \
      return __VA_ARGS__();                                                  \
    } else {                                                                 \
      constexpr bool NAME = false;                                           \
      return __VA_ARGS__();                                                  \
    }                                                                        \
  }()

// Activation mode of the fused epilogue: off -> kActNone; on with a zero
// slope -> kActRelu (the instantiation ReLU models have always run, so their
// results do not move); any other slope -> kActLeaky.
inline int act_mode(bool on, float slope) {
  return !on ? kActNone : (slope == 0.f ? kActRelu : kActLeaky);
}

#define MSBN_DISPATCH_ACT(MODE, NAME, ...)                                   \
  [&] {                                                                      \
    switch (MODE) {                                                          \
      case kActRelu: {                                                       \
        constexpr int NAME = kActRelu;                                       \
        return __VA_ARGS__();                                                \
      }                                                                      \
      case kActLeaky: {                                                      \
        constexpr int NAME = kActLeaky;                                      \
        return __VA_ARGS__();                                                \
      }                                                                      \
      default: {                                                             \
        constexpr int NAME = kActNone;                                       \
        return __VA_ARGS__();                                                \
      }                                                                      \
    }                                                                        \
  }()

// The frozen / small-plane launchers prune flag combinations that cannot
// occur (no gate -> no residual read); they pass the mode as a type.
template <int ACT>
using ActC = std::integral_constant<int, ACT>;
}  // namespace

at::Tensor bn_make_coefs(const at::Tensor& mean, const at::Tensor& invstd,
                         const c10::optional<at::Tensor>& weight,
                         const c10::optional<at::Tensor>& bias) {
  return make_fwd_coefs(mean, invstd, weight, bias, mean.numel());
}

namespace {
// ceil(numel / 8) dense bytes next to the activation tensor they describe
void check_gate_tensor(const at::Tensor& gate, const at::Tensor& input,
                       const char* name) {
  TORCH_CHECK(gate.scalar_type() == at::kByte && gate.is_contiguous() &&
                  gate.device() == input.device() &&
                  gate.numel() == (input.numel() + 7) / 8,
              name, " must be a contiguous uint8 tensor of ceil(numel/8) "
              "bytes on the input's device");
}

// The bit-storing forward kernels exist for an activation, a residual and a
// pack of 8 (one thread = one byte); anything else declines.
inline bool elemt_writes_gate(int act, bool has_res, int v) {
  return act != kActNone && has_res && v == 8;
}
}  // namespace

std::tuple<at::Tensor, bool> batch_norm_elemt_act(
    const at::Tensor& input, const c10::optional<at::Tensor>& residual,
    const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, const at::Tensor& mean,
    const at::Tensor& invstd, bool relu,
    const c10::optional<at::Tensor>& coefs_in, double negative_slope,
    const c10::optional<at::Tensor>& gate_out) {
  const Layout L = get_layout(input);
  auto out = at::empty_like(input);
  if (gate_out.has_value())
    check_gate_tensor(*gate_out, input, "gate_out");
  bool wrote_gate = false;
  if (input.numel() == 0) return {out, wrote_gate};
  const float slope = (float)negative_slope;
  const int act = act_mode(relu, slope);
  auto stream = cur_stream();
  auto coefs = coefs_in.has_value()
                   ? *coefs_in
                   : make_fwd_coefs(mean, invstd, weight, bias, L.C);
  float* scale = coefs.data_ptr<float>();
  float* shift = scale + L.C;
  const bool has_res = residual.has_value();
  if (has_res) {
    TORCH_CHECK(residual->sizes() == input.sizes() &&
                    residual->strides() == input.strides() &&
                    residual->scalar_type() == input.scalar_type(),
                "residual must match input shape/strides/dtype");
  }

  const int64_t total = input.numel();
  MSBN_DISPATCH_FLOAT_TYPES(input.scalar_type(), "bn_elemt", [&] {
    const native_t* x =
        reinterpret_cast<const native_t*>(input.data_ptr<scalar_t>());
    const native_t* res =
        has_res ? reinterpret_cast<const native_t*>(residual->data_ptr())
                : nullptr;
    native_t* y = reinterpret_cast<native_t*>(out.data_ptr<scalar_t>());
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    const ElemtPlan plan =
        plan_elemt(L, total, (int)sizeof(native_t), {x, y, res}, scale);
    const int v = plan.v;
    const int grid = plan.grid;
    wrote_gate = gate_out.has_value() && elemt_writes_gate(act, has_res, v);
    unsigned char* gate =
        wrote_gate ? gate_out->data_ptr<unsigned char>() : nullptr;
    MSBN_DISPATCH_V(v, VMAX, [&] {
      MSBN_DISPATCH_ACT(act, ACT_, [&] {
        MSBN_DISPATCH_BOOL(has_res, RES_, [&] {
          auto launch = [&](auto gate_c) {
            constexpr bool GATE_ = decltype(gate_c)::value;
            if (!L.nhwc) {
              hipLaunchKernelGGL(
                  (bn_elemt_nchw<native_t, VV, ACT_, RES_, GATE_>), dim3(grid),
                  dim3(MSBN_BLOCK), 0, stream, x, res, y, scale, shift, total,
                  L.C, L.S, slope, gate);
            } else {
              hipLaunchKernelGGL(
                  (bn_elemt_nhwc<native_t, VV, ACT_, RES_, GATE_>), dim3(grid),
                  dim3(MSBN_BLOCK), 0, stream, x, res, y, scale, shift, total,
                  L.C, slope, gate);
            }
          };
          // the bit store is compiled for the one combination that can run
          // it (elemt_writes_gate): 2 dtypes x 2 activations x 2 layouts
          constexpr bool kCanGate = VV == 8 && sizeof(native_t) == 2 &&
                                    ACT_ != kActNone && RES_;
          if (wrote_gate) {
            launch(std::integral_constant<bool, kCanGate>{});
          } else {
            launch(std::false_type{});
          }
        });
      });
    });
  });
  return {out, wrote_gate};
}

at::Tensor batch_norm_elemt(const at::Tensor& input,
                            const c10::optional<at::Tensor>& weight,
                            const c10::optional<at::Tensor>& bias,
                            const at::Tensor& mean, const at::Tensor& invstd,
                            double eps) {
  (void)eps;  // invstd already folds eps
  return std::get<0>(batch_norm_elemt_act(input, c10::nullopt, weight, bias,
                                          mean, invstd, false, c10::nullopt,
                                          0.0, c10::nullopt));
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_backward_reduce_act(
    const at::Tensor& grad_out, const at::Tensor& input,
    const c10::optional<at::Tensor>& residual, const at::Tensor& mean,
    const at::Tensor& invstd, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, bool relu_mask, bool input_g,
    bool weight_g, bool bias_g, const c10::optional<at::Tensor>& coefs_in,
    const c10::optional<at::Tensor>& gm_out, double negative_slope,
    const c10::optional<at::Tensor>& grad_out2,
    const c10::optional<at::Tensor>& gate) {
  const Layout L = get_layout(input);
  const float slope = (float)negative_slope;
  const int act = act_mode(relu_mask, slope);
  const bool has_gate = gate.has_value();
  if (has_gate) {
    // the bits stand in for the residual: the forward wrote them for an
    // activated bn+add layer of a 2-byte dtype, and gm carries the result
    TORCH_CHECK(act != kActNone && !residual.has_value() &&
                    gm_out.has_value() && input.element_size() == 2,
                "gate needs relu_mask, gm_out, a bf16 / half input and no "
                "residual");
    check_gate_tensor(*gate, input, "gate");
  }
  if (input.numel() == 0) {
    auto z32 = input.options().dtype(at::kFloat);
    auto combined0 = at::zeros({2 * L.C}, z32);
    const auto wt = weight.has_value() ? weight->scalar_type()
                                       : input.scalar_type();
    at::Tensor gw0, gb0;
    if (weight_g) gw0 = at::zeros({L.C}, input.options().dtype(wt));
    if (bias_g) gb0 = at::zeros({L.C}, input.options().dtype(wt));
    return {combined0.narrow(0, 0, L.C), combined0.narrow(0, L.C, L.C), gw0,
            gb0};
  }
  const bool want_gm = gm_out.has_value();
  if (want_gm) {
    TORCH_CHECK(gm_out->sizes() == input.sizes() &&
                    gm_out->strides() == input.strides() &&
                    gm_out->scalar_type() == input.scalar_type(),
                "gm_out must match input shape/strides/dtype");
  }
  TORCH_CHECK(grad_out.sizes() == input.sizes() &&
                  grad_out.strides() == input.strides(),
              "grad_out must match input shape and layout");
  const bool has_dy2 = grad_out2.has_value();
  if (has_dy2) {
    TORCH_CHECK(want_gm, "grad_out2 requires gm_out");
    TORCH_CHECK(grad_out2->sizes() == input.sizes() &&
                    grad_out2->strides() == input.strides() &&
                    grad_out2->scalar_type() == input.scalar_type() &&
                    grad_out2->device() == input.device(),
                "grad_out2 must match input shape/strides/dtype");
  }
  TORCH_CHECK(!residual.has_value() ||
                  (residual->sizes() == input.sizes() &&
                   residual->strides() == input.strides()),
              "residual must match input shape and layout");
  auto f32 = input.options().dtype(at::kFloat);
  // ONE contiguous buffer for [sum_dy | sum_dy_xmu] -> single all_reduce.
  auto combined = at::empty({2 * L.C}, f32);
  auto sum_dy = combined.narrow(0, 0, L.C);
  auto sum_dy_xmu = combined.narrow(0, L.C, L.C);
  const auto wtype =
      weight.has_value() ? weight->scalar_type() : input.scalar_type();
  auto wopts = input.options().dtype(wtype);
  at::Tensor grad_weight, grad_bias;
  if (weight_g) grad_weight = at::empty({L.C}, wopts);
  if (bias_g) grad_bias = at::empty({L.C}, wopts);

  const bool has_res = residual.has_value();
  float* scale = nullptr;
  float* shift = nullptr;
  at::Tensor coefs;
  if (relu_mask && !has_gate) {  // the gate kernels never form z
    coefs = coefs_in.has_value()
                ? *coefs_in
                : make_fwd_coefs(mean, invstd, weight, bias, L.C);
    scale = coefs.data_ptr<float>();
    shift = scale + L.C;
  }
  // byte loads: no alignment demand, so not among plan_reduce's pointers
  const unsigned char* gate_p =
      has_gate ? gate->data_ptr<unsigned char>() : nullptr;

  auto stream = cur_stream();
  MSBN_DISPATCH_FLOAT_TYPES(input.scalar_type(), "bn_bwd_reduce", [&] {
    const native_t* x =
        reinterpret_cast<const native_t*>(input.data_ptr<scalar_t>());
    const native_t* dy =
        reinterpret_cast<const native_t*>(grad_out.data_ptr<scalar_t>());
    const native_t* res =
        has_res ? reinterpret_cast<const native_t*>(residual->data_ptr())
                : nullptr;
    native_t* gm =
        want_gm ? reinterpret_cast<native_t*>(gm_out->data_ptr()) : nullptr;
    const native_t* dy2 =
        has_dy2 ? reinterpret_cast<const native_t*>(grad_out2->data_ptr())
                : nullptr;
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    // every pointer the partial kernel dereferences, gm_out / dy2 included
    const ReducePlan plan =
        plan_reduce(L, (int)sizeof(native_t), {x, dy, res, gm, dy2});
    const int v = plan.v;
    const int nchunks = plan.nchunks;
    at::Tensor ws = at::empty({(int64_t)nchunks * L.C * 2},
                              input.options().dtype(at::kDouble));
    MSBN_DISPATCH_ACT(act, ACT_, [&] {
      MSBN_DISPATCH_BOOL(has_res, RES_, [&] {
        MSBN_DISPATCH_BOOL(want_gm, GM_, [&] {
          // DY2 exists only with GMOUT (has_dy2 implies want_gm, checked
          // above): 3 kernels per (T, V, ACT, RES), not 4
          // GATE likewise only where the checks above let it run (an
          // activation, GMOUT, no RES, a 2-byte dtype)
          auto launch = [&](auto dy2_c, auto gate_c) {
            constexpr bool DY2_ = decltype(dy2_c)::value && GM_;
            constexpr bool GATE_ = decltype(gate_c)::value && GM_ && !RES_ &&
                                   ACT_ != kActNone && sizeof(native_t) == 2;
            if (!L.nhwc) {
              if (plan.path == RedPath::NchwFlat) {
                const auto& g = plan.flat;
                hipLaunchKernelGGL(
                    (bn_bwd_reduce_partial_nchw_flat<native_t, ACT_, RES_,
                                                     GM_, DY2_, GATE_>),
                    g.grid, dim3(MSBN_BLOCK), 0, stream, dy, dy2, x, res, gm,
                    mean.data_ptr<float>(), scale, shift,
                    ws.data_ptr<double>(), L.N, L.C, L.S, g.chunk_len, slope,
                    gate_p);
              } else {
                const auto& g = plan.nchw;
                MSBN_DISPATCH_V(v, VMAX, [&] {
                  hipLaunchKernelGGL(
                      (bn_bwd_reduce_partial_nchw<native_t, VV, ACT_, RES_,
                                                  GM_, DY2_, GATE_>),
                      g.grid, dim3(MSBN_BLOCK), 0, stream, dy, dy2, x, res,
                      gm, mean.data_ptr<float>(), scale, shift,
                      ws.data_ptr<double>(), L.N, L.C, L.S, g.chunkN,
                      g.chunkS, slope, gate_p);
                });
              }
            } else {
              const auto& g = plan.nhwc;
              MSBN_DISPATCH_V(v, VMAX, [&] {
                hipLaunchKernelGGL(
                    (bn_bwd_reduce_partial_nhwc<native_t, VV, ACT_, RES_, GM_,
                                                DY2_, GATE_>),
                    g.grid, dim3(MSBN_BLOCK), 0, stream, dy, dy2, x, res, gm,
                    mean.data_ptr<float>(), scale, shift,
                    ws.data_ptr<double>(), L.rows, L.C, g.chunk_rows, g.lpr,
                    slope, gate_p);
              });
            }
          };
          if (has_gate) {
            if (has_dy2) {
              launch(std::true_type{}, std::true_type{});
            } else {
              launch(std::false_type{}, std::true_type{});
            }
          } else if (has_dy2) {
            launch(std::true_type{}, std::false_type{});
          } else {
            launch(std::false_type{}, std::false_type{});
          }
        });
      });
    });
    const int fgrid = (int)cdiv(L.C, kFinalizeWavesPerBlock);
    MSBN_DISPATCH_RSTAT(wtype, "bn_bwd_reduce", [&] {
      rstat_t* gw = weight_g ? reinterpret_cast<rstat_t*>(grad_weight.data_ptr())
                             : nullptr;
      rstat_t* gb =
          bias_g ? reinterpret_cast<rstat_t*>(grad_bias.data_ptr()) : nullptr;
      hipLaunchKernelGGL((bn_bwd_reduce_finalize<rstat_t>), dim3(fgrid),
                         dim3(MSBN_BLOCK), 0, stream, ws.data_ptr<double>(),
                         nchunks, L.C, invstd.data_ptr<float>(),
                         sum_dy.data_ptr<float>(),
                         sum_dy_xmu.data_ptr<float>(), gw, gb);
    });
  });
  (void)input_g;
  return {sum_dy, sum_dy_xmu, grad_weight, grad_bias};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_backward_reduce(const at::Tensor& grad_out, const at::Tensor& input,
                           const at::Tensor& mean, const at::Tensor& invstd,
                           const c10::optional<at::Tensor>& weight, bool input_g,
                           bool weight_g, bool bias_g) {
  return batch_norm_backward_reduce_act(grad_out, input, c10::nullopt, mean,
                                        invstd, weight, c10::nullopt, false,
                                        input_g, weight_g, bias_g,
                                        c10::nullopt, c10::nullopt, 0.0,
                                        c10::nullopt, c10::nullopt);
}

std::tuple<at::Tensor, at::Tensor> batch_norm_backward_elemt_act(
    const at::Tensor& grad_out, const at::Tensor& input,
    const c10::optional<at::Tensor>& residual, const at::Tensor& mean,
    const at::Tensor& invstd, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, const at::Tensor& sum_dy,
    const at::Tensor& sum_dy_xmu, const at::Tensor& count, bool relu_mask,
    bool want_res_grad, const c10::optional<at::Tensor>& coefs_in,
    double negative_slope) {
  const Layout L = get_layout(input);
  const float slope = (float)negative_slope;
  const int act = act_mode(relu_mask, slope);
  auto dx = at::empty_like(grad_out);
  at::Tensor dres;
  if (want_res_grad) dres = at::empty_like(grad_out);
  if (input.numel() == 0) return {dx, dres};
  // total count as a device fp32 scalar (no host sync)
  at::Tensor count_sum;
  if (count.numel() == 1 && count.scalar_type() == at::kFloat) {
    count_sum = count;
  } else {
    count_sum = count.to(at::kFloat).sum().reshape({1});
  }
  auto stream = cur_stream();
  auto f32 = input.options().dtype(at::kFloat);
  auto coefs = at::empty({3 * L.C}, f32);
  float* ca = coefs.data_ptr<float>();
  float* cb = ca + L.C;
  float* cd = cb + L.C;
  const int cgrid = (int)cdiv(L.C, MSBN_BLOCK);
  const auto wtype =
      weight.has_value() ? weight->scalar_type() : at::kFloat;
  MSBN_DISPATCH_RSTAT(wtype, "bn_bwd_elemt", [&] {
    const rstat_t* w =
        weight.has_value()
            ? reinterpret_cast<const rstat_t*>(weight->data_ptr())
            : nullptr;
    hipLaunchKernelGGL((bn_affine_bwd<rstat_t>), dim3(cgrid), dim3(MSBN_BLOCK),
                       0, stream, mean.data_ptr<float>(),
                       invstd.data_ptr<float>(), w, sum_dy.data_ptr<float>(),
                       sum_dy_xmu.data_ptr<float>(),
                       count_sum.data_ptr<float>(), L.C, ca, cb, cd);
  });
  const bool has_res = residual.has_value();
  float* scale = nullptr;
  float* shift = nullptr;
  at::Tensor fcoefs;
  if (relu_mask) {
    fcoefs = coefs_in.has_value()
                 ? *coefs_in
                 : make_fwd_coefs(mean, invstd, weight, bias, L.C);
    scale = fcoefs.data_ptr<float>();
    shift = scale + L.C;
  }

  const int64_t total = input.numel();
  MSBN_DISPATCH_FLOAT_TYPES(input.scalar_type(), "bn_bwd_elemt", [&] {
    const native_t* x =
        reinterpret_cast<const native_t*>(input.data_ptr<scalar_t>());
    const native_t* dy =
        reinterpret_cast<const native_t*>(grad_out.data_ptr<scalar_t>());
    const native_t* res =
        has_res ? reinterpret_cast<const native_t*>(residual->data_ptr())
                : nullptr;
    native_t* o = reinterpret_cast<native_t*>(dx.data_ptr<scalar_t>());
    native_t* dr = want_res_grad
                       ? reinterpret_cast<native_t*>(dres.data_ptr<scalar_t>())
                       : nullptr;
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    // every pointer the launch touches (absent ones are nullptr)
    const ElemtPlan plan = plan_elemt(L, total, (int)sizeof(native_t),
                                      {x, dy, res, o, dr}, scale);
    const int v = plan.v;
    const int grid = plan.grid;
    MSBN_DISPATCH_V(v, VMAX, [&] {
      MSBN_DISPATCH_ACT(act, ACT_, [&] {
        MSBN_DISPATCH_BOOL(has_res, RES_, [&] {
          MSBN_DISPATCH_BOOL(want_res_grad, RESG_, [&] {
            if (!L.nhwc) {
              hipLaunchKernelGGL(
                  (bn_bwd_elemt_nchw<native_t, VV, ACT_, RES_, RESG_>),
                  dim3(grid), dim3(MSBN_BLOCK), 0, stream, dy, x, res, o, dr,
                  ca, cb, cd, scale, shift, total, L.C, L.S, slope);
            } else {
              hipLaunchKernelGGL(
                  (bn_bwd_elemt_nhwc<native_t, VV, ACT_, RES_, RESG_>),
                  dim3(grid), dim3(MSBN_BLOCK), 0, stream, dy, x, res, o, dr,
                  ca, cb, cd, scale, shift, total, L.C, slope);
            }
          });
        });
      });
    });
  });
  return {dx, dres};
}

at::Tensor batch_norm_backward_elemt(
    const at::Tensor& grad_out, const at::Tensor& input, const at::Tensor& mean,
    const at::Tensor& invstd, const c10::optional<at::Tensor>& weight,
    const at::Tensor& sum_dy, const at::Tensor& sum_dy_xmu,
    const at::Tensor& count) {
  return std::get<0>(batch_norm_backward_elemt_act(
      grad_out, input, c10::nullopt, mean, invstd, weight, c10::nullopt,
      sum_dy, sum_dy_xmu, count, false, false, c10::nullopt, 0.0));
}

// ---------------------------------------------------------------------------
// stem pool fusion: bn + act + MaxPool2d(3, 2, 1), channels-last
// ---------------------------------------------------------------------------
namespace {
struct PoolGeom {
  int H, W, OH, OW;
};

// The pool ops' layout of x: always rows x C.  A 1x1 plane is dense in both
// formats (get_layout calls it NCHW); its memory is rows x C all the same.
Layout pool_layout(const at::Tensor& x, const char* op) {
  TORCH_CHECK(x.dim() == 4 &&
                  x.is_contiguous(at::MemoryFormat::ChannelsLast),
              op, ": input must be a dense 4-D channels-last tensor");
  Layout L{};
  L.nhwc = true;
  L.N = x.size(0);
  L.C = x.size(1);
  L.S = x.size(2) * x.size(3);
  L.rows = L.N * L.S;
  return L;
}

// geometry of the fixed kernel-3 / stride-2 / padding-1 / floor-mode pool
PoolGeom pool_geom(const at::Tensor& x, const Layout& L, const char* op) {
  TORCH_CHECK(L.rows < (int64_t)INT32_MAX, op, ": N*H*W must be below 2^31");
  PoolGeom g{};
  g.H = (int)x.size(2);
  g.W = (int)x.size(3);
  g.OH = (g.H - 1) / 2 + 1;
  g.OW = (g.W - 1) / 2 + 1;
  return g;
}

void check_pooled(const at::Tensor& t, const at::Tensor& x, const PoolGeom& g,
                  at::ScalarType dtype, const char* op, const char* what) {
  TORCH_CHECK(t.dim() == 4 && t.size(0) == x.size(0) &&
                  t.size(1) == x.size(1) && t.size(2) == g.OH &&
                  t.size(3) == g.OW && t.scalar_type() == dtype &&
                  t.device() == x.device() &&
                  t.is_contiguous(at::MemoryFormat::ChannelsLast),
              op, ": ", what, " must be a channels-last [N, C, OH, OW] ",
              dtype, " tensor on the input's device");
}
}  // namespace

std::tuple<at::Tensor, at::Tensor> batch_norm_elemt_act_pool(
    const at::Tensor& input, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, const at::Tensor& mean,
    const at::Tensor& invstd, bool relu,
    const c10::optional<at::Tensor>& coefs_in, double negative_slope) {
  const Layout L = pool_layout(input, "bn_elemt_pool");
  TORCH_CHECK(input.numel() > 0, "bn_elemt_pool: empty input");
  const PoolGeom g = pool_geom(input, L, "bn_elemt_pool");
  const float slope = (float)negative_slope;
  const int act = act_mode(relu, slope);
  auto out = at::empty({input.size(0), L.C, g.OH, g.OW},
                       input.options().memory_format(
                           at::MemoryFormat::ChannelsLast));
  auto codes = at::empty_like(out, out.options().dtype(at::kByte));
  auto stream = cur_stream();
  auto coefs = coefs_in.has_value()
                   ? *coefs_in
                   : make_fwd_coefs(mean, invstd, weight, bias, L.C);
  float* scale = coefs.data_ptr<float>();
  float* shift = scale + L.C;
  const int64_t total = out.numel();
  MSBN_DISPATCH_FLOAT_TYPES(input.scalar_type(), "bn_elemt_pool", [&] {
    const native_t* x =
        reinterpret_cast<const native_t*>(input.data_ptr<scalar_t>());
    native_t* y = reinterpret_cast<native_t*>(out.data_ptr<scalar_t>());
    uint8_t* cp = codes.data_ptr<uint8_t>();
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    const ElemtPlan plan =
        plan_elemt(L, total, (int)sizeof(native_t), {x, y, cp}, scale);
    MSBN_DISPATCH_V(plan.v, VMAX, [&] {
      // the dispatcher names widths past 16 B for this type; never chosen
      constexpr int VK = VV * (int)sizeof(native_t) <= 16 ? VV : 1;
      MSBN_DISPATCH_ACT(act, ACT_, [&] {
        hipLaunchKernelGGL((bn_elemt_pool_nhwc<native_t, VK, ACT_>),
                           dim3(plan.grid), dim3(MSBN_BLOCK), 0, stream, x, y,
                           cp, scale, shift, total, L.C, g.H, g.W, g.OH, g.OW,
                           slope);
      });
    });
  });
  return {out, codes};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_backward_reduce_act_pool(
    const at::Tensor& grad_out, const c10::optional<at::Tensor>& grad_out2,
    const at::Tensor& codes, const at::Tensor& input, const at::Tensor& mean,
    const at::Tensor& invstd, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, bool relu_mask, bool input_g,
    bool weight_g, bool bias_g, const c10::optional<at::Tensor>& coefs_in,
    double negative_slope) {
  const Layout L = pool_layout(input, "bn_bwd_reduce_pool");
  TORCH_CHECK(input.numel() > 0, "bn_bwd_reduce_pool: empty input");
  const PoolGeom g = pool_geom(input, L, "bn_bwd_reduce_pool");
  const float slope = (float)negative_slope;
  const int act = act_mode(relu_mask, slope);
  check_pooled(grad_out, input, g, input.scalar_type(), "bn_bwd_reduce_pool",
               "grad_out");
  const bool has_dy2 = grad_out2.has_value();
  if (has_dy2)
    check_pooled(*grad_out2, input, g, input.scalar_type(),
                 "bn_bwd_reduce_pool", "grad_out2");
  check_pooled(codes, input, g, at::kByte, "bn_bwd_reduce_pool", "codes");
  auto f32 = input.options().dtype(at::kFloat);
  // ONE contiguous buffer for [sum_dy | sum_dy_xmu] -> single all_reduce.
  auto combined = at::empty({2 * L.C}, f32);
  auto sum_dy = combined.narrow(0, 0, L.C);
  auto sum_dy_xmu = combined.narrow(0, L.C, L.C);
  const auto wtype =
      weight.has_value() ? weight->scalar_type() : input.scalar_type();
  auto wopts = input.options().dtype(wtype);
  at::Tensor grad_weight, grad_bias;
  if (weight_g) grad_weight = at::empty({L.C}, wopts);
  if (bias_g) grad_bias = at::empty({L.C}, wopts);

  float* scale = nullptr;
  float* shift = nullptr;
  at::Tensor coefs;
  if (relu_mask) {
    coefs = coefs_in.has_value()
                ? *coefs_in
                : make_fwd_coefs(mean, invstd, weight, bias, L.C);
    scale = coefs.data_ptr<float>();
    shift = scale + L.C;
  }

  auto stream = cur_stream();
  MSBN_DISPATCH_FLOAT_TYPES(input.scalar_type(), "bn_bwd_reduce_pool", [&] {
    const native_t* x =
        reinterpret_cast<const native_t*>(input.data_ptr<scalar_t>());
    const native_t* dy =
        reinterpret_cast<const native_t*>(grad_out.data_ptr<scalar_t>());
    const native_t* dy2 =
        has_dy2 ? reinterpret_cast<const native_t*>(grad_out2->data_ptr())
                : nullptr;
    const uint8_t* cp = codes.data_ptr<uint8_t>();
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    // bwd_reduce's plan over x's rows; the pooled tensors and the codes
    // take part in the vector-width choice
    const ReducePlan plan =
        plan_reduce(L, (int)sizeof(native_t), {x, dy, dy2, cp});
    const int nchunks = plan.nchunks;
    const auto& ng = plan.nhwc;
    at::Tensor ws = at::empty({(int64_t)nchunks * L.C * 2},
                              input.options().dtype(at::kDouble));
    MSBN_DISPATCH_V(plan.v, VMAX, [&] {
      // the dispatcher names widths past 16 B for this type; never chosen
      constexpr int VK = VV * (int)sizeof(native_t) <= 16 ? VV : 1;
      MSBN_DISPATCH_ACT(act, ACT_, [&] {
        MSBN_DISPATCH_BOOL(has_dy2, DY2_, [&] {
          hipLaunchKernelGGL(
              (bn_bwd_reduce_pool_partial_nhwc<native_t, VK, ACT_, DY2_>),
              ng.grid, dim3(MSBN_BLOCK), 0, stream, dy, dy2, cp, x,
              mean.data_ptr<float>(), scale, shift, ws.data_ptr<double>(),
              L.rows, L.C, ng.chunk_rows, ng.lpr, g.H, g.W, g.OH, g.OW,
              slope);
        });
      });
    });
    const int fgrid = (int)cdiv(L.C, kFinalizeWavesPerBlock);
    MSBN_DISPATCH_RSTAT(wtype, "bn_bwd_reduce_pool", [&] {
      rstat_t* gw = weight_g ? reinterpret_cast<rstat_t*>(grad_weight.data_ptr())
                             : nullptr;
      rstat_t* gb =
          bias_g ? reinterpret_cast<rstat_t*>(grad_bias.data_ptr()) : nullptr;
      hipLaunchKernelGGL((bn_bwd_reduce_finalize<rstat_t>), dim3(fgrid),
                         dim3(MSBN_BLOCK), 0, stream, ws.data_ptr<double>(),
                         nchunks, L.C, invstd.data_ptr<float>(),
                         sum_dy.data_ptr<float>(),
                         sum_dy_xmu.data_ptr<float>(), gw, gb);
    });
  });
  (void)input_g;
  return {sum_dy, sum_dy_xmu, grad_weight, grad_bias};
}

at::Tensor batch_norm_backward_elemt_act_pool(
    const at::Tensor& grad_out, const c10::optional<at::Tensor>& grad_out2,
    const at::Tensor& codes, const at::Tensor& input, const at::Tensor& mean,
    const at::Tensor& invstd, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, const at::Tensor& sum_dy,
    const at::Tensor& sum_dy_xmu, const at::Tensor& count, bool relu_mask,
    const c10::optional<at::Tensor>& coefs_in, double negative_slope) {
  const Layout L = pool_layout(input, "bn_bwd_elemt_pool");
  TORCH_CHECK(input.numel() > 0, "bn_bwd_elemt_pool: empty input");
  const PoolGeom g = pool_geom(input, L, "bn_bwd_elemt_pool");
  const float slope = (float)negative_slope;
  const int act = act_mode(relu_mask, slope);
  check_pooled(grad_out, input, g, input.scalar_type(), "bn_bwd_elemt_pool",
               "grad_out");
  const bool has_dy2 = grad_out2.has_value();
  if (has_dy2)
    check_pooled(*grad_out2, input, g, input.scalar_type(),
                 "bn_bwd_elemt_pool", "grad_out2");
  check_pooled(codes, input, g, at::kByte, "bn_bwd_elemt_pool", "codes");
  auto dx = at::empty_like(input);
  // total count as a device fp32 scalar (no host sync)
  at::Tensor count_sum;
  if (count.numel() == 1 && count.scalar_type() == at::kFloat) {
    count_sum = count;
  } else {
    count_sum = count.to(at::kFloat).sum().reshape({1});
  }
  auto stream = cur_stream();
  auto f32 = input.options().dtype(at::kFloat);
  auto coefs = at::empty({3 * L.C}, f32);
  float* ca = coefs.data_ptr<float>();
  float* cb = ca + L.C;
  float* cd = cb + L.C;
  const int cgrid = (int)cdiv(L.C, MSBN_BLOCK);
  const auto wtype =
      weight.has_value() ? weight->scalar_type() : at::kFloat;
  MSBN_DISPATCH_RSTAT(wtype, "bn_bwd_elemt_pool", [&] {
    const rstat_t* w =
        weight.has_value()
            ? reinterpret_cast<const rstat_t*>(weight->data_ptr())
            : nullptr;
    hipLaunchKernelGGL((bn_affine_bwd<rstat_t>), dim3(cgrid), dim3(MSBN_BLOCK),
                       0, stream, mean.data_ptr<float>(),
                       invstd.data_ptr<float>(), w, sum_dy.data_ptr<float>(),
                       sum_dy_xmu.data_ptr<float>(),
                       count_sum.data_ptr<float>(), L.C, ca, cb, cd);
  });
  float* scale = nullptr;
  float* shift = nullptr;
  at::Tensor fcoefs;
  if (relu_mask) {
    fcoefs = coefs_in.has_value()
                 ? *coefs_in
                 : make_fwd_coefs(mean, invstd, weight, bias, L.C);
    scale = fcoefs.data_ptr<float>();
    shift = scale + L.C;
  }
  const int64_t total = input.numel();
  MSBN_DISPATCH_FLOAT_TYPES(input.scalar_type(), "bn_bwd_elemt_pool", [&] {
    const native_t* x =
        reinterpret_cast<const native_t*>(input.data_ptr<scalar_t>());
    const native_t* dy =
        reinterpret_cast<const native_t*>(grad_out.data_ptr<scalar_t>());
    const native_t* dy2 =
        has_dy2 ? reinterpret_cast<const native_t*>(grad_out2->data_ptr())
                : nullptr;
    const uint8_t* cp = codes.data_ptr<uint8_t>();
    native_t* o = reinterpret_cast<native_t*>(dx.data_ptr<scalar_t>());
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    const ElemtPlan plan = plan_elemt(L, total, (int)sizeof(native_t),
                                      {x, dy, dy2, cp, o}, scale);
    MSBN_DISPATCH_V(plan.v, VMAX, [&] {
      // the dispatcher names widths past 16 B for this type; never chosen
      constexpr int VK = VV * (int)sizeof(native_t) <= 16 ? VV : 1;
      MSBN_DISPATCH_ACT(act, ACT_, [&] {
        MSBN_DISPATCH_BOOL(has_dy2, DY2_, [&] {
          hipLaunchKernelGGL(
              (bn_bwd_elemt_pool_nhwc<native_t, VK, ACT_, DY2_>),
              dim3(plan.grid), dim3(MSBN_BLOCK), 0, stream, dy, dy2, cp, x, o,
              ca, cb, cd, scale, shift, total, L.C, g.H, g.W, g.OH, g.OW,
              slope);
        });
      });
    });
  });
  return dx;
}

// ---------------------------------------------------------------------------
// in-place activated path: forward over x, backward from y
// ---------------------------------------------------------------------------
namespace {
// The in-place kernels exist for the invertible activations only.
int inplace_act_mode(bool act, float slope, const char* name) {
  TORCH_CHECK(!act || slope > 0.f, name,
              ": the in-place path needs an invertible activation (identity, "
              "or LeakyReLU with negative_slope > 0); got negative_slope=",
              slope);
  return act ? kActLeaky : kActNone;
}

void check_same_dense(const at::Tensor& a, const at::Tensor& ref,
                      const char* what) {
  TORCH_CHECK(a.sizes() == ref.sizes() && a.strides() == ref.strides() &&
                  a.scalar_type() == ref.scalar_type() &&
                  a.device() == ref.device(),
              what, " must match the output's shape/strides/dtype/device");
}

at::ScalarType affine_type(const c10::optional<at::Tensor>& weight,
                           const c10::optional<at::Tensor>& bias) {
  const bool has_w = weight.has_value() && weight->defined();
  const bool has_b = bias.has_value() && bias->defined();
  TORCH_CHECK(!has_w || !has_b || weight->scalar_type() == bias->scalar_type(),
              "weight and bias dtypes differ");
  return has_w ? weight->scalar_type()
               : has_b ? bias->scalar_type() : at::kFloat;
}
}  // namespace

at::Tensor batch_norm_elemt_act_(at::Tensor& input,
                                 const c10::optional<at::Tensor>& weight,
                                 const c10::optional<at::Tensor>& bias,
                                 const at::Tensor& mean,
                                 const at::Tensor& invstd, bool act,
                                 const c10::optional<at::Tensor>& coefs_in,
                                 double negative_slope) {
  const float slope = (float)negative_slope;
  const int mode = inplace_act_mode(act, slope, "batch_norm_elemt_act_");
  const Layout L = get_layout(input);
  if (input.numel() == 0) return input;
  auto stream = cur_stream();
  auto coefs = coefs_in.has_value() && coefs_in->defined()
                   ? *coefs_in
                   : make_fwd_coefs(mean, invstd, weight, bias, L.C);
  TORCH_CHECK(coefs.scalar_type() == at::kFloat && coefs.is_contiguous() &&
                  coefs.numel() == 2 * L.C,
              "coefs must be contiguous fp32 [2C] ([scale | shift])");
  const float* scale = coefs.data_ptr<float>();
  const float* shift = scale + L.C;
  const int64_t total = input.numel();
  MSBN_DISPATCH_FLOAT_TYPES(input.scalar_type(), "bn_elemt_inplace", [&] {
    native_t* xy = reinterpret_cast<native_t*>(input.data_ptr<scalar_t>());
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    const ElemtPlan plan =
        plan_elemt(L, total, (int)sizeof(native_t), {xy}, scale);
    MSBN_DISPATCH_V(plan.v, VMAX, [&] {
      auto launch = [&](auto act_c) {
        constexpr int ACT_ = decltype(act_c)::value;
        if (!L.nhwc) {
          hipLaunchKernelGGL((bn_elemt_inplace_nchw<native_t, VV, ACT_>),
                             dim3(plan.grid), dim3(MSBN_BLOCK), 0, stream, xy,
                             scale, shift, total, L.C, L.S, slope);
        } else {
          hipLaunchKernelGGL((bn_elemt_inplace_nhwc<native_t, VV, ACT_>),
                             dim3(plan.grid), dim3(MSBN_BLOCK), 0, stream, xy,
                             scale, shift, total, L.C, slope);
        }
      };
      if (mode == kActLeaky) launch(ActC<kActLeaky>{});
      else launch(ActC<kActNone>{});
    });
  });
  return input;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_backward_reduce_inplace(
    const at::Tensor& grad_out, const at::Tensor& output,
    const at::Tensor& invstd, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, bool act, bool input_g,
    bool weight_g, bool bias_g, const c10::optional<at::Tensor>& coefs_in,
    double negative_slope) {
  (void)input_g;
  (void)coefs_in;  // 1/scale is formed from invstd*weight, as the coefs were
  const float slope = (float)negative_slope;
  const int mode =
      inplace_act_mode(act, slope, "batch_norm_backward_reduce_inplace");
  const float inv_slope = act ? 1.f / slope : 1.f;
  const Layout L = get_layout(output);
  const auto wtype = affine_type(weight, bias);
  auto f32 = output.options().dtype(at::kFloat);
  const auto gtype = weight.has_value() && weight->defined()
                         ? weight->scalar_type()
                         : output.scalar_type();
  auto wopts = output.options().dtype(gtype);
  if (output.numel() == 0) {
    auto combined0 = at::zeros({2 * L.C}, f32);
    at::Tensor gw0, gb0;
    if (weight_g) gw0 = at::zeros({L.C}, wopts);
    if (bias_g) gb0 = at::zeros({L.C}, wopts);
    return {combined0.narrow(0, 0, L.C), combined0.narrow(0, L.C, L.C), gw0,
            gb0};
  }
  check_same_dense(grad_out, output, "grad_out");
  // ONE contiguous buffer for [sum_dy | sum_dy_xmu] -> single all_reduce.
  auto combined = at::empty({2 * L.C}, f32);
  auto sum_dy = combined.narrow(0, 0, L.C);
  auto sum_dy_xmu = combined.narrow(0, L.C, L.C);
  at::Tensor grad_weight, grad_bias;
  if (weight_g) grad_weight = at::empty({L.C}, wopts);
  if (bias_g) grad_bias = at::empty({L.C}, wopts);

  auto stream = cur_stream();
  auto aux = at::empty({2 * L.C}, f32);
  float* rscale = aux.data_ptr<float>();
  float* bias_f = rscale + L.C;
  const int cgrid = (int)cdiv(L.C, MSBN_BLOCK);
  MSBN_DISPATCH_RSTAT(wtype, "bn_inplace_aux", [&] {
    const rstat_t* w =
        weight.has_value() && weight->defined()
            ? reinterpret_cast<const rstat_t*>(weight->data_ptr())
            : nullptr;
    const rstat_t* b = bias.has_value() && bias->defined()
                           ? reinterpret_cast<const rstat_t*>(bias->data_ptr())
                           : nullptr;
    hipLaunchKernelGGL((bn_inplace_aux<rstat_t>), dim3(cgrid),
                       dim3(MSBN_BLOCK), 0, stream, invstd.data_ptr<float>(),
                       w, b, L.C, rscale, bias_f);
  });

  MSBN_DISPATCH_FLOAT_TYPES(output.scalar_type(), "bn_bwd_reduce_inplace", [&] {
    const native_t* y =
        reinterpret_cast<const native_t*>(output.data_ptr<scalar_t>());
    const native_t* dy =
        reinterpret_cast<const native_t*>(grad_out.data_ptr<scalar_t>());
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    const ReducePlan plan = plan_reduce(L, (int)sizeof(native_t), {y, dy});
    const int nchunks = plan.nchunks;
    at::Tensor ws = at::empty({(int64_t)nchunks * L.C * 2},
                              output.options().dtype(at::kDouble));
    auto launch = [&](auto act_c) {
      constexpr int ACT_ = decltype(act_c)::value;
      if (plan.path == RedPath::NchwFlat) {
        const auto& g = plan.flat;
        hipLaunchKernelGGL(
            (bn_bwd_reduce_inplace_partial_nchw_flat<native_t, ACT_>), g.grid,
            dim3(MSBN_BLOCK), 0, stream, dy, y, rscale, bias_f,
            ws.data_ptr<double>(), L.N, L.C, L.S, g.chunk_len, slope,
            inv_slope);
      } else if (plan.path == RedPath::NchwVec) {
        const auto& g = plan.nchw;
        MSBN_DISPATCH_V(plan.v, VMAX, [&] {
          hipLaunchKernelGGL(
              (bn_bwd_reduce_inplace_partial_nchw<native_t, VV, ACT_>),
              g.grid, dim3(MSBN_BLOCK), 0, stream, dy, y, rscale, bias_f,
              ws.data_ptr<double>(), L.N, L.C, L.S, g.chunkN, g.chunkS, slope,
              inv_slope);
        });
      } else {
        const auto& g = plan.nhwc;
        MSBN_DISPATCH_V(plan.v, VMAX, [&] {
          hipLaunchKernelGGL(
              (bn_bwd_reduce_inplace_partial_nhwc<native_t, VV, ACT_>),
              g.grid, dim3(MSBN_BLOCK), 0, stream, dy, y, rscale, bias_f,
              ws.data_ptr<double>(), L.rows, L.C, g.chunk_rows, g.lpr, slope,
              inv_slope);
        });
      }
    };
    if (mode == kActLeaky) launch(ActC<kActLeaky>{});
    else launch(ActC<kActNone>{});
    const int fgrid = (int)cdiv(L.C, kFinalizeWavesPerBlock);
    MSBN_DISPATCH_RSTAT(gtype, "bn_bwd_reduce_inplace", [&] {
      rstat_t* gw = weight_g ? reinterpret_cast<rstat_t*>(grad_weight.data_ptr())
                             : nullptr;
      rstat_t* gb =
          bias_g ? reinterpret_cast<rstat_t*>(grad_bias.data_ptr()) : nullptr;
      hipLaunchKernelGGL((bn_bwd_reduce_finalize<rstat_t>), dim3(fgrid),
                         dim3(MSBN_BLOCK), 0, stream, ws.data_ptr<double>(),
                         nchunks, L.C, invstd.data_ptr<float>(),
                         sum_dy.data_ptr<float>(),
                         sum_dy_xmu.data_ptr<float>(), gw, gb);
    });
  });
  return {sum_dy, sum_dy_xmu, grad_weight, grad_bias};
}

at::Tensor batch_norm_backward_elemt_inplace(
    const at::Tensor& grad_out, const at::Tensor& output,
    const at::Tensor& mean, const at::Tensor& invstd,
    const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, const at::Tensor& sum_dy,
    const at::Tensor& sum_dy_xmu, const at::Tensor& count, bool act,
    const c10::optional<at::Tensor>& coefs_in, double negative_slope) {
  (void)coefs_in;
  const float slope = (float)negative_slope;
  const int mode =
      inplace_act_mode(act, slope, "batch_norm_backward_elemt_inplace");
  const float inv_slope = act ? 1.f / slope : 1.f;
  const Layout L = get_layout(output);
  auto dx = at::empty_like(grad_out);
  if (output.numel() == 0) return dx;
  check_same_dense(grad_out, output, "grad_out");
  // total count as a device fp32 scalar (no host sync)
  at::Tensor count_sum;
  if (count.numel() == 1 && count.scalar_type() == at::kFloat) {
    count_sum = count;
  } else {
    count_sum = count.to(at::kFloat).sum().reshape({1});
  }
  auto stream = cur_stream();
  auto coefs = at::empty({3 * L.C}, output.options().dtype(at::kFloat));
  float* ca = coefs.data_ptr<float>();
  float* cb = ca + L.C;
  float* cd = cb + L.C;
  const int cgrid = (int)cdiv(L.C, MSBN_BLOCK);
  MSBN_DISPATCH_RSTAT(affine_type(weight, bias), "bn_bwd_elemt_inplace", [&] {
    const rstat_t* w =
        weight.has_value() && weight->defined()
            ? reinterpret_cast<const rstat_t*>(weight->data_ptr())
            : nullptr;
    const rstat_t* b = bias.has_value() && bias->defined()
                           ? reinterpret_cast<const rstat_t*>(bias->data_ptr())
                           : nullptr;
    hipLaunchKernelGGL((bn_affine_bwd<rstat_t>), dim3(cgrid), dim3(MSBN_BLOCK),
                       0, stream, mean.data_ptr<float>(),
                       invstd.data_ptr<float>(), w, sum_dy.data_ptr<float>(),
                       sum_dy_xmu.data_ptr<float>(),
                       count_sum.data_ptr<float>(), L.C, ca, cb, cd);
    hipLaunchKernelGGL((bn_inplace_bwd_coefs<rstat_t>), dim3(cgrid),
                       dim3(MSBN_BLOCK), 0, stream, invstd.data_ptr<float>(),
                       w, b, sum_dy.data_ptr<float>(),
                       count_sum.data_ptr<float>(), L.C, ca, cb, cd);
  });

  const int64_t total = output.numel();
  MSBN_DISPATCH_FLOAT_TYPES(output.scalar_type(), "bn_bwd_elemt_inplace", [&] {
    const native_t* y =
        reinterpret_cast<const native_t*>(output.data_ptr<scalar_t>());
    const native_t* dy =
        reinterpret_cast<const native_t*>(grad_out.data_ptr<scalar_t>());
    native_t* o = reinterpret_cast<native_t*>(dx.data_ptr<scalar_t>());
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    // ca / cb / cd are this op's own aligned buffer: C % V == 0 (pick_v)
    // keeps every V-float pack of them aligned
    const ElemtPlan plan =
        plan_elemt(L, total, (int)sizeof(native_t), {y, dy, o}, nullptr);
    MSBN_DISPATCH_V(plan.v, VMAX, [&] {
      auto launch = [&](auto act_c) {
        constexpr int ACT_ = decltype(act_c)::value;
        if (!L.nhwc) {
          hipLaunchKernelGGL((bn_bwd_elemt_inplace_nchw<native_t, VV, ACT_>),
                             dim3(plan.grid), dim3(MSBN_BLOCK), 0, stream, dy,
                             y, o, ca, cb, cd, total, L.C, L.S, slope,
                             inv_slope);
        } else {
          hipLaunchKernelGGL((bn_bwd_elemt_inplace_nhwc<native_t, VV, ACT_>),
                             dim3(plan.grid), dim3(MSBN_BLOCK), 0, stream, dy,
                             y, o, ca, cb, cd, total, L.C, slope, inv_slope);
        }
      };
      if (mode == kActLeaky) launch(ActC<kActLeaky>{});
      else launch(ActC<kActNone>{});
    });
  });
  return dx;
}

// ---------------------------------------------------------------------------
// frozen path (running-stat normalization with autograd on)
// ---------------------------------------------------------------------------
at::Tensor bn_frozen_coefs(const at::Tensor& running_mean,
                           const at::Tensor& running_var, double eps,
                           const c10::optional<at::Tensor>& weight,
                           const c10::optional<at::Tensor>& bias) {
  const int64_t C = running_mean.numel();
  TORCH_CHECK(running_mean.dim() == 1 && running_mean.is_contiguous() &&
                  running_var.is_contiguous() &&
                  running_var.sizes() == running_mean.sizes() &&
                  running_var.scalar_type() == running_mean.scalar_type(),
              "bn_frozen_coefs: running_mean / running_var must be matching "
              "contiguous [C] tensors");
  const bool has_w = weight.has_value() && weight->defined();
  const bool has_b = bias.has_value() && bias->defined();
  TORCH_CHECK(!has_w || (weight->numel() == C && weight->is_contiguous()),
              "bn_frozen_coefs: weight must be contiguous [C]");
  TORCH_CHECK(!has_b || (bias->numel() == C && bias->is_contiguous()),
              "bn_frozen_coefs: bias must be contiguous [C]");
  TORCH_CHECK(!has_w || !has_b ||
                  weight->scalar_type() == bias->scalar_type(),
              "bn_frozen_coefs: weight and bias dtypes differ");
  auto coefs = at::empty({2 * C}, running_mean.options().dtype(at::kFloat));
  if (C == 0) return coefs;
  float* scale = coefs.data_ptr<float>();
  float* shift = scale + C;
  auto stream = cur_stream();
  const int cgrid = (int)cdiv(C, MSBN_BLOCK);
  const auto w_type = has_w   ? weight->scalar_type()
                      : has_b ? bias->scalar_type()
                              : at::kFloat;
  MSBN_DISPATCH_RSTAT(running_mean.scalar_type(), "bn_frozen_coefs", [&] {
    MSBN_DISPATCH_WTYPE(w_type, "bn_frozen_coefs", [&] {
      const rstat_t* rm =
          reinterpret_cast<const rstat_t*>(running_mean.data_ptr());
      const rstat_t* rv =
          reinterpret_cast<const rstat_t*>(running_var.data_ptr());
      const wt_t* wp =
          has_w ? reinterpret_cast<const wt_t*>(weight->data_ptr()) : nullptr;
      const wt_t* bp =
          has_b ? reinterpret_cast<const wt_t*>(bias->data_ptr()) : nullptr;
      hipLaunchKernelGGL((bn_frozen_coefs<rstat_t, wt_t>), dim3(cgrid),
                         dim3(MSBN_BLOCK), 0, stream, rm, rv, (float)eps, wp,
                         bp, C, scale, shift);
    });
  });
  return coefs;
}

std::tuple<at::Tensor, at::Tensor> batch_norm_frozen_backward_elemt(
    const at::Tensor& grad_out, const c10::optional<at::Tensor>& input,
    const c10::optional<at::Tensor>& residual, const at::Tensor& coefs,
    bool relu_mask, bool want_input_grad, bool want_res_grad,
    double negative_slope) {
  const float slope = (float)negative_slope;
  TORCH_CHECK(grad_out.dim() >= 2,
              "batch_norm_frozen_backward_elemt: grad_out must be >= 2-D");
  const Layout L = get_layout(grad_out);
  // every tensor is indexed with grad_out's dense layout
  auto same_layout = [&](const at::Tensor& t) {
    if (t.sizes() != grad_out.sizes() ||
        t.scalar_type() != grad_out.scalar_type())
      return false;
    if (t.strides() == grad_out.strides()) return true;
    if (!L.nhwc) return t.is_contiguous();
    return t.is_contiguous(grad_out.dim() == 4
                               ? at::MemoryFormat::ChannelsLast
                               : at::MemoryFormat::ChannelsLast3d);
  };
  const bool has_x = input.has_value() && input->defined();
  const bool has_res = relu_mask && residual.has_value() && residual->defined();
  TORCH_CHECK(!relu_mask || has_x,
              "batch_norm_frozen_backward_elemt: relu_mask needs the input");
  TORCH_CHECK(!relu_mask || same_layout(*input),
              "input must match grad_out shape/strides/dtype");
  TORCH_CHECK(!has_res || same_layout(*residual),
              "residual must match grad_out shape/strides/dtype");
  TORCH_CHECK(coefs.scalar_type() == at::kFloat && coefs.is_contiguous() &&
                  coefs.numel() == 2 * L.C,
              "coefs must be contiguous fp32 [2C] ([scale | shift])");

  at::Tensor dx, dres;
  // without the gate the residual branch's gradient IS grad_out
  const bool resg = want_res_grad && relu_mask;
  if (want_res_grad && !relu_mask) dres = grad_out;
  if (want_input_grad) dx = at::empty_like(grad_out);
  if (resg) dres = at::empty_like(grad_out);
  if (grad_out.numel() == 0 || (!want_input_grad && !resg)) return {dx, dres};

  auto stream = cur_stream();
  const float* scale = coefs.data_ptr<float>();
  const float* shift = scale + L.C;
  const int64_t total = grad_out.numel();
  MSBN_DISPATCH_FLOAT_TYPES(grad_out.scalar_type(), "bn_frozen_bwd_elemt", [&] {
    const native_t* dy =
        reinterpret_cast<const native_t*>(grad_out.data_ptr<scalar_t>());
    const native_t* x =
        relu_mask ? reinterpret_cast<const native_t*>(input->data_ptr())
                  : nullptr;
    const native_t* res =
        has_res ? reinterpret_cast<const native_t*>(residual->data_ptr())
                : nullptr;
    native_t* o = want_input_grad
                      ? reinterpret_cast<native_t*>(dx.data_ptr<scalar_t>())
                      : nullptr;
    native_t* dr =
        resg ? reinterpret_cast<native_t*>(dres.data_ptr<scalar_t>())
             : nullptr;
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    // every pointer the launch touches (absent ones are nullptr); NHWC
    // packs load V fp32 coefficients at once, hence `scale`
    const ElemtPlan plan = plan_elemt(L, total, (int)sizeof(native_t),
                                      {dy, x, res, o, dr}, scale);
    const int v = plan.v;
    const int grid = plan.grid;
    MSBN_DISPATCH_V(v, VMAX, [&] {
      auto launch = [&](auto act_c, auto res_c, auto resg_c) {
        constexpr int ACT_ = decltype(act_c)::value;
        constexpr bool RES_ = decltype(res_c)::value;
        constexpr bool RESG_ = decltype(resg_c)::value;
        if (!L.nhwc) {
          hipLaunchKernelGGL(
              (bn_frozen_bwd_elemt_nchw<native_t, VV, ACT_, RES_, RESG_>),
              dim3(grid), dim3(MSBN_BLOCK), 0, stream, dy, x, res, o, dr,
              scale, shift, total, L.C, L.S, slope);
        } else {
          hipLaunchKernelGGL(
              (bn_frozen_bwd_elemt_nhwc<native_t, VV, ACT_, RES_, RESG_>),
              dim3(grid), dim3(MSBN_BLOCK), 0, stream, dy, x, res, o, dr,
              scale, shift, total, L.C, slope);
        }
      };
      using T = std::true_type;
      using F = std::false_type;
      auto gated = [&](auto act_c) {
        if (has_res && resg) launch(act_c, T{}, T{});
        else if (has_res) launch(act_c, T{}, F{});
        else if (resg) launch(act_c, F{}, T{});
        else launch(act_c, F{}, F{});
      };
      if (!relu_mask) launch(ActC<kActNone>{}, F{}, F{});
      else if (slope == 0.f) gated(ActC<kActRelu>{});
      else gated(ActC<kActLeaky>{});
    });
  });
  return {dx, dres};
}

// ---------------------------------------------------------------------------
// small-plane world-1 fused path (single-launch forward / backward)
// ---------------------------------------------------------------------------
namespace {
// Measured crossover (tools/fused_local_bench.py, gpurun_out/flb_*.log):
// block-per-channel wins up to plane ~8K elems (128bs x 8x8 and smaller);
// beyond that a single block serializes too much plane work and the
// two-stage chip-filling pipeline wins (3.4x at plane 32K).
constexpr int64_t kFusedSmallPlaneMax = 8192;
constexpr int64_t kFusedSmallMinC = 64;  // >= 64 blocks on the grid

bool fp32_or_absent(const c10::optional<at::Tensor>& t) {
  return !t.has_value() || !t->defined() || t->scalar_type() == at::kFloat;
}
}  // namespace

bool bn_fused_local_eligible(const at::Tensor& input,
                             const c10::optional<at::Tensor>& weight,
                             const c10::optional<at::Tensor>& bias,
                             const c10::optional<at::Tensor>& running_mean,
                             const c10::optional<at::Tensor>& running_var) {
  if (!input.is_cuda() || input.dim() < 2 || input.numel() == 0) return false;
  const auto st = input.scalar_type();
  if (st != at::kFloat && st != at::kBFloat16 && st != at::kHalf) return false;
  if (!input.is_contiguous()) return false;  // NCHW only
  // a 4-D tensor that REPORTS channels-last gets the NHWC kernels instead
  if (input.dim() >= 4 &&
      input.suggest_memory_format() == at::MemoryFormat::ChannelsLast)
    return false;
  const int64_t C = input.size(1);
  const int64_t N = input.size(0);
  const int64_t plane = input.numel() / C;
  const int64_t S = plane / std::max<int64_t>(N, 1);
  const int vmax = 16 / (int)input.element_size();
  const bool vec = (S % vmax) == 0;
  // vectorized blocks chew 4-8x more plane per cycle -> higher crossover
  // (measured: win at 16K, slight loss at 32K — gpurun_out/flb2.log)
  const int64_t lim = vec ? 2 * kFusedSmallPlaneMax : kFusedSmallPlaneMax;
  if (C < kFusedSmallMinC || plane > lim) return false;
  return fp32_or_absent(weight) && fp32_or_absent(bias) &&
         fp32_or_absent(running_mean) && fp32_or_absent(running_var);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_fwd_fused_local(const at::Tensor& input,
                           const c10::optional<at::Tensor>& residual,
                           const c10::optional<at::Tensor>& weight,
                           const c10::optional<at::Tensor>& bias, double eps,
                           double momentum,
                           const c10::optional<at::Tensor>& running_mean,
                           const c10::optional<at::Tensor>& running_var,
                           bool relu, double negative_slope) {
  const float slope = (float)negative_slope;
  const int64_t C = input.size(1);
  const int64_t N = input.size(0);
  const int64_t S = input.numel() / std::max<int64_t>(N * C, 1);
  auto opts = input.options().dtype(at::kFloat);
  auto mean = at::empty({C}, opts);
  auto invstd = at::empty({C}, opts);
  auto count = at::empty({1}, opts);
  auto coefs = at::empty({2 * C}, opts);
  auto y = at::empty_like(input);
  auto stream = cur_stream();
  const bool has_res = residual.has_value() && residual->defined();
  TORCH_CHECK(!has_res || residual->is_contiguous(),
              "fused local: residual must match NCHW layout");
  float* rm = running_mean.has_value() && running_mean->defined()
                  ? running_mean->data_ptr<float>()
                  : nullptr;
  float* rv = running_var.has_value() && running_var->defined()
                  ? running_var->data_ptr<float>()
                  : nullptr;
  const float* w = weight.has_value() && weight->defined()
                       ? weight->data_ptr<float>()
                       : nullptr;
  const float* b =
      bias.has_value() && bias->defined() ? bias->data_ptr<float>() : nullptr;
  float* scale_p = coefs.data_ptr<float>();
  float* shift_p = scale_p + C;
  MSBN_DISPATCH_FLOAT_TYPES(input.scalar_type(), "bn_fwd_fused_local", [&] {
    const native_t* x =
        reinterpret_cast<const native_t*>(input.data_ptr<scalar_t>());
    const native_t* res =
        has_res ? reinterpret_cast<const native_t*>(
                      residual->data_ptr<scalar_t>())
                : nullptr;
    native_t* yp = reinterpret_cast<native_t*>(y.data_ptr<scalar_t>());
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    const int v = pick_v((int)sizeof(native_t), {x, res, yp}, S);
    MSBN_DISPATCH_V(v, VMAX, [&] {
      MSBN_DISPATCH_ACT(act_mode(relu, slope), ACT_, [&] {
        MSBN_DISPATCH_BOOL(has_res, RES_, [&] {
          hipLaunchKernelGGL(
              (bn_fwd_fused_small_nchw<native_t, VV, ACT_, RES_>),
              dim3((unsigned)C), dim3(MSBN_BLOCK), 0, stream, x, res, yp,
              (int)N, C, (int)S, (float)eps, (float)momentum,
              mean.data_ptr<float>(), invstd.data_ptr<float>(),
              count.data_ptr<float>(), rm, rv, w, b, scale_p, shift_p, slope);
        });
      });
    });
  });
  return {y, mean, invstd, count, coefs};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_bwd_fused_local(const at::Tensor& grad_out, const at::Tensor& input,
                           const c10::optional<at::Tensor>& residual,
                           const at::Tensor& mean, const at::Tensor& invstd,
                           const c10::optional<at::Tensor>& weight,
                           const c10::optional<at::Tensor>& coefs,
                           bool relu_mask, bool want_res_grad, bool weight_g,
                           bool bias_g, double negative_slope) {
  const float slope = (float)negative_slope;
  const int64_t C = input.size(1);
  const int64_t N = input.size(0);
  const int64_t S = input.numel() / std::max<int64_t>(N * C, 1);
  TORCH_CHECK(grad_out.is_contiguous(), "fused local bwd: grad layout");
  TORCH_CHECK(!relu_mask || (coefs.has_value() && coefs->defined()),
              "fused local bwd: relu mask needs coefs");
  auto opts = input.options().dtype(at::kFloat);
  auto dx = at::empty_like(input);
  at::Tensor gw, gb, dres;
  if (weight_g) gw = at::empty({C}, opts);
  if (bias_g) gb = at::empty({C}, opts);
  if (want_res_grad) dres = at::empty_like(grad_out);
  auto stream = cur_stream();
  const bool has_res = residual.has_value() && residual->defined();
  const float* scale_p = nullptr;
  const float* shift_p = nullptr;
  if (relu_mask) {
    scale_p = coefs->data_ptr<float>();
    shift_p = scale_p + C;
  }
  const float* w = weight.has_value() && weight->defined()
                       ? weight->data_ptr<float>()
                       : nullptr;
  MSBN_DISPATCH_FLOAT_TYPES(input.scalar_type(), "bn_bwd_fused_local", [&] {
    const native_t* dy =
        reinterpret_cast<const native_t*>(grad_out.data_ptr<scalar_t>());
    const native_t* x =
        reinterpret_cast<const native_t*>(input.data_ptr<scalar_t>());
    const native_t* res =
        (relu_mask && has_res)
            ? reinterpret_cast<const native_t*>(residual->data_ptr<scalar_t>())
            : nullptr;
    native_t* dxp = reinterpret_cast<native_t*>(dx.data_ptr<scalar_t>());
    native_t* drp = want_res_grad
                        ? reinterpret_cast<native_t*>(dres.data_ptr<scalar_t>())
                        : nullptr;
    constexpr int VMAX = 16 / (int)sizeof(native_t);
    const int v =
        pick_v((int)sizeof(native_t), {dy, x, res, dxp, drp}, S);
    MSBN_DISPATCH_V(v, VMAX, [&] {
      auto launch = [&](auto act_c, auto res_c, auto resg_c) {
        hipLaunchKernelGGL(
            (bn_bwd_fused_small_nchw<native_t, VV, decltype(act_c)::value,
                                     decltype(res_c)::value,
                                     decltype(resg_c)::value>),
            dim3((unsigned)C), dim3(MSBN_BLOCK), 0, stream, dy, x, res, dxp,
            drp, mean.data_ptr<float>(), invstd.data_ptr<float>(), scale_p,
            shift_p, w, weight_g ? gw.data_ptr<float>() : nullptr,
            bias_g ? gb.data_ptr<float>() : nullptr, (int)N, C, (int)S,
            slope);
      };
      using T = std::true_type;
      using F = std::false_type;
      auto gated = [&](auto act_c) {
        if (has_res && want_res_grad) launch(act_c, T{}, T{});
        else if (has_res) launch(act_c, T{}, F{});
        else if (want_res_grad) launch(act_c, F{}, T{});
        else launch(act_c, F{}, F{});
      };
      if (!relu_mask) {
        if (want_res_grad) launch(ActC<kActNone>{}, F{}, T{});
        else launch(ActC<kActNone>{}, F{}, F{});
      } else if (slope == 0.f) {
        gated(ActC<kActRelu>{});
      } else {
        gated(ActC<kActLeaky>{});
      }
    });
  });
  return {dx, gw, gb, dres};
}

// ---------------------------------------------------------------------------
// dual BN: relu(bn(x) + bn_d(x_d)) (kernels: "dual BN" above)
// ---------------------------------------------------------------------------
namespace {
// the dual kernels exist for the two 2-byte dtypes only
#define MSBN_DISPATCH_HALF_TYPES(TYPE, NAME, ...)                           \
  [&] {                                                                     \
    switch (TYPE) {                                                         \
      case at::kBFloat16: {                                                 \
        using native_t = __hip_bfloat16;                                    \
        return __VA_ARGS__();                                               \
      }                                                                     \
      case at::kHalf: {                                                     \
        using native_t = __half;                                            \
        return __VA_ARGS__();                                               \
      }                                                                     \
      default:                                                              \
        TORCH_CHECK(false, NAME, ": unsupported dtype ", TYPE);             \
    }                                                                       \
  }()

// What the dual kernels take: a non-empty dense channels-last 4-D bf16 / half
// tensor on the GPU with C a multiple of 8.  Alignment is the plans' business.
bool dual_tensor_ok(const at::Tensor& x) {
  if (!x.is_cuda() || x.dim() != 4 || x.numel() == 0) return false;
  if (x.scalar_type() != at::kBFloat16 && x.scalar_type() != at::kHalf)
    return false;
  if (x.suggest_memory_format() != at::MemoryFormat::ChannelsLast ||
      !x.is_contiguous(at::MemoryFormat::ChannelsLast))
    return false;
  return x.size(1) % 8 == 0;
}

bool dual_same(const at::Tensor& t, const at::Tensor& x) {
  return t.defined() && t.sizes() == x.sizes() && t.strides() == x.strides() &&
         t.scalar_type() == x.scalar_type() && t.device() == x.device();
}

bool dual_coef_ok(const at::Tensor& c, int64_t rows, int64_t C,
                  const at::Tensor& x) {
  return c.defined() && c.scalar_type() == at::kFloat && c.is_contiguous() &&
         c.numel() == rows * C && c.device() == x.device() &&
         ((uintptr_t)c.data_ptr() % (8 * sizeof(float))) == 0;
}

// The reduce runs on the plan the single gated reduce takes for these
// pointers (x2 is one more pack pointer); declined unless that is V = 8.
bool dual_reduce_plan(const at::Tensor& x, const at::Tensor& x2,
                      const at::Tensor& dy, const at::Tensor& gm,
                      const c10::optional<at::Tensor>& dy2, ReducePlan* out) {
  if (!dual_tensor_ok(x) || !dual_same(x2, x) || !dual_same(dy, x) ||
      !dual_same(gm, x))
    return false;
  if (dy2.has_value() && !dual_same(*dy2, x)) return false;
  const Layout L = get_layout(x);
  const ReducePlan p = plan_reduce(
      L, 2,
      {x.data_ptr(), dy.data_ptr(), x2.data_ptr(), gm.data_ptr(),
       dy2.has_value() ? dy2->data_ptr() : nullptr});
  if (p.path != RedPath::Nhwc || p.v != 8) return false;
  *out = p;
  return true;
}

bool dual_elemt_plan(const at::Tensor& x,
                     c10::ArrayRef<const at::Tensor*> same, ElemtPlan* out) {
  if (!dual_tensor_ok(x)) return false;
  std::vector<const void*> ptrs{x.data_ptr()};
  for (const at::Tensor* t : same) {
    if (!dual_same(*t, x)) return false;
    ptrs.push_back(t->data_ptr());
  }
  const ElemtPlan p = plan_elemt(get_layout(x), x.numel(), 2, ptrs, nullptr);
  if (p.v != 8) return false;
  *out = p;
  return true;
}
}  // namespace

std::tuple<at::Tensor, bool> batch_norm_elemt_act_dual(
    const at::Tensor& input, const at::Tensor& input2, const at::Tensor& coefs,
    const at::Tensor& coefs2, bool relu, double negative_slope,
    const at::Tensor& gate_out) {
  ElemtPlan plan{};
  if (!relu || negative_slope != 0.0 ||
      !dual_elemt_plan(input, {&input2}, &plan))
    return {at::Tensor(), false};
  const int64_t C = input.size(1);
  if (!dual_coef_ok(coefs, 2, C, input) || !dual_coef_ok(coefs2, 2, C, input))
    return {at::Tensor(), false};
  check_gate_tensor(gate_out, input, "gate_out");
  auto out = at::empty_like(input);  // allocator-aligned
  const int64_t total = input.numel();
  auto stream = cur_stream();
  const float* sc = coefs.data_ptr<float>();
  const float* sc2 = coefs2.data_ptr<float>();
  MSBN_DISPATCH_HALF_TYPES(input.scalar_type(), "bn_elemt_dual", [&] {
    hipLaunchKernelGGL(
        (bn_elemt_dual_nhwc<native_t>), dim3(plan.grid), dim3(MSBN_BLOCK), 0,
        stream, reinterpret_cast<const native_t*>(input.data_ptr()),
        reinterpret_cast<const native_t*>(input2.data_ptr()),
        reinterpret_cast<native_t*>(out.data_ptr()), sc, sc + C, sc2, sc2 + C,
        total, C, gate_out.data_ptr<unsigned char>());
  });
  return {out, true};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_backward_reduce_act_dual(
    const at::Tensor& grad_out, const at::Tensor& input,
    const at::Tensor& input2, const at::Tensor& mean, const at::Tensor& mean2,
    const at::Tensor& invstd, const at::Tensor& invstd2,
    const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& weight2, bool weight_g, bool bias_g,
    bool weight2_g, bool bias2_g, const at::Tensor& gm_out,
    const c10::optional<at::Tensor>& grad_out2, const at::Tensor& gate) {
  TORCH_CHECK(input.dim() >= 2 && input2.sizes() == input.sizes(),
              "input2 must match input");
  const int64_t C = input.size(1);
  auto f32 = input.options().dtype(at::kFloat);
  ReducePlan plan{};
  if (!dual_reduce_plan(input, input2, grad_out, gm_out, grad_out2, &plan)) {
    // declined (a gradient off alignment, ...): the composition's two
    // reduces, packed into the same message
    auto r1 = msbn::batch_norm_backward_reduce_act(
        grad_out, input, c10::nullopt, mean, invstd, weight, c10::nullopt,
        true, true, weight_g, bias_g, c10::nullopt, gm_out, 0.0, grad_out2,
        gate);
    auto r2 = msbn::batch_norm_backward_reduce(
        gm_out, input2, mean2, invstd2, weight2, true, weight2_g, bias2_g);
    auto sums = at::cat({std::get<0>(r1), std::get<1>(r1), std::get<0>(r2),
                         std::get<1>(r2)});
    return {sums, std::get<2>(r1), std::get<3>(r1), std::get<2>(r2),
            std::get<3>(r2)};
  }
  check_gate_tensor(gate, input, "gate");
  const Layout L = get_layout(input);
  // ONE contiguous buffer [sum_dy | sum_dy_xmu | sum_dy_2 | sum_dy_xmu_2]
  auto sums = at::empty({4 * C}, f32);
  float* sp = sums.data_ptr<float>();
  auto affine = [&](const c10::optional<at::Tensor>& w, bool on) {
    return on ? at::empty({C}, input.options().dtype(
                                   w.has_value() ? w->scalar_type()
                                                 : input.scalar_type()))
              : at::Tensor();
  };
  at::Tensor gw = affine(weight, weight_g), gb = affine(weight, bias_g);
  at::Tensor gw2 = affine(weight2, weight2_g), gb2 = affine(weight2, bias2_g);
  const int nchunks = plan.nchunks;
  at::Tensor ws = at::empty({2, (int64_t)nchunks * C * 2},
                            input.options().dtype(at::kDouble));
  double* ws1 = ws.data_ptr<double>();
  double* ws2 = ws1 + (int64_t)nchunks * C * 2;
  const bool has_dy2 = grad_out2.has_value();
  auto stream = cur_stream();
  MSBN_DISPATCH_HALF_TYPES(input.scalar_type(), "bn_bwd_reduce_dual", [&] {
    const auto& g = plan.nhwc;
    MSBN_DISPATCH_BOOL(has_dy2, DY2_, [&] {
      hipLaunchKernelGGL(
          (bn_bwd_reduce_dual_partial_nhwc<native_t, DY2_>), g.grid,
          dim3(MSBN_BLOCK), 0, stream,
          reinterpret_cast<const native_t*>(grad_out.data_ptr()),
          has_dy2 ? reinterpret_cast<const native_t*>(grad_out2->data_ptr())
                  : nullptr,
          reinterpret_cast<const native_t*>(input.data_ptr()),
          reinterpret_cast<const native_t*>(input2.data_ptr()),
          reinterpret_cast<native_t*>(gm_out.data_ptr()),
          mean.data_ptr<float>(), mean2.data_ptr<float>(), ws1, ws2, L.rows,
          L.C, g.chunk_rows, g.lpr, gate.data_ptr<unsigned char>());
    });
  });
  const int fgrid = (int)cdiv(C, kFinalizeWavesPerBlock);
  auto finalize = [&](const double* w, const at::Tensor& istd, float* s,
                      at::Tensor& gwt, at::Tensor& gbt, at::ScalarType wt) {
    MSBN_DISPATCH_RSTAT(wt, "bn_bwd_reduce_dual", [&] {
      hipLaunchKernelGGL(
          (bn_bwd_reduce_finalize<rstat_t>), dim3(fgrid), dim3(MSBN_BLOCK), 0,
          stream, w, nchunks, C, istd.data_ptr<float>(), s, s + C,
          gwt.defined() ? reinterpret_cast<rstat_t*>(gwt.data_ptr()) : nullptr,
          gbt.defined() ? reinterpret_cast<rstat_t*>(gbt.data_ptr())
                        : nullptr);
    });
  };
  finalize(ws1, invstd, sp, gw, gb,
           weight.has_value() ? weight->scalar_type() : input.scalar_type());
  finalize(ws2, invstd2, sp + 2 * C, gw2, gb2,
           weight2.has_value() ? weight2->scalar_type() : input.scalar_type());
  return {sums, gw, gb, gw2, gb2};
}

std::tuple<at::Tensor, at::Tensor> batch_norm_backward_elemt_dual(
    const at::Tensor& gm, const at::Tensor& input, const at::Tensor& input2,
    const at::Tensor& mean, const at::Tensor& mean2, const at::Tensor& invstd,
    const at::Tensor& invstd2, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& weight2, const at::Tensor& sums,
    const at::Tensor& count) {
  ElemtPlan plan{};
  TORCH_CHECK(dual_elemt_plan(input, {&input2, &gm}, &plan),
              "batch_norm_backward_elemt_dual: needs dense channels-last "
              "bf16 / half tensors, C a multiple of 8, 16-byte aligned");
  const int64_t C = input.size(1);
  TORCH_CHECK(sums.scalar_type() == at::kFloat && sums.is_contiguous() &&
                  sums.numel() == 4 * C,
              "sums must be the contiguous fp32 [4C] buffer of the dual "
              "reduce");
  auto dx = at::empty_like(input);
  auto dx2 = at::empty_like(input);
  at::Tensor count_sum;
  if (count.numel() == 1 && count.scalar_type() == at::kFloat) {
    count_sum = count;
  } else {
    count_sum = count.to(at::kFloat).sum().reshape({1});
  }
  auto stream = cur_stream();
  // [a | b | d] of the main layer, then of the skip layer (allocator-aligned;
  // 3C floats is a multiple of 32 bytes since C % 8 == 0)
  auto co = at::empty({6 * C}, input.options().dtype(at::kFloat));
  float* co1 = co.data_ptr<float>();
  float* co2 = co1 + 3 * C;
  const float* sp = sums.data_ptr<float>();
  const int cgrid = (int)cdiv(C, MSBN_BLOCK);
  auto affine = [&](const at::Tensor& mu, const at::Tensor& istd,
                    const c10::optional<at::Tensor>& w, const float* s,
                    float* o) {
    const auto wtype = w.has_value() ? w->scalar_type() : at::kFloat;
    MSBN_DISPATCH_RSTAT(wtype, "bn_bwd_elemt_dual", [&] {
      hipLaunchKernelGGL(
          (bn_affine_bwd<rstat_t>), dim3(cgrid), dim3(MSBN_BLOCK), 0, stream,
          mu.data_ptr<float>(), istd.data_ptr<float>(),
          w.has_value() ? reinterpret_cast<const rstat_t*>(w->data_ptr())
                        : nullptr,
          s, s + C, count_sum.data_ptr<float>(), C, o, o + C, o + 2 * C);
    });
  };
  affine(mean, invstd, weight, sp, co1);
  affine(mean2, invstd2, weight2, sp + 2 * C, co2);
  MSBN_DISPATCH_HALF_TYPES(input.scalar_type(), "bn_bwd_elemt_dual", [&] {
    hipLaunchKernelGGL(
        (bn_bwd_elemt_dual_nhwc<native_t>), dim3(plan.grid), dim3(MSBN_BLOCK),
        0, stream, reinterpret_cast<const native_t*>(gm.data_ptr()),
        reinterpret_cast<const native_t*>(input.data_ptr()),
        reinterpret_cast<const native_t*>(input2.data_ptr()),
        reinterpret_cast<native_t*>(dx.data_ptr()),
        reinterpret_cast<native_t*>(dx2.data_ptr()), co1, co2, input.numel(),
        C);
  });
  return {dx, dx2};
}

// ---------------------------------------------------------------------------
// launch_plan: host-only; launches nothing.  Reports, from the SAME helpers
// the ops launch with (get_layout, plan_reduce / plan_elemt -> pick_v, *_grid,
// bn_fused_local_eligible), which kernel path a call would take and how far
// its loops run.  Output tensors the ops allocate themselves are taken as
// allocator-aligned.
// ---------------------------------------------------------------------------
std::tuple<std::string, std::map<std::string, int64_t>> launch_plan(
    const std::string& kind, const at::Tensor& input,
    const std::vector<c10::optional<at::Tensor>>& others,
    const c10::optional<at::Tensor>& coefs) {
  TORCH_CHECK(input.dim() >= 2 && input.numel() > 0,
              "launch_plan: input must be a non-empty >= 2-D tensor");
  const int esize = (int)input.element_size();
  TORCH_CHECK(esize == 2 || esize == 4, "launch_plan: unsupported dtype");
  // gate bits: the optional last entry of "elemt" (others[1]) and
  // "bwd_reduce" (others[4]).  Bytes, so never among the pack pointers.
  const size_t gate_at = kind == "elemt"        ? 1
                         : kind == "bwd_reduce" ? 4
                                                : others.size();
  auto given = [&](size_t i) {
    return i < others.size() && others[i].has_value() && others[i]->defined();
  };
  std::vector<const void*> ptrs{input.data_ptr()};
  for (size_t i = 0; i < others.size(); ++i)
    if (i != gate_at && given(i)) ptrs.push_back(others[i]->data_ptr());
  const float* coef = coefs.has_value() && coefs->defined()
                          ? coefs->data_ptr<float>()
                          : nullptr;
  std::map<std::string, int64_t> d;
  std::string path;

  // dual BN: the single counterparts' numbers plus "dual", or "ineligible"
  // where the ops decline and the composition runs
  if (kind == "elemt_dual" || kind == "bwd_elemt_dual") {
    // elemt_dual: others = {x2[, coefs2]}; bwd_elemt_dual: others = {gm, x2}
    const bool fwd = kind == "elemt_dual";
    ElemtPlan p{};
    bool ok = given(0);
    if (ok && fwd) {
      const int64_t C = input.size(1);
      ok = dual_elemt_plan(input, {&*others[0]}, &p) &&
           (!coefs.has_value() || dual_coef_ok(*coefs, 2, C, input)) &&
           (!given(1) || dual_coef_ok(*others[1], 2, C, input));
    } else if (ok) {
      ok = given(1) && dual_elemt_plan(input, {&*others[0], &*others[1]}, &p);
    }
    if (!ok) return {"ineligible", d};
    const int64_t threads = (int64_t)p.grid * MSBN_BLOCK;
    d["V"] = p.v;
    d["grid"] = p.grid;
    d["packs"] = p.packs;
    d["trips"] = cdiv(p.packs, threads);
    d["multi_trip"] = p.packs > threads ? 1 : 0;
    d["dual"] = 1;
    return {"nhwc", d};
  }
  if (kind == "bwd_reduce_dual") {
    // others = {grad_out, x2, gm_out, grad_out2, gate}
    ReducePlan p{};
    const bool ok =
        given(0) && given(1) && given(2) && given(4) &&
        dual_reduce_plan(input, *others[1], *others[0], *others[2],
                         given(3) ? others[3] : c10::optional<at::Tensor>(),
                         &p);
    if (!ok) return {"ineligible", d};
    d["V"] = p.v;
    d["nchunks"] = p.nchunks;
    d["trips"] = p.trips;
    d["flush_every"] = p.flush_every;
    d["finalize_trips"] = cdiv(p.nchunks, MSBN_WAVE);
    d["chunk_rows"] = p.nhwc.chunk_rows;
    d["lpr"] = p.nhwc.lpr;
    d["ctiles"] = p.nhwc.grid.x;
    d["gate"] = 1;
    d["dual"] = 1;
    return {"nhwc", d};
  }

  if (kind == "fused_local") {
    if (!bn_fused_local_eligible(input, c10::nullopt, c10::nullopt,
                                 c10::nullopt, c10::nullopt))
      return {"ineligible", d};
    const int64_t C = input.size(1);
    const int64_t plane = input.numel() / C;
    const int64_t S = plane / input.size(0);
    d["V"] = pick_v(esize, ptrs, S);
    d["trips"] = cdiv(plane / d["V"], MSBN_BLOCK);
    d["blocks"] = C;
    return {"small_plane", d};
  }

  const bool pool_kind = kind == "elemt_pool" || kind == "bwd_reduce_pool" ||
                         kind == "bwd_elemt_pool";
  const Layout L =
      pool_kind ? pool_layout(input, "launch_plan") : get_layout(input);
  if (kind == "stats" || kind == "bwd_reduce" ||
      kind == "bwd_reduce_inplace" || kind == "bwd_reduce_pool") {
    const ReducePlan p = plan_reduce(L, esize, ptrs);
    path = p.path == RedPath::Nhwc       ? "nhwc"
           : p.path == RedPath::NchwFlat ? "nchw_flat"
                                         : "nchw_vec";
    d["V"] = p.v;
    d["nchunks"] = p.nchunks;
    d["trips"] = p.trips;
    d["flush_every"] = p.flush_every;
    d["finalize_trips"] = cdiv(p.nchunks, MSBN_WAVE);
    if (p.path == RedPath::NchwVec) {
      d["chunkN"] = p.nchw.chunkN;
      d["chunkS"] = p.nchw.chunkS;
      d["nchunkS"] = p.nchw.grid.z;
    } else if (p.path == RedPath::NchwFlat) {
      d["chunk_len"] = p.flat.chunk_len;
    } else {
      d["chunk_rows"] = p.nhwc.chunk_rows;
      d["lpr"] = p.nhwc.lpr;
      d["ctiles"] = p.nhwc.grid.x;
    }
    // would the bit-reading kernel run (batch_norm_backward_reduce_act's
    // own conditions; the activation is taken as on)
    if (gate_at < others.size())
      d["gate"] = given(gate_at) && !given(1) && given(2) && esize == 2;
    return {path, d};
  }
  TORCH_CHECK(kind == "elemt" || kind == "bwd_elemt" ||
                  kind == "frozen_bwd_elemt" || kind == "elemt_inplace" ||
                  kind == "bwd_elemt_inplace" || kind == "elemt_pool" ||
                  kind == "bwd_elemt_pool",
              "launch_plan: unknown kind '", kind, "'");
  // elemt_pool threads walk the POOLED tensor, one pack of it each
  int64_t total = input.numel();
  if (kind == "elemt_pool") {
    const PoolGeom g = pool_geom(input, L, "launch_plan");
    total = input.size(0) * L.C * g.OH * g.OW;
  }
  const ElemtPlan p = plan_elemt(L, total, esize, ptrs, coef);
  path = L.nhwc ? "nhwc" : (p.v == 1 ? "nchw_flat" : "nchw_vec");
  const int64_t threads = (int64_t)p.grid * MSBN_BLOCK;
  d["V"] = p.v;
  d["grid"] = p.grid;
  d["packs"] = p.packs;
  d["trips"] = cdiv(p.packs, threads);
  d["multi_trip"] = p.packs > threads ? 1 : 0;
  // would the forward store the bits (the activation is taken as on)
  if (gate_at < others.size())
    d["gate"] = given(gate_at) && elemt_writes_gate(kActRelu, given(0), p.v);
  return {path, d};
}

}  // namespace msbn
