// Squeeze-excite fused into the depthwise BatchNorm+SiLU layer (gfx950,
// CDNA4).  docs/KERNEL_DESIGN.md "Squeeze-excite".
//
//   z = scale[c]*y + shift[c]      a = silu(z)  (fp32, never stored)
//   s[n,c] = mean_hw a             h = silu(W1 s + b1)   g = sigmoid(W2 h + b2)
//   out = a * g[n,c]               (one rounding)
//
// Streaming kernels (se_reduce_nhwc, se_scale_nhwc, se_bwd_elemt_nhwc):
//  * channels-last, 16 bytes (8 channels) per lane, nontemporal accesses.
//  * block 256 = lpr lanes across the channel axis x rpi = 256 / lpr thread
//    rows; grid (channel tiles, chunks of one image, images): a block never
//    straddles two images, so g[n, c..c+7], dpool, scale and shift sit in
//    registers for the block's lifetime.
//  * the reduce kernel keeps 3 sums x 8 channels in fp32 for at most
//    MSBN_ACC_FLUSH pixels, then adds them to fp64 registers; thread rows are
//    combined through an LDS tree in a fixed order, one sum at a time
//    (16 KiB); partials go to ws[N][chunks][C][3].  No atomics.
//      forward:  S = sum a,  Q1 = sum silu'(z),  Q2 = sum silu'(z)(y - mean)
//      backward: R = sum dout a, P1 = sum dout silu'(z),
//                P2 = sum dout silu'(z)(y - mean)
// Gate kernels (se_gate_fwd, se_gate_bwd): one block per image.  The image's
// partials are added in chunk order; s (dz2) lives in LDS; the C-long dot
// products take one wave per hidden unit (lanes stride over C, wave64 shuffle
// tree), the Cr-long ones one thread per channel.  A few MFLOP in all: no
// matrix instruction would be kept busy.
// se_bn_finalize_bwd: the gradient entering the BN+SiLU backward is
//   gz = (dout*g[n,c] + dpool[n,c]) * silu'(z),
// so its per-channel sums factor through the per-image tables:
//   sum_dy[c]     = sum_n g*P1 + dpool*Q1
//   sum_dy_xmu[c] = sum_n g*P2 + dpool*Q2
// one wave per channel, lanes stride over n, fp64.  No second pass over
// (dout, y).  se_param_grads: the SE block's own weight / bias gradients, one
// thread per entry, n ascending in fp64, rounded once.
#include "bn_ops.hpp"
#include "common.hpp"
#include "launch_common.hpp"

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <type_traits>

namespace msbn {

namespace {

constexpr int kSeV = 8;         // channels of a lane: one 16-byte pack
constexpr int kSeMaxC = 4096;   // gate kernels: s / dz2 in LDS, fp32
constexpr int kSeMaxCr = 1024;  // gate kernels: h / dz1 in LDS, fp32
constexpr int kSeWaves = MSBN_BLOCK / MSBN_WAVE;

// =====================================================================
// Per-image partial sums.  grid (ctiles, chunks, N) block 256
// y, dout [N][HW][C]; coefs [scale(C) | shift(C)]; ws [N][chunks][C][3]
// =====================================================================
template <typename T, bool BWD>
__global__ __launch_bounds__(MSBN_BLOCK) void se_reduce_nhwc(
    const T* __restrict__ y, const T* __restrict__ dout,
    const float* __restrict__ coefs, const float* __restrict__ mean,
    double* __restrict__ ws, int64_t HW, int C, int chunk_rows, int lpr,
    int nchunks) {
  constexpr int V = kSeV;
  const int rpi = MSBN_BLOCK / lpr;
  const int lane = threadIdx.x & (lpr - 1);
  const int rowoff = threadIdx.x / lpr;
  const int c = (blockIdx.x * lpr + lane) * V;
  const bool inb = c < C;  // C is a multiple of V: a pack is in or out whole
  const int64_t n = blockIdx.z;
  const int64_t p0 = (int64_t)blockIdx.y * chunk_rows;
  const int64_t p1 = i64min(p0 + chunk_rows, HW);

  float f[3][V];
  double t[3][V];
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int k = 0; k < V; ++k) {
      f[q][k] = 0.f;
      t[q][k] = 0.0;
    }
  auto flush = [&]() {
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int k = 0; k < V; ++k) {
        t[q][k] += (double)f[q][k];
        f[q][k] = 0.f;
      }
  };

  if (inb) {
    float sc[V], sh[V], mu[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      sc[k] = coefs[c + k];
      sh[k] = coefs[C + c + k];
      mu[k] = mean[c + k];
    }
    const int64_t img = n * HW * C + c;
    int since_flush = 0;
    for (int64_t p = p0 + rowoff; p < p1; p += rpi) {
      const Pack<T, V> py = nt_load<T, V>(y + img + p * C);
      Pack<T, V> pg;
      if (BWD) pg = nt_load<T, V>(dout + img + p * C);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float xv = to_f(py.v[k]);
        const float z = sc[k] * xv + sh[k];
        const float a = act_fwd<kActSilu>(z, 0.f);
        const float d = BWD ? to_f(pg.v[k]) : 1.f;
        const float gd = act_grad<kActSilu>(z, d, 0.f);
        f[0][k] += BWD ? d * a : a;
        f[1][k] += gd;
        f[2][k] += gd * (xv - mu[k]);
      }
      if (++since_flush == MSBN_ACC_FLUSH) {
        flush();
        since_flush = 0;
      }
    }
    flush();
  }

  // ---- thread rows -> one value per channel, one sum at a time ----
  __shared__ double sdata[V * MSBN_BLOCK];
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int k = 0; k < V; ++k) sdata[k * MSBN_BLOCK + threadIdx.x] = t[q][k];
    for (int st = 1; st < rpi; st <<= 1) {
      __syncthreads();
      if ((rowoff & ((st << 1) - 1)) == 0 && rowoff + st < rpi) {
        const int other = threadIdx.x + st * lpr;
#pragma unroll
        for (int k = 0; k < V; ++k)
          sdata[k * MSBN_BLOCK + threadIdx.x] += sdata[k * MSBN_BLOCK + other];
      }
    }
    __syncthreads();
    if (rowoff == 0 && inb) {
      double* out = ws + ((n * nchunks + blockIdx.y) * C + c) * 3 + q;
#pragma unroll
      for (int k = 0; k < V; ++k) out[k * 3] = sdata[k * MSBN_BLOCK + threadIdx.x];
    }
    __syncthreads();  // the next sum overwrites the planes
  }
}

// =====================================================================
// out = silu(scale*y + shift) * g[n,c].  grid (ctiles, chunks, N) block 256
// =====================================================================
template <typename T>
__global__ __launch_bounds__(MSBN_BLOCK) void se_scale_nhwc(
    const T* __restrict__ y, const float* __restrict__ coefs,
    const float* __restrict__ g, T* __restrict__ out, int64_t HW, int C,
    int chunk_rows, int lpr) {
  constexpr int V = kSeV;
  const int rpi = MSBN_BLOCK / lpr;
  const int lane = threadIdx.x & (lpr - 1);
  const int rowoff = threadIdx.x / lpr;
  const int c = (blockIdx.x * lpr + lane) * V;
  if (c >= C) return;  // no barrier in this kernel
  const int64_t n = blockIdx.z;
  const int64_t p0 = (int64_t)blockIdx.y * chunk_rows;
  const int64_t p1 = i64min(p0 + chunk_rows, HW);
  float sc[V], sh[V], gk[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    sc[k] = coefs[c + k];
    sh[k] = coefs[C + c + k];
    gk[k] = g[n * C + c + k];
  }
  const int64_t img = n * HW * C + c;
#pragma unroll 2
  for (int64_t p = p0 + rowoff; p < p1; p += rpi) {
    const Pack<T, V> py = nt_load<T, V>(y + img + p * C);
    Pack<T, V> po;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float z = sc[k] * to_f(py.v[k]) + sh[k];
      po.v[k] = from_f<T>(act_fwd<kActSilu>(z, 0.f) * gk[k]);
    }
    nt_store<T, V>(out + img + p * C, po);
  }
}

// =====================================================================
// dy = A*gz + B*y + D,  gz = (dout*g[n,c] + dpool[n,c]) * silu'(z)
// grid (ctiles, chunks, N) block 256; abd = [A(C) | B(C) | D(C)]
// =====================================================================
template <typename T>
__global__ __launch_bounds__(MSBN_BLOCK) void se_bwd_elemt_nhwc(
    const T* __restrict__ dout, const T* __restrict__ y,
    const float* __restrict__ coefs, const float* __restrict__ g,
    const float* __restrict__ dpool, const float* __restrict__ abd,
    T* __restrict__ dy, int64_t HW, int C, int chunk_rows, int lpr) {
  constexpr int V = kSeV;
  const int rpi = MSBN_BLOCK / lpr;
  const int lane = threadIdx.x & (lpr - 1);
  const int rowoff = threadIdx.x / lpr;
  const int c = (blockIdx.x * lpr + lane) * V;
  if (c >= C) return;  // no barrier in this kernel
  const int64_t n = blockIdx.z;
  const int64_t p0 = (int64_t)blockIdx.y * chunk_rows;
  const int64_t p1 = i64min(p0 + chunk_rows, HW);
  float sc[V], sh[V], gk[V], dp[V], A[V], B[V], D[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    sc[k] = coefs[c + k];
    sh[k] = coefs[C + c + k];
    gk[k] = g[n * C + c + k];
    dp[k] = dpool[n * C + c + k];
    A[k] = abd[c + k];
    B[k] = abd[C + c + k];
    D[k] = abd[2 * C + c + k];
  }
  const int64_t img = n * HW * C + c;
#pragma unroll 2
  for (int64_t p = p0 + rowoff; p < p1; p += rpi) {
    const Pack<T, V> pg = nt_load<T, V>(dout + img + p * C);
    const Pack<T, V> py = nt_load<T, V>(y + img + p * C);
    Pack<T, V> po;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float xv = to_f(py.v[k]);
      const float z = sc[k] * xv + sh[k];
      const float gz =
          act_grad<kActSilu>(z, to_f(pg.v[k]) * gk[k] + dp[k], 0.f);
      po.v[k] = from_f<T>(A[k] * gz + B[k] * xv + D[k]);
    }
    nt_store<T, V>(dy + img + p * C, po);
  }
}

// a C-long dot product of one wave: lanes stride over C, then the shuffle
// tree; the result is valid on lane 0
template <typename F>
__device__ __forceinline__ float se_wave_dot(int C, int lane, F term) {
  float acc = 0.f;
  for (int c = lane; c < C; c += MSBN_WAVE) acc += term(c);
#pragma unroll
  for (int off = MSBN_WAVE / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, MSBN_WAVE);
  return acc;
}

// the image's three partial sums of channel c, chunks ascending
__device__ __forceinline__ void se_finalize3(const double* __restrict__ ws,
                                             int64_t n, int nchunks, int C,
                                             int c, double (&a)[3]) {
  a[0] = a[1] = a[2] = 0.0;
  for (int j = 0; j < nchunks; ++j) {
    const double* p = ws + ((n * nchunks + j) * C + c) * 3;
    a[0] += p[0];
    a[1] += p[1];
    a[2] += p[2];
  }
}

// =====================================================================
// grid N block 256.  w1 [Cr][C], b1 [Cr], w2 [C][Cr], b2 [C]
// s, g [N][C]; hpre [N][Cr]; q [N][C][2] = {Q1, Q2} (sums, not means)
// =====================================================================
template <typename WT>
__global__ __launch_bounds__(MSBN_BLOCK) void se_gate_fwd(
    const double* __restrict__ ws, const WT* __restrict__ w1,
    const WT* __restrict__ b1, const WT* __restrict__ w2,
    const WT* __restrict__ b2, float* __restrict__ s_out,
    float* __restrict__ hpre_out, float* __restrict__ g_out,
    float* __restrict__ q_out, int64_t HW, int C, int Cr, int nchunks) {
  __shared__ float ls[kSeMaxC];
  __shared__ float lh[kSeMaxCr];
  const int64_t n = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += MSBN_BLOCK) {
    double a[3];
    se_finalize3(ws, n, nchunks, C, c, a);
    const float s = (float)(a[0] / (double)HW);
    ls[c] = s;
    s_out[n * C + c] = s;
    q_out[(n * C + c) * 2] = (float)a[1];
    q_out[(n * C + c) * 2 + 1] = (float)a[2];
  }
  __syncthreads();
  const int lane = threadIdx.x & (MSBN_WAVE - 1);
  for (int j = threadIdx.x >> 6; j < Cr; j += kSeWaves) {  // wave-uniform
    const WT* row = w1 + (int64_t)j * C;
    const float acc =
        se_wave_dot(C, lane, [&](int c) { return to_f(row[c]) * ls[c]; });
    if (lane == 0) {
      const float hp = acc + to_f(b1[j]);
      hpre_out[n * Cr + j] = hp;
      lh[j] = act_fwd<kActSilu>(hp, 0.f);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += MSBN_BLOCK) {
    const WT* row = w2 + (int64_t)c * Cr;
    float acc = 0.f;
    for (int j = 0; j < Cr; ++j) acc += to_f(row[j]) * lh[j];
    g_out[n * C + c] = fast_sigmoid(acc + to_f(b2[c]));
  }
}

// =====================================================================
// grid N block 256.  dz2 = R g (1 - g); dh = W2^T dz2; dz1 = dh silu'(hpre);
// dpool = W1^T dz1 / HW.  p [N][C][2] = {P1, P2}
// =====================================================================
template <typename WT>
__global__ __launch_bounds__(MSBN_BLOCK) void se_gate_bwd(
    const double* __restrict__ ws, const float* __restrict__ g,
    const float* __restrict__ hpre, const WT* __restrict__ w1,
    const WT* __restrict__ w2, float* __restrict__ dpool,
    float* __restrict__ dz2_out, float* __restrict__ dz1_out,
    float* __restrict__ p_out, int64_t HW, int C, int Cr, int nchunks) {
  __shared__ float l2[kSeMaxC];
  __shared__ float l1[kSeMaxCr];
  const int64_t n = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += MSBN_BLOCK) {
    double a[3];
    se_finalize3(ws, n, nchunks, C, c, a);
    const float gv = g[n * C + c];
    const float d2 = (float)a[0] * gv * (1.f - gv);
    l2[c] = d2;
    dz2_out[n * C + c] = d2;
    p_out[(n * C + c) * 2] = (float)a[1];
    p_out[(n * C + c) * 2 + 1] = (float)a[2];
  }
  __syncthreads();
  const int lane = threadIdx.x & (MSBN_WAVE - 1);
  for (int j = threadIdx.x >> 6; j < Cr; j += kSeWaves) {  // wave-uniform
    const float dh = se_wave_dot(C, lane, [&](int c) {
      return to_f(w2[(int64_t)c * Cr + j]) * l2[c];
    });
    if (lane == 0) {
      const float d1 = act_grad<kActSilu>(hpre[n * Cr + j], dh, 0.f);
      l1[j] = d1;
      dz1_out[n * Cr + j] = d1;
    }
  }
  __syncthreads();
  const float inv_hw = 1.f / (float)HW;
  for (int c = threadIdx.x; c < C; c += MSBN_BLOCK) {
    float acc = 0.f;
    for (int j = 0; j < Cr; ++j) acc += to_f(w1[(int64_t)j * C + c]) * l1[j];
    dpool[n * C + c] = acc * inv_hw;
  }
}

// =====================================================================
// grid ceil(C / 4) block 256: one wave per channel, lanes stride over n.
// sums [sum_dy(C) | sum_dy_xmu(C)]; gw = sum_dy_xmu * invstd, gb = sum_dy
// =====================================================================
__global__ __launch_bounds__(MSBN_BLOCK) void se_bn_finalize_bwd(
    const float* __restrict__ g, const float* __restrict__ dpool,
    const float* __restrict__ p, const float* __restrict__ q,
    const float* __restrict__ invstd, float* __restrict__ sums,
    float* __restrict__ gw, float* __restrict__ gb, int N, int C) {
  const int lane = threadIdx.x & (MSBN_WAVE - 1);
  const int c = blockIdx.x * kSeWaves + (threadIdx.x >> 6);
  if (c >= C) return;  // a whole wave leaves; no barrier follows
  double a = 0.0, b = 0.0;
  for (int n = lane; n < N; n += MSBN_WAVE) {
    const int64_t i = (int64_t)n * C + c;
    const double gv = g[i], dp = dpool[i];
    a += gv * (double)p[2 * i] + dp * (double)q[2 * i];
    b += gv * (double)p[2 * i + 1] + dp * (double)q[2 * i + 1];
  }
  wave_reduce_pair(a, b);
  if (lane == 0) {
    sums[c] = (float)a;
    sums[C + c] = (float)b;
    if (gw != nullptr) gw[c] = (float)(b * (double)invstd[c]);
    if (gb != nullptr) gb[c] = (float)a;
  }
}

// fp64 -> WT with one rounding (dwconv5x5_kernels.hip d5_round_once)
template <typename WT>
__device__ __forceinline__ WT se_round_once(double s) {
  float f = (float)s;
  if (!std::is_same<WT, float>::value && (double)f != s) {
    unsigned bits = __float_as_uint(f);
    if (fabs((double)f) > fabs(s)) bits -= 1;
    f = __uint_as_float(bits | 1u);
  }
  return from_f<WT>(f);
}

// =====================================================================
// dW2[c][j] = sum_n dz2[n,c] silu(hpre[n,j]),  db2[c] = sum_n dz2[n,c],
// dW1[j][c] = sum_n dz1[n,j] s[n,c],           db1[j] = sum_n dz1[n,j]
// one thread per entry, n ascending in fp64; a null output is skipped
// =====================================================================
template <typename WT>
__global__ __launch_bounds__(MSBN_BLOCK) void se_param_grads(
    const float* __restrict__ dz2, const float* __restrict__ dz1,
    const float* __restrict__ hpre, const float* __restrict__ s,
    WT* __restrict__ dw1, WT* __restrict__ db1, WT* __restrict__ dw2,
    WT* __restrict__ db2, int N, int C, int Cr) {
  const int64_t idx = (int64_t)blockIdx.x * MSBN_BLOCK + threadIdx.x;
  const int64_t cc = (int64_t)C * Cr;
  double a = 0.0;
  if (idx < cc) {
    if (dw2 == nullptr) return;
    const int c = (int)(idx / Cr), j = (int)(idx - (int64_t)c * Cr);
    for (int64_t n = 0; n < N; ++n)
      a += (double)dz2[n * C + c] *
           (double)act_fwd<kActSilu>(hpre[n * Cr + j], 0.f);
    dw2[idx] = se_round_once<WT>(a);
  } else if (idx < 2 * cc) {
    if (dw1 == nullptr) return;
    const int64_t i = idx - cc;
    const int j = (int)(i / C), c = (int)(i - (int64_t)j * C);
    for (int64_t n = 0; n < N; ++n)
      a += (double)dz1[n * Cr + j] * (double)s[n * C + c];
    dw1[i] = se_round_once<WT>(a);
  } else if (idx < 2 * cc + C) {
    if (db2 == nullptr) return;
    const int c = (int)(idx - 2 * cc);
    for (int64_t n = 0; n < N; ++n) a += (double)dz2[n * C + c];
    db2[c] = se_round_once<WT>(a);
  } else if (idx < 2 * cc + C + Cr) {
    if (db1 == nullptr) return;
    const int j = (int)(idx - 2 * cc - C);
    for (int64_t n = 0; n < N; ++n) a += (double)dz1[n * Cr + j];
    db1[j] = se_round_once<WT>(a);
  }
}

// dy = A*gz + B*y + D (bn_kernels.hip bn_affine_bwd, fp32 weight):
//   f1 = invstd*gamma, f2 = sum_dy/n, f3 = invstd^2*sum_dy_xmu/n
//   A = f1, B = -f1*f3, D = f1*(f3*mean - f2)
__global__ void se_affine_bwd(const float* __restrict__ mean,
                              const float* __restrict__ invstd,
                              const float* __restrict__ w,
                              const float* __restrict__ sum_dy,
                              const float* __restrict__ sum_dy_xmu,
                              const float* __restrict__ count, int C,
                              float* __restrict__ abd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float n = count[0];
  if (n <= 0.f) {
    abd[c] = abd[C + c] = abd[2 * C + c] = 0.f;
    return;
  }
  const float istd = invstd[c];
  const float f1 = istd * (w != nullptr ? w[c] : 1.f);
  const float f2 = sum_dy[c] / n;
  const float f3 = istd * istd * sum_dy_xmu[c] / n;
  abd[c] = f1;
  abd[C + c] = -f1 * f3;
  abd[2 * C + c] = f1 * (f3 * mean[c] - f2);
}

// ------------------------------------------------------------------- host
inline int64_t se_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

void se_check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "squeeze-excite: ", what, ": ",
              hipGetErrorString(e));
}

// a dense channels-last [N, C, H, W] of y's dtype and device, 16-byte aligned
bool se_same_as(const at::Tensor& t, const at::Tensor& y) {
  return t.defined() && t.dim() == 4 && t.sizes() == y.sizes() &&
         t.scalar_type() == y.scalar_type() && t.device() == y.device() &&
         t.is_contiguous(at::MemoryFormat::ChannelsLast) &&
         (uintptr_t)t.data_ptr() % 16 == 0;
}

// a contiguous fp32 tensor of `numel` elements on y's device
bool se_is_f32(const at::Tensor& t, int64_t numel, const at::Tensor& y) {
  return t.defined() && t.scalar_type() == at::kFloat && t.is_contiguous() &&
         t.numel() == numel && t.device() == y.device();
}

void se_check_f32(const at::Tensor& t, int64_t numel, const at::Tensor& y,
                  const char* name) {
  TORCH_CHECK(se_is_f32(t, numel, y),
              "squeeze-excite: ", name, " must be a contiguous fp32 tensor of ",
              numel, " elements on the activation's device");
}

template <typename F>
void se_dispatch_act(const at::Tensor& y, F&& go) {
  if (y.scalar_type() == at::kBFloat16)
    go(__hip_bfloat16{});
  else
    go(__half{});
}

template <typename F>
void se_dispatch_weight(at::ScalarType t, F&& go) {
  if (t == at::kFloat)
    go(float{});
  else if (t == at::kBFloat16)
    go(__hip_bfloat16{});
  else
    go(__half{});
}

dim3 se_grid(const SePlan& p) {
  return dim3((unsigned)p.ctiles, (unsigned)p.chunks_per_image, (unsigned)p.n);
}

// the SE parameters the gate kernels take: w1 [Cr, C(,1,1)], w2 [C, Cr(,1,1)]
// contiguous, of one dtype (fp32 / bf16 / half) and on `dev`
bool se_weights_ok(const at::Tensor& w1, const at::Tensor& w2, int64_t C,
                   const at::Device& dev) {
  if (!w1.defined() || !w2.defined() || w1.dim() < 2 || w2.dim() < 2)
    return false;
  const int64_t Cr = w1.size(0);
  if (!se_gate_fits(C, Cr)) return false;
  if (w1.numel() != Cr * C || w1.size(1) != C || w2.numel() != Cr * C ||
      w2.size(0) != C || w2.size(1) != Cr)
    return false;
  const auto dt = w1.scalar_type();
  if (dt != at::kFloat && dt != at::kBFloat16 && dt != at::kHalf) return false;
  return w2.scalar_type() == dt && w1.is_contiguous() && w2.is_contiguous() &&
         w1.device() == dev && w2.device() == dev;
}

// the partials of se_squeeze: a non-empty contiguous fp64 [N, chunks, C, 3]
// on the weights' device
bool se_ws_ok(const at::Tensor& ws, const at::Tensor& like, int64_t C) {
  return ws.defined() && ws.dim() == 4 && ws.scalar_type() == at::kDouble &&
         ws.is_contiguous() && ws.size(2) == C && ws.size(3) == 3 &&
         ws.numel() > 0 && ws.size(0) <= INT32_MAX && ws.size(1) <= INT32_MAX &&
         ws.device() == like.device();
}

using SeFour = std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>;

// what a gate op returns for tensors it does not take: nothing launched
SeFour se_declined() { return SeFour{}; }

}  // namespace

bool se_gate_fits(int64_t C, int64_t Cr) {
  return C >= 1 && C <= kSeMaxC && Cr >= 1 && Cr <= kSeMaxCr;
}

SePlan se_plan(const at::Tensor& y) {
  SePlan p{};
  if (!y.defined() || y.dim() != 4 || y.numel() == 0) return p;
  const auto dt = y.scalar_type();
  if (dt != at::kBFloat16 && dt != at::kHalf) return p;
  if (!y.is_contiguous(at::MemoryFormat::ChannelsLast)) return p;
  const int64_t C = y.size(1);
  if (C % kSeV != 0 || C > (1 << 24)) return p;
  if ((uintptr_t)y.data_ptr() % 16 != 0) return p;
  p.n = y.size(0);
  p.c = C;
  p.hw = y.size(2) * y.size(3);
  if (p.n > 65535) return p;  // images are the grid's z axis
  p.v = kSeV;
  p.lpr = nhwc_lanes_per_row(C, kSeV);
  p.ctiles = (int)se_cdiv(C, (int64_t)p.lpr * kSeV);
  const int64_t rpi = MSBN_BLOCK / p.lpr;
  // about kTargetBlocks blocks in all; a chunk is whole trips of the block
  const int64_t want = std::max<int64_t>(1, kTargetBlocks / (p.ctiles * p.n));
  const int64_t chunks = std::min(want, se_cdiv(p.hw, rpi));
  const int64_t rows = se_cdiv(se_cdiv(p.hw, chunks), rpi) * rpi;
  if (rows > INT32_MAX) return p;
  p.chunk_rows = (int)rows;
  p.chunks_per_image = (int)se_cdiv(p.hw, rows);
  if (p.chunks_per_image > 65535) return p;
  p.trips = (int)(rows / rpi);
  p.flush_every = MSBN_ACC_FLUSH;
  p.ok = true;
  return p;
}

at::Tensor se_squeeze(const at::Tensor& y, const at::Tensor& coefs,
                      const at::Tensor& mean,
                      const c10::optional<at::Tensor>& grad_out) {
  if (!y.defined() || !y.is_cuda()) return at::Tensor();
  const SePlan p = se_plan(y);
  if (!p.ok) return at::Tensor();
  const bool bwd = grad_out.has_value() && grad_out->defined();
  if (bwd && !se_same_as(*grad_out, y)) return at::Tensor();
  se_check_f32(coefs, 2 * p.c, y, "coefs");
  se_check_f32(mean, p.c, y, "mean");
  at::Tensor ws = at::empty({p.n, (int64_t)p.chunks_per_image, p.c, 3},
                            y.options().dtype(at::kDouble));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  se_dispatch_act(y, [&](auto tag) {
    using T = decltype(tag);
    auto kernel = bwd ? se_reduce_nhwc<T, true> : se_reduce_nhwc<T, false>;
    hipLaunchKernelGGL(
        kernel, se_grid(p), dim3(MSBN_BLOCK), 0, stream,
        reinterpret_cast<const T*>(y.data_ptr()),
        bwd ? reinterpret_cast<const T*>(grad_out->data_ptr()) : nullptr,
        coefs.data_ptr<float>(), mean.data_ptr<float>(), ws.data_ptr<double>(),
        p.hw, (int)p.c, p.chunk_rows, p.lpr, p.chunks_per_image);
  });
  se_check_launch(bwd ? "backward reduce launch" : "squeeze launch");
  return ws;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> se_gate(
    const at::Tensor& ws, int64_t hw, const at::Tensor& w1,
    const at::Tensor& b1, const at::Tensor& w2, const at::Tensor& b2) {
  if (!w1.defined() || !w1.is_cuda()) return se_declined();
  const int64_t C = w2.defined() && w2.dim() >= 1 ? w2.size(0) : 0;
  if (!se_weights_ok(w1, w2, C, w1.device()) || !se_ws_ok(ws, w1, C) || hw < 1)
    return se_declined();
  const int64_t Cr = w1.size(0);
  for (const at::Tensor* b : {&b1, &b2})
    if (!(b->defined() && b->scalar_type() == w1.scalar_type() &&
          b->is_contiguous() && b->device() == w1.device()))
      return se_declined();
  if (b1.numel() != Cr || b2.numel() != C) return se_declined();
  const int64_t N = ws.size(0);
  auto f32 = w1.options().dtype(at::kFloat);
  at::Tensor s = at::empty({N, C}, f32), hpre = at::empty({N, Cr}, f32),
             g = at::empty({N, C}, f32), q = at::empty({N, C, 2}, f32);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  se_dispatch_weight(w1.scalar_type(), [&](auto tag) {
    using WT = decltype(tag);
    hipLaunchKernelGGL(
        (se_gate_fwd<WT>), dim3((unsigned)N), dim3(MSBN_BLOCK), 0, stream,
        ws.data_ptr<double>(), reinterpret_cast<const WT*>(w1.data_ptr()),
        reinterpret_cast<const WT*>(b1.data_ptr()),
        reinterpret_cast<const WT*>(w2.data_ptr()),
        reinterpret_cast<const WT*>(b2.data_ptr()), s.data_ptr<float>(),
        hpre.data_ptr<float>(), g.data_ptr<float>(), q.data_ptr<float>(), hw,
        (int)C, (int)Cr, (int)ws.size(1));
  });
  se_check_launch("gate launch");
  return {s, hpre, g, q};
}

at::Tensor se_scale(const at::Tensor& y, const at::Tensor& coefs,
                    const at::Tensor& g) {
  if (!y.defined() || !y.is_cuda()) return at::Tensor();
  const SePlan p = se_plan(y);
  if (!p.ok) return at::Tensor();
  se_check_f32(coefs, 2 * p.c, y, "coefs");
  se_check_f32(g, p.n * p.c, y, "g");
  at::Tensor out = at::empty_like(y);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  se_dispatch_act(y, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((se_scale_nhwc<T>), se_grid(p), dim3(MSBN_BLOCK), 0,
                       stream, reinterpret_cast<const T*>(y.data_ptr()),
                       coefs.data_ptr<float>(), g.data_ptr<float>(),
                       reinterpret_cast<T*>(out.data_ptr()), p.hw, (int)p.c,
                       p.chunk_rows, p.lpr);
  });
  se_check_launch("scale launch");
  return out;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> se_gate_backward(
    const at::Tensor& ws, int64_t hw, const at::Tensor& g,
    const at::Tensor& hpre, const at::Tensor& w1, const at::Tensor& w2) {
  if (!w1.defined() || !w1.is_cuda()) return se_declined();
  const int64_t C = w2.defined() && w2.dim() >= 1 ? w2.size(0) : 0;
  if (!se_weights_ok(w1, w2, C, w1.device()) || !se_ws_ok(ws, w1, C) || hw < 1)
    return se_declined();
  const int64_t Cr = w1.size(0);
  const int64_t N = ws.size(0);
  if (!se_is_f32(g, N * C, w1) || !se_is_f32(hpre, N * Cr, w1))
    return se_declined();
  auto f32 = w1.options().dtype(at::kFloat);
  at::Tensor dpool = at::empty({N, C}, f32), dz2 = at::empty({N, C}, f32),
             dz1 = at::empty({N, Cr}, f32), pt = at::empty({N, C, 2}, f32);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  se_dispatch_weight(w1.scalar_type(), [&](auto tag) {
    using WT = decltype(tag);
    hipLaunchKernelGGL(
        (se_gate_bwd<WT>), dim3((unsigned)N), dim3(MSBN_BLOCK), 0, stream,
        ws.data_ptr<double>(), g.data_ptr<float>(), hpre.data_ptr<float>(),
        reinterpret_cast<const WT*>(w1.data_ptr()),
        reinterpret_cast<const WT*>(w2.data_ptr()), dpool.data_ptr<float>(),
        dz2.data_ptr<float>(), dz1.data_ptr<float>(), pt.data_ptr<float>(), hw,
        (int)C, (int)Cr, (int)ws.size(1));
  });
  se_check_launch("gate backward launch");
  return {dpool, dz2, dz1, pt};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
se_bn_finalize_backward(const at::Tensor& g, const at::Tensor& dpool,
                        const at::Tensor& p, const at::Tensor& q,
                        const at::Tensor& invstd, bool weight_g, bool bias_g) {
  if (!g.defined() || !g.is_cuda() || g.dim() != 2 || g.numel() == 0)
    return se_declined();
  const int64_t N = g.size(0), C = g.size(1);
  if (N > INT32_MAX || C > (1 << 24)) return se_declined();
  if (!se_is_f32(g, N * C, g) || !se_is_f32(dpool, N * C, g) ||
      !se_is_f32(p, 2 * N * C, g) || !se_is_f32(q, 2 * N * C, g) ||
      !se_is_f32(invstd, C, g))
    return se_declined();
  at::Tensor sums = at::empty({2 * C}, g.options());
  at::Tensor gw, gb;
  if (weight_g) gw = at::empty({C}, g.options());
  if (bias_g) gb = at::empty({C}, g.options());
  hipLaunchKernelGGL(se_bn_finalize_bwd, dim3((unsigned)se_cdiv(C, kSeWaves)),
                     dim3(MSBN_BLOCK), 0,
                     c10::hip::getCurrentHIPStream().stream(),
                     g.data_ptr<float>(), dpool.data_ptr<float>(),
                     p.data_ptr<float>(), q.data_ptr<float>(),
                     invstd.data_ptr<float>(), sums.data_ptr<float>(),
                     weight_g ? gw.data_ptr<float>() : nullptr,
                     bias_g ? gb.data_ptr<float>() : nullptr, (int)N, (int)C);
  se_check_launch("BN finalize launch");
  return {sums.narrow(0, 0, C), sums.narrow(0, C, C), gw, gb};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> se_param_backward(
    const at::Tensor& dz2, const at::Tensor& dz1, const at::Tensor& hpre,
    const at::Tensor& s, const at::Tensor& w1, const at::Tensor& w2,
    bool want_w1, bool want_b1, bool want_w2, bool want_b2) {
  if (!dz2.defined() || !dz2.is_cuda() || dz2.dim() != 2 ||
      dz2.numel() == 0 || !dz1.defined() || dz1.dim() != 2)
    return se_declined();
  const int64_t N = dz2.size(0), C = dz2.size(1), Cr = dz1.size(1);
  if (N > INT32_MAX || !se_weights_ok(w1, w2, C, dz2.device()) ||
      w1.size(0) != Cr)
    return se_declined();
  if (!se_is_f32(dz2, N * C, dz2) || !se_is_f32(dz1, N * Cr, dz2) ||
      !se_is_f32(hpre, N * Cr, dz2) || !se_is_f32(s, N * C, dz2))
    return se_declined();
  at::Tensor dw1, db1, dw2, db2;
  if (want_w1) dw1 = at::empty_like(w1);
  if (want_b1) db1 = at::empty({Cr}, w1.options());
  if (want_w2) dw2 = at::empty_like(w2);
  if (want_b2) db2 = at::empty({C}, w1.options());
  if (!(want_w1 || want_b1 || want_w2 || want_b2)) return {dw1, db1, dw2, db2};
  const int64_t total = 2 * C * Cr + C + Cr;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  se_dispatch_weight(w1.scalar_type(), [&](auto tag) {
    using WT = decltype(tag);
    auto ptr = [](at::Tensor& t) {
      return t.defined() ? reinterpret_cast<WT*>(t.data_ptr()) : nullptr;
    };
    hipLaunchKernelGGL((se_param_grads<WT>),
                       dim3((unsigned)se_cdiv(total, MSBN_BLOCK)),
                       dim3(MSBN_BLOCK), 0, stream, dz2.data_ptr<float>(),
                       dz1.data_ptr<float>(), hpre.data_ptr<float>(),
                       s.data_ptr<float>(), ptr(dw1), ptr(db1), ptr(dw2),
                       ptr(db2), (int)N, (int)C, (int)Cr);
  });
  se_check_launch("parameter gradient launch");
  return {dw1, db1, dw2, db2};
}

at::Tensor se_backward_elemt(const at::Tensor& grad_out, const at::Tensor& y,
                             const at::Tensor& coefs, const at::Tensor& g,
                             const at::Tensor& dpool, const at::Tensor& mean,
                             const at::Tensor& invstd,
                             const c10::optional<at::Tensor>& weight,
                             const at::Tensor& sum_dy,
                             const at::Tensor& sum_dy_xmu,
                             const at::Tensor& count) {
  if (!y.defined() || !y.is_cuda()) return at::Tensor();
  const SePlan p = se_plan(y);
  if (!p.ok || !se_same_as(grad_out, y)) return at::Tensor();
  se_check_f32(coefs, 2 * p.c, y, "coefs");
  se_check_f32(g, p.n * p.c, y, "g");
  se_check_f32(dpool, p.n * p.c, y, "dpool");
  se_check_f32(mean, p.c, y, "mean");
  se_check_f32(invstd, p.c, y, "invstd");
  se_check_f32(sum_dy, p.c, y, "sum_dy");
  se_check_f32(sum_dy_xmu, p.c, y, "sum_dy_xmu");
  se_check_f32(count, 1, y, "count");
  const bool has_w = weight.has_value() && weight->defined();
  if (has_w) se_check_f32(*weight, p.c, y, "weight");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  at::Tensor abd = at::empty({3 * p.c}, y.options().dtype(at::kFloat));
  hipLaunchKernelGGL(se_affine_bwd, dim3((unsigned)se_cdiv(p.c, MSBN_BLOCK)),
                     dim3(MSBN_BLOCK), 0, stream, mean.data_ptr<float>(),
                     invstd.data_ptr<float>(),
                     has_w ? weight->data_ptr<float>() : nullptr,
                     sum_dy.data_ptr<float>(), sum_dy_xmu.data_ptr<float>(),
                     count.data_ptr<float>(), (int)p.c, abd.data_ptr<float>());
  se_check_launch("backward coefficient launch");
  at::Tensor dy = at::empty_like(y);
  se_dispatch_act(y, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((se_bwd_elemt_nhwc<T>), se_grid(p), dim3(MSBN_BLOCK), 0,
                       stream, reinterpret_cast<const T*>(grad_out.data_ptr()),
                       reinterpret_cast<const T*>(y.data_ptr()),
                       coefs.data_ptr<float>(), g.data_ptr<float>(),
                       dpool.data_ptr<float>(), abd.data_ptr<float>(),
                       reinterpret_cast<T*>(dy.data_ptr()), p.hw, (int)p.c,
                       p.chunk_rows, p.lpr);
  });
  se_check_launch("backward elementwise launch");
  return dy;
}

std::tuple<std::string, std::map<std::string, int64_t>> launch_plan_se(
    const std::string& kind, const at::Tensor& input,
    const std::vector<c10::optional<at::Tensor>>& others) {
  std::map<std::string, int64_t> d;
  auto given = [&](size_t i) {
    return i < others.size() && others[i].has_value() && others[i]->defined();
  };
  const bool gate = kind == "se_gate" || kind == "se_gate_bwd";
  const bool with_grad = kind == "se_bwd_reduce" || kind == "se_bwd_elemt";
  TORCH_CHECK(gate || with_grad || kind == "se_squeeze" || kind == "se_scale",
              "launch_plan: unknown kind '", kind, "'");
  const SePlan p = se_plan(input);
  if (!p.ok) return {"ineligible", d};
  if (with_grad && !(given(0) && se_same_as(*others[0], input)))
    return {"ineligible", d};
  if (gate) {
    if (!given(0) || !given(1) ||
        !se_weights_ok(*others[0], *others[1], p.c, others[0]->device()))
      return {"ineligible", d};
    d["Cr"] = others[0]->size(0);
    d["lds_bytes"] = (kSeMaxC + kSeMaxCr) * (int64_t)sizeof(float);
  }
  d["V"] = p.v;
  d["lpr"] = p.lpr;
  d["ctiles"] = p.ctiles;
  d["chunk_rows"] = p.chunk_rows;
  d["chunks_per_image"] = p.chunks_per_image;
  d["trips"] = p.trips;
  d["flush_every"] = p.flush_every;
  // the per-channel sum over the images: lanes of one wave stride over n
  d["finalize_trips"] = se_cdiv(p.n, MSBN_WAVE);
  return {gate ? "se_gate" : "se", d};
}

}  // namespace msbn
