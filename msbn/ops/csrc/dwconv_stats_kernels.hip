// Depthwise 3x3 convolution (padding 1, stride 1 or 2, channel multiplier 1)
// that also emits the following BatchNorm's statistics (gfx950, CDNA4).
// docs/KERNEL_DESIGN.md "Depthwise conv + statistics".
//
// Channels-last, a depthwise convolution has no reduction over channels: a
// lane that owns one 16-byte pack of 8 channels needs nothing from its
// neighbours.  It is 9 FMAs per output element over streamed packs, i.e. the
// BN kernels' kind of work, and the kernel is laid out like them:
//
//  * grid (channel tiles, chunks), block 256.  lpr lanes lie across the
//    channel axis (nhwc_lanes_per_row: a row segment stays >= 128 B), the
//    other rpi = 256 / lpr thread rows each take work items.  A work item is
//    one output row of one image x a strip of kDwStrip consecutive output
//    columns; a chunk is a contiguous run of items, dealt round-robin to the
//    thread rows.  An item is addressed by (n, oh, strip) and every input row
//    by (n, ih) with 0 <= ih < H: it cannot reach into a neighbouring image.
//  * the lane's 9 weight packs (72 contiguous values, w[c..c+7][0][kh][kw])
//    are loaded once per block with cached loads and held as fp32.
//  * the thread slides a 3-column fp32 register window along its strip: each
//    new output column costs 3 (stride 1) or 6 (stride 2) nontemporal 16-byte
//    loads, issued one output column ahead of the FMAs that use them.  The
//    rows above / below are re-read by the threads of the neighbouring output
//    rows and come from L1 / L2.  Taps outside the image are never loaded:
//    their window entry is a zero made in registers (for finite weights the
//    sum is bit for bit the one that skips them).
//  * the 9 products go kh then kw ascending into one fp32 accumulator per
//    element, which is rounded to T once and stored with a nontemporal store.
//  * statistics are those of the rounded values, always shifted (nothing can
//    be re-read): per thread and channel the pivot is the thread's first
//    stored value of the chunk, d = y - pivot and d^2 are summed in fp32 for
//    at most MSBN_ACC_FLUSH terms, flushed into fp64 totals (kept in the
//    thread's own LDS slots, see below), un-shifted in fp64 with the thread's
//    own count, and the thread rows' pairs are added through the [k][tid]
//    split-plane LDS tree of the NHWC reduce kernels.
//    One {sum y, sum y^2} pair per (channel, chunk): ws[C][nchunks][2], the
//    workspace bn_stats_finalize consumes.  No atomics.
#include "bn_ops.hpp"
#include "common.hpp"
#include "launch_common.hpp"

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>

// Scalar fp32 arithmetic only in this file's device code (as in
// conv_stats_kernels.hip): the per-channel FMAs over a pack are what the
// vectorizer turns into packed fp32 instructions.  Hence the spelled-out
// barrier (grouped_bn_kernels.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace msbn {

namespace {

constexpr int kDwV = 8;      // channels of a lane: one 16-byte pack
constexpr int kDwStrip = 8;  // output columns of a work item (TW)
// items between two flushes: kDwStrip terms each
constexpr int kDwFlushItems = MSBN_ACC_FLUSH / kDwStrip;
static_assert(kDwFlushItems >= 1, "a strip must fit one flush period");

__device__ __forceinline__ void dw_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// 16 bytes of x or w; all zero until something is loaded into it
template <typename T>
union DwPack {
  Pack<T, kDwV> pk;
  int __attribute__((vector_size(16))) raw;
  __device__ __forceinline__ DwPack() : raw{0, 0, 0, 0} {}
};

// =====================================================================
// grid (ctiles, nchunks) block 256; lpr a power of two dividing 256
// x [N][H][W][C], w [C][1][3][3], y [N][OH][OW][C], ws [C][nchunks][2]
// spr = strips per output row; items = N * OH * spr (< 2^31 - 256)
// =====================================================================
template <typename T, int S>
__global__ __launch_bounds__(MSBN_BLOCK, 2) void dwconv3x3_stats_nhwc(
    const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y,
    double* __restrict__ ws, int H, int W, int C, int OH, int OW, int spr,
    int items, int chunk_items, int lpr, int nchunks) {
  constexpr int V = kDwV;
  constexpr int TW = kDwStrip;
  constexpr int NEWC = S;  // window columns an output column adds
  const int rpi = MSBN_BLOCK / lpr;
  const int lane = threadIdx.x & (lpr - 1);
  const int rowoff = threadIdx.x / lpr;
  const int c = (blockIdx.x * lpr + lane) * V;
  const bool inb = c < C;  // C is a multiple of V: a pack is in or out whole

  __shared__ double sdata[MSBN_BLOCK * V * 2];

  // ---- this lane's weights: 72 contiguous values from w + 9 c ----
  float wf[9][V];
  {
    DwPack<T> wp[9];
    if (inb) {
#pragma unroll
      for (int i = 0; i < 9; ++i)
        wp[i].pk =
            *reinterpret_cast<const Pack<T, V>*>(w + (int64_t)c * 9 + i * V);
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int t = 0; t < 9; ++t)
        wf[t][k] = to_f(wp[(k * 9 + t) / V].pk.v[(k * 9 + t) % V]);
  }

  // The fp64 totals of this thread live in its own slots of the tree's
  // planes (sdata[k][tid], sdata[V + k][tid]: conflict-free and private until
  // the tree starts), not in 32 VGPRs: next to 72 weights and a 72-value
  // window those would cost the second wave per SIMD.  Registers hold the
  // fp32 chunk sums alone.
  float fa[V], fb[V], pivot[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    fa[k] = fb[k] = pivot[k] = 0.f;
    sdata[k * MSBN_BLOCK + threadIdx.x] = 0.0;
    sdata[(V + k) * MSBN_BLOCK + threadIdx.x] = 0.0;
  }
  auto flush = [&]() {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      sdata[k * MSBN_BLOCK + threadIdx.x] += (double)fa[k];
      sdata[(V + k) * MSBN_BLOCK + threadIdx.x] += (double)fb[k];
      fa[k] = fb[k] = 0.f;
    }
  };
  bool have_pivot = false;
  int cnt = 0;  // values this thread has summed, per channel

  if (inb) {
    const int i0 = blockIdx.y * chunk_items;
    const int i1 = i0 + chunk_items < items ? i0 + chunk_items : items;
    int since_flush = 0;
    for (int item = i0 + rowoff; item < i1; item += rpi) {
      const int orow = item / spr;  // n * OH + oh
      const int ow0 = (item - orow * spr) * TW;
      const int n = orow / OH;
      const int oh = orow - n * OH;
      const int nvalid = OW - ow0 < TW ? OW - ow0 : TW;  // >= 1

      // the three input rows: pointer to (n, ih, 0, c), or unused
      bool rok[3];
      const T* xr[3];
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int ih = oh * S - 1 + kh;
        rok[kh] = ih >= 0 && ih < H;
        xr[kh] = x + ((int64_t)n * H + (rok[kh] ? ih : 0)) * W * C + c;
      }
      T* yp = y + ((int64_t)orow * OW + ow0) * C + c;

      // one window column: rows kh of input column iw, zero where outside
      auto load_col = [&](DwPack<T>(&col)[3], int iw, bool want) {
        const bool cok = want && iw >= 0 && iw < W;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          DwPack<T> v;
          if (cok && rok[kh]) v.pk = nt_load<T, V>(xr[kh] + (int64_t)iw * C);
          col[kh] = v;
        }
      };
      auto to_window = [&](float(&dst)[3][V], const DwPack<T>(&col)[3]) {
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int k = 0; k < V; ++k) dst[kh][k] = to_f(col[kh].pk.v[k]);
      };

      float win[3][3][V];  // [kw][kh][k]
      {
        DwPack<T> first[3][3];
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) load_col(first[kw], ow0 * S - 1 + kw, true);
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) to_window(win[kw], first[kw]);
      }

#pragma unroll
      for (int j = 0; j < TW; ++j) {
        // the columns output j + 1 adds, in flight during output j's FMAs
        DwPack<T> nxt[NEWC][3];
        if (j + 1 < TW) {
          const bool want = j + 1 < nvalid;
#pragma unroll
          for (int q = 0; q < NEWC; ++q)
            load_col(nxt[q], (ow0 + j + 1) * S - 1 + (3 - NEWC) + q, want);
        }
        if (j < nvalid) {
          DwPack<T> out;
#pragma unroll
          for (int k = 0; k < V; ++k) {
            float a = 0.f;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
              for (int kw = 0; kw < 3; ++kw)
                a += win[kw][kh][k] * wf[kh * 3 + kw][k];
            const T r = from_f<T>(a);
            out.pk.v[k] = r;
            const float v = to_f(r);
            if (j == 0 && !have_pivot) pivot[k] = v;
            const float d = v - pivot[k];
            fa[k] += d;
            fb[k] += d * d;
          }
          if (j == 0) have_pivot = true;
          nt_store<T, V>(yp + (int64_t)j * C, out.pk);
        }
        if (j + 1 < TW) {
          // slide: stride 1 keeps two columns, stride 2 keeps one
#pragma unroll
          for (int kw = 0; kw < 3 - NEWC; ++kw)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
              for (int k = 0; k < V; ++k)
                win[kw][kh][k] = win[kw + NEWC][kh][k];
#pragma unroll
          for (int q = 0; q < NEWC; ++q) to_window(win[3 - NEWC + q], nxt[q]);
        }
      }
      cnt += nvalid;
      if (++since_flush == kDwFlushItems) {
        flush();
        since_flush = 0;
      }
    }
  }

  flush();
#pragma unroll
  for (int k = 0; k < V; ++k) {
    double a = sdata[k * MSBN_BLOCK + threadIdx.x];
    double b = sdata[(V + k) * MSBN_BLOCK + threadIdx.x];
    // cnt == 0: pivot and both sums are zero, and stay so
    unshift_pair(a, b, pivot[k], (double)cnt);
    sdata[k * MSBN_BLOCK + threadIdx.x] = a;
    sdata[(V + k) * MSBN_BLOCK + threadIdx.x] = b;
  }

  // ---- thread rows -> one pair per channel: [k][tid] planes ----
  for (int st = 1; st < rpi; st <<= 1) {
    dw_sync();
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
  dw_sync();
  if (rowoff == 0 && inb) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      double* out = ws + ((int64_t)(c + k) * nchunks + blockIdx.y) * 2;
      out[0] = sdata[k * MSBN_BLOCK + threadIdx.x];
      out[1] = sdata[(V + k) * MSBN_BLOCK + threadIdx.x];
    }
  }
}

inline int64_t dw_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

template <typename T, int S>
void dw_launch(const DwConvPlan& p, const at::Tensor& x, const at::Tensor& w,
               at::Tensor& y, at::Tensor& ws) {
  hipLaunchKernelGGL((dwconv3x3_stats_nhwc<T, S>),
                     dim3((unsigned)p.ctiles, (unsigned)p.nchunks),
                     dim3(MSBN_BLOCK), 0,
                     c10::hip::getCurrentHIPStream().stream(),
                     reinterpret_cast<const T*>(x.data_ptr()),
                     reinterpret_cast<const T*>(w.data_ptr()),
                     reinterpret_cast<T*>(y.data_ptr()), ws.data_ptr<double>(),
                     (int)p.h, (int)p.w, (int)p.c, (int)p.oh, (int)p.ow,
                     (int)(p.items / (p.n * p.oh)), (int)p.items,
                     (int)p.chunk_items, p.lpr, p.nchunks);
  const hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "dwconv3x3_stats: launch: ",
              hipGetErrorString(e));
}

}  // namespace

DwConvPlan dwconv3x3_plan(const at::Tensor& input, const at::Tensor& weight,
                          int64_t stride) {
  DwConvPlan p{};
  if (stride != 1 && stride != 2) return p;
  if (!input.defined() || !weight.defined()) return p;
  if (input.dim() != 4 || weight.dim() != 4 || input.numel() == 0) return p;
  const auto dt = input.scalar_type();
  if (dt != at::kBFloat16 && dt != at::kHalf) return p;
  if (weight.scalar_type() != dt || weight.device() != input.device()) return p;
  if (!input.is_contiguous(at::MemoryFormat::ChannelsLast)) return p;
  const int64_t C = input.size(1);
  if (weight.size(0) != C || weight.size(1) != 1 || weight.size(2) != 3 ||
      weight.size(3) != 3 || !weight.is_contiguous())
    return p;
  if (C % kDwV != 0 || C > (1 << 24)) return p;
  if ((uintptr_t)input.data_ptr() % 16 != 0 ||
      (uintptr_t)weight.data_ptr() % 16 != 0)
    return p;
  p.n = input.size(0);
  p.c = C;
  p.h = input.size(2);
  p.w = input.size(3);
  p.stride = (int)stride;
  p.oh = (p.h - 1) / stride + 1;
  p.ow = (p.w - 1) / stride + 1;
  p.strip = kDwStrip;
  const int64_t spr = dw_cdiv(p.ow, kDwStrip);
  p.items = p.n * p.oh * spr;
  // the kernel counts items, rows and columns in 32 bits
  if (p.items >= (int64_t)INT32_MAX - MSBN_BLOCK || p.h >= (1 << 30) ||
      p.w >= (1 << 30))
    return p;
  p.v = kDwV;
  p.lpr = nhwc_lanes_per_row(C, kDwV);
  p.ctiles = (int)dw_cdiv(C, (int64_t)p.lpr * kDwV);
  const int rpi = MSBN_BLOCK / p.lpr;
  // the NHWC reductions' chunk rule over the output pixels (a workspace of a
  // few per cent of y), and no more chunks than give every thread row an item
  const int64_t pixels = p.n * p.oh * p.ow;
  const int64_t per_tile = std::max<int64_t>(1, kTargetBlocks / p.ctiles);
  const int64_t max_chunks = std::min(
      dw_cdiv(pixels, std::max<int64_t>(4 * rpi, 16)), dw_cdiv(p.items, rpi));
  const int64_t nchunks =
      std::max<int64_t>(1, std::min(per_tile, std::max<int64_t>(max_chunks, 1)));
  p.chunk_items = dw_cdiv(p.items, nchunks);
  p.nchunks = (int)dw_cdiv(p.items, p.chunk_items);
  p.trips = (int)dw_cdiv(p.chunk_items, rpi);
  p.flush_every = kDwFlushItems * kDwStrip;
  p.ok = true;
  return p;
}

std::tuple<at::Tensor, at::Tensor, int64_t> dwconv3x3_stats(
    const at::Tensor& input, const at::Tensor& weight, int64_t stride) {
  if (!input.defined() || !input.is_cuda())
    return {at::Tensor(), at::Tensor(), 0};
  const DwConvPlan p = dwconv3x3_plan(input, weight, stride);
  if (!p.ok) return {at::Tensor(), at::Tensor(), 0};
  // allocator-aligned outputs
  at::Tensor y = at::empty(
      {p.n, p.c, p.oh, p.ow},
      input.options().memory_format(at::MemoryFormat::ChannelsLast));
  at::Tensor ws = at::empty({p.c, (int64_t)p.nchunks, 2},
                            input.options().dtype(at::kDouble));
  auto go = [&](auto tag) {
    using T = decltype(tag);
    if (p.stride == 1)
      dw_launch<T, 1>(p, input, weight, y, ws);
    else
      dw_launch<T, 2>(p, input, weight, y, ws);
  };
  if (input.scalar_type() == at::kBFloat16)
    go(__hip_bfloat16{});
  else
    go(__half{});
  return {y, ws, (int64_t)p.nchunks};
}

}  // namespace msbn

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
