// Gradients of the depthwise 3x3 convolution of dwconv_stats_kernels.hip
// (padding 1, stride 1 or 2, channel multiplier 1) for gfx950 (CDNA4).
// docs/KERNEL_DESIGN.md "Depthwise conv gradients".
//
// Channels-last, both gradients are the forward's kind of work: no reduction
// over channels, one lane = one 16-byte pack of 8 channels, a handful of FMAs
// per streamed element.  Both kernels use the forward's layout: block 256,
// lpr lanes across the channel axis (nhwc_lanes_per_row), rpi = 256 / lpr
// thread rows that take work items round-robin from the block's chunk (a
// contiguous run of items), nontemporal streaming accesses, cached weights.
//
// Data gradient (dwconv3x3_dgrad_nhwc), input-centric:
//   dx[n,c,ih,iw] = sum dy[n,c,oh,ow] * w[c,kh,kw] over the (kh, kw) with
//   ih = oh*s - 1 + kh, iw = ow*s - 1 + kw, 0 <= oh < OH, 0 <= ow < OW.
//  * a work item is one dx row of one image x a strip of kGradStrip columns,
//    addressed (n, ih, strip); every dy row is addressed (n, oh) with
//    0 <= oh < OH, so nothing reaches into a neighbouring image.
//  * tap order, both strides: dy rows ascending (kh descending), within a row
//    dy columns ascending (kw descending), fp32 products into one fp32
//    accumulator per element, rounded to T once.  Taps outside dy are never
//    loaded: their operand is a zero made in registers (stride 1), or the tap
//    is not issued at all (the parity scheme of stride 2 below; its one
//    out-of-range row / column, oh == OH or ow == OW for even H / W, is a
//    register zero too).  For finite weights the sum is the one that skips
//    them.
//  * stride 1 is the forward over dy with the weights flipped: a sliding
//    3-column fp32 window, 3 loads per dx column issued one column ahead.
//  * stride 2: a dx element takes 1, 2 or 4 taps by the parity of (ih, iw).
//    Even ih has kh = 1 alone (oh = ih/2); odd ih has kh = 2 (oh = (ih-1)/2)
//    and kh = 0 (oh = (ih+1)/2); columns alike.  The row parity is uniform
//    over an item, so the item body is compiled twice (ODD) with 1 or 2 dy
//    rows; the column parity is that of the unrolled column index (strips
//    start at multiples of 8).  An 8-column strip needs 5 dy columns: all 5
//    or 10 packs are loaded up front, then 12 (even row) or 24 (odd row)
//    FMAs per channel and strip follow, against 72 for nine predicated taps.
//
// Weight gradient (dwconv3x3_wgrad_partial_nhwc + dwconv3x3_wgrad_finalize),
// output-centric:
//   dw[c,kh,kw] = sum over (n,oh,ow) dy[n,c,oh,ow] * x[n,c,oh*s-1+kh,ow*s-1+kw]
//  * the forward's traversal: items are output row x strip, the sliding fp32
//    window runs over x (zeros outside the image, so such a term adds
//    0 * dy = +-0: absent for finite dy), one dy pack per output column, both
//    one column ahead.  72 fp32 accumulators per lane (9 taps x 8 channels),
//    each taking one term per output column in the thread's item order.
//  * flush rule: the PLAN bounds a thread to kWgMaxTrips = MSBN_ACC_FLUSH /
//    strip items of a chunk, so no fp32 accumulator takes more than
//    MSBN_ACC_FLUSH terms before the block ends; it then moves to fp64 once.
//    (72 fp64 totals per thread fit neither registers nor, at 147 KiB, LDS.)
//    The price is a chunk of at most 8 * rpi items: the workspace is
//    9/(16 * rpi * s^2) of x's bytes at full strips, 1.8 % / 3.5 % at
//    lpr = 8 / 16 and stride 1.
//  * the thread rows' sums are added in fp64 through the [k][tid] split-plane
//    LDS tree of the NHWC reduce kernels, tap after tap over the same 8
//    planes (16 KiB).  One fp64 per (channel, tap, chunk):
//    ws[C][9][nchunks], the chunk axis contiguous.  No atomics.
//  * the finalize has one wave per (channel, tap): lane l adds chunks l,
//    l + 64, .. in ascending order, a shuffle tree adds the lanes, the fp64
//    sum is rounded to T once (through an fp32 rounded to odd) into the
//    contiguous dw[C][1][3][3].
#include "bn_ops.hpp"
#include "common.hpp"
#include "launch_common.hpp"

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>

// Scalar fp32 arithmetic only in this file's device code, as in
// dwconv_stats_kernels.hip; hence the spelled-out barrier.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace msbn {

namespace {

constexpr int kGradV = 8;      // channels of a lane: one 16-byte pack
constexpr int kGradStrip = 8;  // columns of a work item (TW)
// wgrad: most items of one chunk a thread may take (one flush period)
constexpr int kWgMaxTrips = MSBN_ACC_FLUSH / kGradStrip;
static_assert(kWgMaxTrips >= 1, "a strip must fit one flush period");
static_assert(kGradStrip % 2 == 0, "stride 2 reads a strip's column parity "
                                   "off the unrolled index");

__device__ __forceinline__ void dg_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// 16 bytes of x, dy or w; all zero until something is loaded into it
template <typename T>
union DgPack {
  Pack<T, kGradV> pk;
  int __attribute__((vector_size(16))) raw;
  __device__ __forceinline__ DgPack() : raw{0, 0, 0, 0} {}
};

// this lane's weights as fp32 [tap][k]: 72 contiguous values from w + 9 c
template <typename T>
__device__ __forceinline__ void dg_load_weights(const T* __restrict__ w, int c,
                                                float (&wf)[9][kGradV]) {
  constexpr int V = kGradV;
  DgPack<T> wp[9];
#pragma unroll
  for (int i = 0; i < 9; ++i)
    wp[i].pk = *reinterpret_cast<const Pack<T, V>*>(w + (int64_t)c * 9 + i * V);
#pragma unroll
  for (int k = 0; k < V; ++k)
#pragma unroll
    for (int t = 0; t < 9; ++t)
      wf[t][k] = to_f(wp[(k * 9 + t) / V].pk.v[(k * 9 + t) % V]);
}

// ---- data gradient, stride 1: one item ------------------------------------
// gy = dy + c; dxp = the item's first dx pack
template <typename T>
__device__ __forceinline__ void dg_item_s1(const T* __restrict__ gy,
                                           T* __restrict__ dxp,
                                           const float (&wf)[9][kGradV], int n,
                                           int ih, int iw0, int nvalid, int OH,
                                           int OW, int C) {
  constexpr int V = kGradV;
  constexpr int TW = kGradStrip;
  // the three dy rows oh = ih - 1 + r (tap kh = 2 - r)
  bool rok[3];
  const T* gr[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int oh = ih - 1 + r;
    rok[r] = oh >= 0 && oh < OH;
    gr[r] = gy + ((int64_t)n * OH + (rok[r] ? oh : 0)) * OW * C;
  }
  auto load_col = [&](DgPack<T>(&col)[3], int ow, bool want) {
    const bool cok = want && ow >= 0 && ow < OW;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      DgPack<T> v;
      if (cok && rok[r]) v.pk = nt_load<T, V>(gr[r] + (int64_t)ow * C);
      col[r] = v;
    }
  };
  auto to_window = [&](float(&dst)[3][V], const DgPack<T>(&col)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < V; ++k) dst[r][k] = to_f(col[r].pk.v[k]);
  };

  float win[3][3][V];  // [cw][r][k]: dy column iw - 1 + cw (tap kw = 2 - cw)
  {
    DgPack<T> first[3][3];
#pragma unroll
    for (int cw = 0; cw < 3; ++cw) load_col(first[cw], iw0 - 1 + cw, true);
#pragma unroll
    for (int cw = 0; cw < 3; ++cw) to_window(win[cw], first[cw]);
  }
#pragma unroll
  for (int j = 0; j < TW; ++j) {
    // the column dx column j + 1 adds, in flight during column j's FMAs
    DgPack<T> nxt[3];
    if (j + 1 < TW) load_col(nxt, iw0 + j + 2, j + 1 < nvalid);
    if (j < nvalid) {
      DgPack<T> out;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float a = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int cw = 0; cw < 3; ++cw)
            a += win[cw][r][k] * wf[(2 - r) * 3 + (2 - cw)][k];
        out.pk.v[k] = from_f<T>(a);
      }
      nt_store<T, V>(dxp + (int64_t)j * C, out.pk);
    }
    if (j + 1 < TW) {
#pragma unroll
      for (int cw = 0; cw < 2; ++cw)
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int k = 0; k < V; ++k) win[cw][r][k] = win[cw + 1][r][k];
      to_window(win[2], nxt);
    }
  }
}

// ---- data gradient, stride 2: one item of row parity ODD ------------------
// iw0 is a multiple of kGradStrip, so dx column j of the strip has j's parity
template <typename T, bool ODD>
__device__ __forceinline__ void dg_item_s2(const T* __restrict__ gy,
                                           T* __restrict__ dxp,
                                           const float (&wf)[9][kGradV], int n,
                                           int ih, int iw0, int nvalid, int OH,
                                           int OW, int C) {
  constexpr int V = kGradV;
  constexpr int TW = kGradStrip;
  constexpr int NR = ODD ? 2 : 1;      // dy rows of the item
  constexpr int NQ = TW / 2 + 1;       // dy columns of the item
  // rows ascending.  even ih: oh = ih/2 (kh 1).  odd ih: oh = (ih-1)/2 (kh 2),
  // then oh = (ih+1)/2 (kh 0), which is OH for the last row of an even H.
  bool rok[NR];
  const T* gr[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int oh = ODD ? (ih - 1) / 2 + r : ih / 2;
    rok[r] = oh < OH;
    gr[r] = gy + ((int64_t)n * OH + (rok[r] ? oh : 0)) * OW * C;
  }
  // dy column q is ow = iw0/2 + q; dx column j reads q = j/2 (even j, kw 1) or
  // q = (j-1)/2 (kw 2) and (j+1)/2 (kw 0): column q serves j >= 2q - 1
  const int owb = iw0 / 2;
  DgPack<T> d[NR][NQ];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (rok[r] && owb + q < OW && 2 * q - 1 < nvalid)
        d[r][q].pk = nt_load<T, V>(gr[r] + (int64_t)(owb + q) * C);
  float df[NR][NQ][V];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int k = 0; k < V; ++k) df[r][q][k] = to_f(d[r][q].pk.v[k]);

#pragma unroll
  for (int j = 0; j < TW; ++j) {
    if (j < nvalid) {
      DgPack<T> out;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float a = 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int kh = ODD ? (r == 0 ? 2 : 0) : 1;
          if (j % 2 == 0) {
            a += df[r][j / 2][k] * wf[kh * 3 + 1][k];
          } else {
            a += df[r][(j - 1) / 2][k] * wf[kh * 3 + 2][k];
            a += df[r][(j + 1) / 2][k] * wf[kh * 3 + 0][k];
          }
        }
        out.pk.v[k] = from_f<T>(a);
      }
      nt_store<T, V>(dxp + (int64_t)j * C, out.pk);
    }
  }
}

// =====================================================================
// grid (ctiles, nchunks) block 256; lpr a power of two dividing 256
// dy [N][OH][OW][C], w [C][1][3][3], dx [N][H][W][C]
// spr = strips per dx row; items = N * H * spr (< 2^31 - 256)
// =====================================================================
template <typename T, int S>
__global__ __launch_bounds__(MSBN_BLOCK, 2) void dwconv3x3_dgrad_nhwc(
    const T* __restrict__ dy, const T* __restrict__ w, T* __restrict__ dx,
    int H, int W, int C, int OH, int OW, int spr, int items, int chunk_items,
    int lpr) {
  constexpr int V = kGradV;
  constexpr int TW = kGradStrip;
  const int rpi = MSBN_BLOCK / lpr;
  const int lane = threadIdx.x & (lpr - 1);
  const int rowoff = threadIdx.x / lpr;
  const int c = (blockIdx.x * lpr + lane) * V;
  if (c >= C) return;  // C is a multiple of V; the kernel has no barrier

  float wf[9][V];
  dg_load_weights<T>(w, c, wf);

  const int i0 = blockIdx.y * chunk_items;
  const int i1 = items - i0 < chunk_items ? items : i0 + chunk_items;
  for (int item = i0 + rowoff; item < i1; item += rpi) {
    const int irow = item / spr;  // n * H + ih
    const int iw0 = (item - irow * spr) * TW;
    const int n = irow / H;
    const int ih = irow - n * H;
    const int nvalid = W - iw0 < TW ? W - iw0 : TW;  // >= 1
    T* dxp = dx + ((int64_t)irow * W + iw0) * C + c;
    if (S == 1)
      dg_item_s1<T>(dy + c, dxp, wf, n, ih, iw0, nvalid, OH, OW, C);
    else if (ih & 1)
      dg_item_s2<T, true>(dy + c, dxp, wf, n, ih, iw0, nvalid, OH, OW, C);
    else
      dg_item_s2<T, false>(dy + c, dxp, wf, n, ih, iw0, nvalid, OH, OW, C);
  }
}

// =====================================================================
// grid (nchunks, ctiles) block 256; lpr a power of two dividing 256
// x [N][H][W][C], dy [N][OH][OW][C], ws [C][9][nchunks]
// spr = strips per dy row; items = N * OH * spr (< 2^31 - 256); the plan
// keeps chunk_items <= kWgMaxTrips * rpi
// =====================================================================
template <typename T, int S>
__global__ __launch_bounds__(MSBN_BLOCK, 2) void dwconv3x3_wgrad_partial_nhwc(
    const T* __restrict__ x, const T* __restrict__ dy, double* __restrict__ ws,
    int H, int W, int C, int OH, int OW, int spr, int items, int chunk_items,
    int lpr, int nchunks) {
  constexpr int V = kGradV;
  constexpr int TW = kGradStrip;
  constexpr int NEWC = S;  // window columns an output column adds
  const int rpi = MSBN_BLOCK / lpr;
  const int lane = threadIdx.x & (lpr - 1);
  const int rowoff = threadIdx.x / lpr;
  const int c = (blockIdx.y * lpr + lane) * V;
  const bool inb = c < C;

  __shared__ double sdata[MSBN_BLOCK * V];

  float acc[9][V];  // [kh * 3 + kw][k]
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int k = 0; k < V; ++k) acc[t][k] = 0.f;

  if (inb) {
    const int i0 = blockIdx.x * chunk_items;
    const int i1 = items - i0 < chunk_items ? items : i0 + chunk_items;
    for (int item = i0 + rowoff; item < i1; item += rpi) {
      const int orow = item / spr;  // n * OH + oh
      const int ow0 = (item - orow * spr) * TW;
      const int n = orow / OH;
      const int oh = orow - n * OH;
      const int nvalid = OW - ow0 < TW ? OW - ow0 : TW;  // >= 1

      bool rok[3];
      const T* xr[3];
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int ih = oh * S - 1 + kh;
        rok[kh] = ih >= 0 && ih < H;
        xr[kh] = x + ((int64_t)n * H + (rok[kh] ? ih : 0)) * W * C + c;
      }
      const T* gp = dy + ((int64_t)orow * OW + ow0) * C + c;

      auto load_col = [&](DgPack<T>(&col)[3], int iw, bool want) {
        const bool cok = want && iw >= 0 && iw < W;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          DgPack<T> v;
          if (cok && rok[kh]) v.pk = nt_load<T, V>(xr[kh] + (int64_t)iw * C);
          col[kh] = v;
        }
      };
      auto to_window = [&](float(&dst)[3][V], const DgPack<T>(&col)[3]) {
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int k = 0; k < V; ++k) dst[kh][k] = to_f(col[kh].pk.v[k]);
      };

      float win[3][3][V];  // [kw][kh][k]
      DgPack<T> g;         // dy of the current output column
      {
        DgPack<T> first[3][3];
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
          load_col(first[kw], ow0 * S - 1 + kw, true);
        g.pk = nt_load<T, V>(gp);
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) to_window(win[kw], first[kw]);
      }

#pragma unroll
      for (int j = 0; j < TW; ++j) {
        // what output column j + 1 needs, in flight during column j's FMAs
        DgPack<T> nxt[NEWC][3];
        DgPack<T> gnxt;
        if (j + 1 < TW) {
          const bool want = j + 1 < nvalid;
#pragma unroll
          for (int q = 0; q < NEWC; ++q)
            load_col(nxt[q], (ow0 + j + 1) * S - 1 + (3 - NEWC) + q, want);
          if (want) gnxt.pk = nt_load<T, V>(gp + (int64_t)(j + 1) * C);
        }
        if (j < nvalid) {
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const float gv = to_f(g.pk.v[k]);
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
              for (int kw = 0; kw < 3; ++kw)
                acc[kh * 3 + kw][k] += win[kw][kh][k] * gv;
          }
        }
        if (j + 1 < TW) {
#pragma unroll
          for (int kw = 0; kw < 3 - NEWC; ++kw)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
              for (int k = 0; k < V; ++k)
                win[kw][kh][k] = win[kw + NEWC][kh][k];
#pragma unroll
          for (int q = 0; q < NEWC; ++q) to_window(win[3 - NEWC + q], nxt[q]);
          g = gnxt;
        }
      }
    }
  }

  // ---- thread rows -> one value per (channel, tap): [k][tid] planes, tap
  // after tap.  The barrier that ends a tap's tree also orders its last
  // reads before the next tap's writes.
#pragma unroll
  for (int t = 0; t < 9; ++t) {
#pragma unroll
    for (int k = 0; k < V; ++k)
      sdata[k * MSBN_BLOCK + threadIdx.x] = (double)acc[t][k];
    for (int st = 1; st < rpi; st <<= 1) {
      dg_sync();
      if ((rowoff & ((st << 1) - 1)) == 0 && rowoff + st < rpi) {
        const int other = threadIdx.x + st * lpr;
#pragma unroll
        for (int k = 0; k < V; ++k)
          sdata[k * MSBN_BLOCK + threadIdx.x] += sdata[k * MSBN_BLOCK + other];
      }
    }
    dg_sync();
    if (rowoff == 0 && inb) {
#pragma unroll
      for (int k = 0; k < V; ++k)
        ws[((int64_t)(c + k) * 9 + t) * nchunks + blockIdx.x] =
            sdata[k * MSBN_BLOCK + threadIdx.x];
    }
  }
}

// fp64 -> T with one rounding: the fp32 nearest to s is stepped back to the
// truncated value where it was rounded away from zero, and an inexact value
// gets its last bit set (round to odd), so that the fp32 -> T rounding, which
// drops at least 13 bits, sees on which side of a tie s lies.
template <typename T>
__device__ __forceinline__ T dg_round_once(double s) {
  float f = (float)s;
  if ((double)f != s) {
    unsigned bits = __float_as_uint(f);
    if (fabs((double)f) > fabs(s)) bits -= 1;
    f = __uint_as_float(bits | 1u);
  }
  return from_f<T>(f);
}

// grid ceil(9 C / 4) block 256: one wave per (channel, tap)
template <typename T>
__global__ __launch_bounds__(MSBN_BLOCK) void dwconv3x3_wgrad_finalize(
    const double* __restrict__ ws, T* __restrict__ dw, int64_t total,
    int nchunks) {
  const int lane = threadIdx.x & (MSBN_WAVE - 1);
  const int64_t o = (int64_t)blockIdx.x * (MSBN_BLOCK / MSBN_WAVE) +
                    (threadIdx.x >> 6);
  if (o >= total) return;  // a whole wave leaves; no barrier follows
  const double* p = ws + o * nchunks;
  double s = 0.0;
  for (int j = lane; j < nchunks; j += MSBN_WAVE) s += p[j];
#pragma unroll
  for (int off = MSBN_WAVE / 2; off > 0; off >>= 1)
    s += __shfl_down(s, off, MSBN_WAVE);
  if (lane == 0) dw[o] = dg_round_once<T>(s);
}

inline int64_t dg_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

void dg_check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "dwconv3x3_backward: ", what, ": ",
              hipGetErrorString(e));
}

template <typename T, int S>
void dg_launch_dgrad(const DwConvPlan& p, const at::Tensor& gy,
                     const at::Tensor& w, at::Tensor& dx) {
  hipLaunchKernelGGL((dwconv3x3_dgrad_nhwc<T, S>),
                     dim3((unsigned)p.ctiles, (unsigned)p.nchunks),
                     dim3(MSBN_BLOCK), 0,
                     c10::hip::getCurrentHIPStream().stream(),
                     reinterpret_cast<const T*>(gy.data_ptr()),
                     reinterpret_cast<const T*>(w.data_ptr()),
                     reinterpret_cast<T*>(dx.data_ptr()), (int)p.h, (int)p.w,
                     (int)p.c, (int)p.oh, (int)p.ow,
                     (int)(p.items / (p.n * p.h)), (int)p.items,
                     (int)p.chunk_items, p.lpr);
  dg_check_launch("dgrad launch");
}

template <typename T, int S>
void dg_launch_wgrad(const DwConvPlan& p, const at::Tensor& x,
                     const at::Tensor& gy, at::Tensor& ws, at::Tensor& dw) {
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL((dwconv3x3_wgrad_partial_nhwc<T, S>),
                     dim3((unsigned)p.nchunks, (unsigned)p.ctiles),
                     dim3(MSBN_BLOCK), 0, stream,
                     reinterpret_cast<const T*>(x.data_ptr()),
                     reinterpret_cast<const T*>(gy.data_ptr()),
                     ws.data_ptr<double>(), (int)p.h, (int)p.w, (int)p.c,
                     (int)p.oh, (int)p.ow, (int)(p.items / (p.n * p.oh)),
                     (int)p.items, (int)p.chunk_items, p.lpr, p.nchunks);
  dg_check_launch("wgrad partial launch");
  const int64_t total = p.c * 9;
  hipLaunchKernelGGL((dwconv3x3_wgrad_finalize<T>),
                     dim3((unsigned)dg_cdiv(total, MSBN_BLOCK / MSBN_WAVE)),
                     dim3(MSBN_BLOCK), 0, stream, ws.data_ptr<double>(),
                     reinterpret_cast<T*>(dw.data_ptr()), total, p.nchunks);
  dg_check_launch("wgrad finalize launch");
}

// What both plans share: the forward's checks on (x, weight, stride) and its
// geometry, then grad_y a dense channels-last [N, C, OH, OW] of x's dtype and
// device at a 16-byte aligned address.
DwConvPlan dg_base_plan(const at::Tensor& input, const at::Tensor& weight,
                        const at::Tensor& grad_y, int64_t stride) {
  DwConvPlan p = dwconv3x3_plan(input, weight, stride);
  if (!p.ok) return p;
  p.ok = false;
  if (!grad_y.defined() || grad_y.dim() != 4) return p;
  if (grad_y.size(0) != p.n || grad_y.size(1) != p.c ||
      grad_y.size(2) != p.oh || grad_y.size(3) != p.ow)
    return p;
  if (grad_y.scalar_type() != input.scalar_type() ||
      grad_y.device() != input.device())
    return p;
  if (!grad_y.is_contiguous(at::MemoryFormat::ChannelsLast)) return p;
  if ((uintptr_t)grad_y.data_ptr() % 16 != 0) return p;
  p.strip = kGradStrip;
  p.ok = true;
  return p;
}

// the NHWC reductions' chunk rule over `pixels` elements per channel, no more
// chunks than give every thread row an item, at most `cap` items per chunk
void dg_chunks(DwConvPlan& p, int64_t pixels, int64_t cap) {
  const int rpi = MSBN_BLOCK / p.lpr;
  const int64_t per_tile = std::max<int64_t>(1, kTargetBlocks / p.ctiles);
  const int64_t max_chunks = std::min(
      dg_cdiv(pixels, std::max<int64_t>(4 * rpi, 16)), dg_cdiv(p.items, rpi));
  const int64_t nchunks =
      std::max<int64_t>(1, std::min(per_tile, std::max<int64_t>(max_chunks, 1)));
  p.chunk_items = std::min(dg_cdiv(p.items, nchunks), cap);
  p.nchunks = (int)dg_cdiv(p.items, p.chunk_items);
  p.trips = (int)dg_cdiv(p.chunk_items, rpi);
}

}  // namespace

DwConvPlan dwconv3x3_dgrad_plan(const at::Tensor& input,
                                const at::Tensor& weight,
                                const at::Tensor& grad_y, int64_t stride) {
  DwConvPlan p = dg_base_plan(input, weight, grad_y, stride);
  if (!p.ok) return p;
  // items run over dx: one row of one image x a strip of columns
  p.items = p.n * p.h * dg_cdiv(p.w, kGradStrip);
  if (p.items >= (int64_t)INT32_MAX - MSBN_BLOCK) {
    p.ok = false;
    return p;
  }
  dg_chunks(p, p.n * p.h * p.w, p.items);
  p.flush_every = 9;  // the taps of one element; nothing is summed further
  return p;
}

DwConvPlan dwconv3x3_wgrad_plan(const at::Tensor& input,
                                const at::Tensor& weight,
                                const at::Tensor& grad_y, int64_t stride) {
  DwConvPlan p = dg_base_plan(input, weight, grad_y, stride);
  if (!p.ok) return p;
  // items run over dy as the forward's do (its plan bounded them); a thread
  // takes at most kWgMaxTrips of a chunk: one flush period of fp32 terms
  const int rpi = MSBN_BLOCK / p.lpr;
  dg_chunks(p, p.n * p.oh * p.ow, (int64_t)kWgMaxTrips * rpi);
  p.flush_every = kWgMaxTrips * kGradStrip;
  return p;
}

std::tuple<at::Tensor, at::Tensor> dwconv3x3_backward(
    const at::Tensor& grad_y, const at::Tensor& input,
    const at::Tensor& weight, int64_t stride, bool want_dx, bool want_dw) {
  at::Tensor dx, dw;
  if (!input.defined() || !input.is_cuda()) return {dx, dw};
  const DwConvPlan pd = dwconv3x3_dgrad_plan(input, weight, grad_y, stride);
  const DwConvPlan pw = dwconv3x3_wgrad_plan(input, weight, grad_y, stride);
  if (!pd.ok || !pw.ok) return {dx, dw};
  at::Tensor ws;
  if (want_dx)
    dx = at::empty(
        {pd.n, pd.c, pd.h, pd.w},
        input.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (want_dw) {
    dw = at::empty({pw.c, 1, 3, 3}, weight.options());
    ws = at::empty({pw.c, 9, (int64_t)pw.nchunks},
                   input.options().dtype(at::kDouble));
  }
  auto go = [&](auto tag) {
    using T = decltype(tag);
    if (want_dx) {
      if (pd.stride == 1)
        dg_launch_dgrad<T, 1>(pd, grad_y, weight, dx);
      else
        dg_launch_dgrad<T, 2>(pd, grad_y, weight, dx);
    }
    if (want_dw) {
      if (pw.stride == 1)
        dg_launch_wgrad<T, 1>(pw, input, grad_y, ws, dw);
      else
        dg_launch_wgrad<T, 2>(pw, input, grad_y, ws, dw);
    }
  };
  if (input.scalar_type() == at::kBFloat16)
    go(__hip_bfloat16{});
  else
    go(__half{});
  return {dx, dw};
}

}  // namespace msbn

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
