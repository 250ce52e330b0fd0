// Depthwise 5x5 convolution (padding 2, stride 1 or 2, channel multiplier 1)
// that emits the following BatchNorm's statistics, and its two gradients
// (gfx950, CDNA4).  docs/KERNEL_DESIGN.md "Depthwise 5x5".
//
// 25 FMAs per output element put this kernel where the FMA rate and HBM meet,
// so unlike its 3x3 siblings it is built around LDS:
//
//  * block 256, lpr lanes across the channel axis (one 16-byte pack of 8
//    channels each; lpr = min(nhwc_lanes_per_row, 16)), rpi = 256 / lpr thread
//    rows.  grid (channel tiles, chunks); a chunk is a contiguous run of work
//    items, an item is a TILE of TH x TW output pixels of one image.
//  * per item the block stages the halo tile, ((TH-1)*s + 5) x ((TW-1)*s + 5)
//    pixels x lpr packs, into LDS as raw T with 16-byte nontemporal loads
//    (zeros made in registers for what lies outside the image: nothing is
//    read across an image boundary), layout [row][col][lane].  Every input
//    element is loaded from memory once per tile it touches: 1.56x (lpr 8,
//    16 x 16 tile) or 1.88x (lpr 16, 8 x 16 tile) of x at stride 1.
//  * a thread row owns one strip of SW output columns of one tile row
//    (SW = 8 at stride 1, 2 at stride 2: TH * TW / SW == rpi).  It keeps
//    acc[SW][8] fp32, walks kh, then the (SW-1)*s + 5 input columns of that
//    row, converts each 16-byte LDS pack once and FMAs it into the outputs
//    that use it.  Only the current kh row of weights (5 x 8 fp32) is in
//    registers; the 25 weight packs sit in LDS, transposed to [tap][lane][k].
//    Per output element: kh ascending, then kw ascending, one accumulator,
//    rounded to T once.
//  * statistics as in the 3x3 forward: of the rounded values, always shifted
//    by the thread's first stored value, fp32 for at most MSBN_ACC_FLUSH
//    terms, then fp64 (registers), un-shifted in fp64, the [k][tid] LDS tree
//    (which reuses the tile's LDS), ws[C][nchunks][2].  No atomics.
//  * data gradient, stride 1: the same kernel over dy with the weights
//    flipped while they are staged (FLIP), no statistics.
//  * data gradient, stride 2: tiles of dx; a dx element takes the taps of its
//    row and column parity only (kh = ih mod 2 + 2i).  The column parity is
//    that of the unrolled column index, the row parity sets the trip count of
//    the dy-row loop (3 or 2): 20 FMAs per dy row instead of 40, none masked.
//  * weight gradient: tiles of dy, the x halo tile and the dy tile in LDS.
//    Thread row r works for tap row kh = r % 5 in group g = r / 5: it holds
//    acc[5 kw][8] fp32 and visits the strips g, g + groups, .. of the tile.
//    After EVERY tile (at most trips * strip <= 64 terms per accumulator) the
//    block moves all 25 taps to fp64 in one round: the accumulators go to an
//    fp32 LDS table [group][tap][lane][k], and each thread adds the groups'
//    values, in ascending order, into the fp64 totals of the (tap, channel)
//    entries it owns -- 13 registers, the block's totals never leave them
//    until the chunk ends.  Two barriers per round, no tree.
//    ws[C][25][nchunks], then one wave per (channel, tap) finalizes.
#include "bn_ops.hpp"
#include "common.hpp"
#include "launch_common.hpp"

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <type_traits>

// Scalar fp32 arithmetic only, as in the 3x3 files: the documented
// accumulation order is then the order of the instructions.  Hence the
// spelled-out barrier.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace msbn {

namespace {

constexpr int kD5V = 8;        // channels of a lane: one 16-byte pack
constexpr int kD5Taps = 25;
constexpr int kD5MaxLpr = 16;  // LDS: a tile's bytes grow with lpr
constexpr int kD5TilePacks = 3840;   // forward / dgrad tile: 60 KiB
constexpr int kD5WgradPacks = 4096;  // wgrad x + dy tiles: 64 KiB
// chunks aimed at: two rounds of the 2 x 256 blocks the device holds
constexpr int kD5TargetBlocks = 1024;
// wgrad: fp64 totals a thread owns, ceil(25 * 16 * 8 / 256)
constexpr int kD5Tot = (kD5Taps * kD5MaxLpr * kD5V + MSBN_BLOCK - 1) / MSBN_BLOCK;

constexpr int d5_strip(int s) { return s == 1 ? 8 : 2; }
// forward: tiles between two flushes of a thread's fp32 sums (strip terms
// each: 64 at stride 1, 16 at stride 2)
constexpr int kD5FlushTiles = 8;

using d5_vec = int __attribute__((vector_size(16)));

__device__ __forceinline__ void d5_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// 16 bytes of x, dy or w; all zero until something is loaded into it
template <typename T>
union D5Pack {
  Pack<T, kD5V> pk;
  d5_vec raw;
  __device__ __forceinline__ D5Pack() : raw{0, 0, 0, 0} {}
};

template <typename T>
__device__ __forceinline__ void d5_to_f(float (&f)[kD5V], d5_vec raw) {
  D5Pack<T> p;
  p.raw = raw;
#pragma unroll
  for (int k = 0; k < kD5V; ++k) f[k] = to_f(p.pk.v[k]);
}

// Rows [r0, r0 + nr) x columns [c0, c0 + nc) of image plane `img` (= n * SH)
// of src [N][SH][SWD][C] -> tile[(r * nc + col) * lpr + lane], zero outside
// the image.  Thread row `rowoff` takes pixels rowoff, rowoff + rpi, ..; four
// loads are in flight before the first LDS write.
template <typename T>
__device__ __forceinline__ void d5_stage(d5_vec* tile, const T* __restrict__ src,
                                         bool inb, int64_t img, int SH, int SWD,
                                         int C, int c, int r0, int c0, int nr,
                                         int nc, int lpr, int lane, int rowoff,
                                         int rpi) {
  const int npx = nr * nc;
  for (int p0 = rowoff; p0 < npx; p0 += 4 * rpi) {
    D5Pack<T> v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int px = p0 + u * rpi;
      const int r = px / nc;
      const int ih = r0 + r, iw = c0 + (px - r * nc);
      if (inb && px < npx && ih >= 0 && ih < SH && iw >= 0 && iw < SWD)
        v[u].pk = nt_load<T, kD5V>(src + ((img + ih) * SWD + iw) * C + c);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int px = p0 + u * rpi;
      if (px < npx) tile[px * lpr + lane] = v[u].raw;
    }
  }
}

// The block's weights, w[c][0][kh][kw] for its lpr * 8 channels, transposed
// into wl[tap][lane][k] (cached loads; zero past C).  FLIP stores tap 24 - t.
template <typename T, bool FLIP>
__device__ __forceinline__ void d5_stage_weights(d5_vec* wl,
                                                 const T* __restrict__ w, int C,
                                                 int lpr) {
  T* wt = reinterpret_cast<T*>(wl);
  for (int i = threadIdx.x; i < kD5Taps * lpr * kD5V; i += MSBN_BLOCK) {
    const int k = i & (kD5V - 1);
    const int ln = (i / kD5V) & (lpr - 1);
    const int t = i / (kD5V * lpr);
    const int cc = (blockIdx.x * lpr + ln) * kD5V + k;
    wt[i] = cc < C ? w[(int64_t)cc * kD5Taps + (FLIP ? kD5Taps - 1 - t : t)]
                   : from_f<T>(0.f);
  }
}

// item -> (n, first output row, first output column) of its tile
__device__ __forceinline__ void d5_tile_of(int item, int tiles_h, int tiles_w,
                                           int TH, int TW, int& n, int& r0,
                                           int& c0) {
  const int per_img = tiles_h * tiles_w;
  n = item / per_img;
  const int rem = item - n * per_img;
  const int th = rem / tiles_w;
  r0 = th * TH;
  c0 = (rem - th * tiles_w) * TW;
}

// =====================================================================
// Forward (+ statistics) and the stride-1 data gradient.
// grid (ctiles, nchunks) block 256; lpr in {8, 16}
// x [N][H][W][C], w [C][1][5][5], y [N][OH][OW][C], ws [C][nchunks][2]
// TH * (TW / SW) == 256 / lpr; ((TH-1)*S+5) * ((TW-1)*S+5) * lpr <= 3840
// =====================================================================
template <typename T, int S, bool FLIP, bool STATS>
__global__ __launch_bounds__(MSBN_BLOCK, 2) void dwconv5x5_tile_nhwc(
    const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y,
    double* __restrict__ ws, int H, int W, int C, int OH, int OW, int TH,
    int TW, int tiles_h, int tiles_w, int items, int chunk_items, int lpr,
    int nchunks) {
  constexpr int V = kD5V;
  constexpr int SW = d5_strip(S);
  constexpr int NC = (SW - 1) * S + 5;  // input columns of a strip
  constexpr int kFlushTiles = kD5FlushTiles;
  static_assert(kFlushTiles * SW <= MSBN_ACC_FLUSH, "one flush period");
  const int rpi = MSBN_BLOCK / lpr;
  const int lane = threadIdx.x & (lpr - 1);
  const int rowoff = threadIdx.x / lpr;
  const int c = (blockIdx.x * lpr + lane) * V;
  const bool inb = c < C;  // C is a multiple of V: a pack is in or out whole

  __shared__ d5_vec tile[kD5TilePacks];
  __shared__ d5_vec wl[kD5Taps * kD5MaxLpr];

  d5_stage_weights<T, FLIP>(wl, w, C, lpr);

  const int IWT = (TW - 1) * S + 5;  // tile pitch in pixels
  const int spt = TW / SW;           // strips of a tile row
  const int trow = rowoff / spt;
  const int tcol = (rowoff - trow * spt) * SW;

  float fa[V], fb[V], pivot[V];
  double ta[V], tb[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    fa[k] = fb[k] = pivot[k] = 0.f;
    ta[k] = tb[k] = 0.0;
  }
  auto flush = [&]() {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      ta[k] += (double)fa[k];
      tb[k] += (double)fb[k];
      fa[k] = fb[k] = 0.f;
    }
  };
  bool have_pivot = false;
  int cnt = 0;  // values this thread has summed, per channel
  int since_flush = 0;

  const int i0 = blockIdx.y * chunk_items;
  const int i1 = items - i0 < chunk_items ? items : i0 + chunk_items;
  for (int item = i0; item < i1; ++item) {  // uniform over the block
    int n, oh0, ow0;
    d5_tile_of(item, tiles_h, tiles_w, TH, TW, n, oh0, ow0);
    const int nrow = OH - oh0 < TH ? OH - oh0 : TH;  // output rows in range
    // the previous tile's reads (first trip: the weights' writes) are done
    d5_sync();
    d5_stage<T>(tile, x, inb, (int64_t)n * H, H, W, C, c, oh0 * S - 2,
                ow0 * S - 2, (nrow - 1) * S + 5, IWT, lpr, lane, rowoff, rpi);
    d5_sync();

    const int oh = oh0 + trow, ow = ow0 + tcol;
    if (inb && oh < OH && ow < OW) {
      float acc[SW][V];
#pragma unroll
      for (int o = 0; o < SW; ++o)
#pragma unroll
        for (int k = 0; k < V; ++k) acc[o][k] = 0.f;
      // one kh row at a time: unrolled over kh, the LDS reads of all five rows
      // are hoisted and the registers spill
#pragma unroll 1
      for (int kh = 0; kh < 5; ++kh) {
        float wf[5][V];
#pragma unroll
        for (int kw = 0; kw < 5; ++kw)
          d5_to_f<T>(wf[kw], wl[(kh * 5 + kw) * lpr + lane]);
        const d5_vec* row =
            tile + ((trow * S + kh) * IWT + tcol * S) * lpr + lane;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          float xf[V];
          d5_to_f<T>(xf, row[j * lpr]);
#pragma unroll
          for (int o = 0; o < SW; ++o) {
            const int kw = j - o * S;
            if (kw >= 0 && kw < 5) {
#pragma unroll
              for (int k = 0; k < V; ++k) acc[o][k] += xf[k] * wf[kw][k];
            }
          }
        }
      }
      const int nvalid = OW - ow < SW ? OW - ow : SW;  // >= 1
      T* yp = y + (((int64_t)n * OH + oh) * OW + ow) * C + c;
#pragma unroll
      for (int o = 0; o < SW; ++o) {
        if (o < nvalid) {
          D5Pack<T> out;
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const T r = from_f<T>(acc[o][k]);
            out.pk.v[k] = r;
            if (STATS) {
              const float v = to_f(r);
              if (o == 0 && !have_pivot) pivot[k] = v;
              const float d = v - pivot[k];
              fa[k] += d;
              fb[k] += d * d;
            }
          }
          if (o == 0) have_pivot = true;
          nt_store<T, V>(yp + (int64_t)o * C, out.pk);
        }
      }
      cnt += nvalid;
    }
    if (STATS && ++since_flush == kFlushTiles) {
      flush();
      since_flush = 0;
    }
  }

  if (!STATS) return;  // uniform: no barrier follows
  flush();
  d5_sync();  // the last tile's reads are done: the planes reuse its LDS
  double* sdata = reinterpret_cast<double*>(tile);
  static_assert(MSBN_BLOCK * V * 2 * sizeof(double) <=
                    kD5TilePacks * sizeof(d5_vec),
                "the statistics planes must fit the tile");
#pragma unroll
  for (int k = 0; k < V; ++k) {
    // cnt == 0: pivot and both sums are zero, and stay so
    unshift_pair(ta[k], tb[k], pivot[k], (double)cnt);
    sdata[k * MSBN_BLOCK + threadIdx.x] = ta[k];
    sdata[(V + k) * MSBN_BLOCK + threadIdx.x] = tb[k];
  }
  // ---- thread rows -> one pair per channel: [k][tid] planes ----
  for (int st = 1; st < rpi; st <<= 1) {
    d5_sync();
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
  d5_sync();
  if (rowoff == 0 && inb) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      double* out = ws + ((int64_t)(c + k) * nchunks + blockIdx.y) * 2;
      out[0] = sdata[k * MSBN_BLOCK + threadIdx.x];
      out[1] = sdata[(V + k) * MSBN_BLOCK + threadIdx.x];
    }
  }
}

// =====================================================================
// Data gradient, stride 2.  grid (ctiles, nchunks) block 256
// dy [N][OH][OW][C], w [C][1][5][5], dx [N][H][W][C]
// tiles of TH x TW dx pixels, TH even, TW a multiple of 8,
// TH * (TW / 8) == 256 / lpr; the dy tile is (TH/2 + 2) x (TW/2 + 2).
// ih = 2 oh - 2 + kh: even ih takes kh 4, 2, 0 at oh = ih/2 - 1, ih/2,
// ih/2 + 1; odd ih takes kh 3, 1 at oh = (ih-1)/2, (ih+1)/2.  Columns alike.
// Order: dy rows ascending, within a row dy columns ascending.
// =====================================================================
template <typename T>
__global__ __launch_bounds__(MSBN_BLOCK, 2) void dwconv5x5s2_dgrad_nhwc(
    const T* __restrict__ dy, const T* __restrict__ w, T* __restrict__ dx,
    int H, int W, int C, int OH, int OW, int TH, int TW, int tiles_h,
    int tiles_w, int items, int chunk_items, int lpr) {
  constexpr int V = kD5V;
  constexpr int SW = 8;       // dx columns of a strip
  constexpr int NQ = SW / 2 + 2;  // dy columns of a strip
  const int rpi = MSBN_BLOCK / lpr;
  const int lane = threadIdx.x & (lpr - 1);
  const int rowoff = threadIdx.x / lpr;
  const int c = (blockIdx.x * lpr + lane) * V;
  const bool inb = c < C;

  __shared__ d5_vec tile[kD5TilePacks / 4];
  __shared__ d5_vec wl[kD5Taps * kD5MaxLpr];

  d5_stage_weights<T, false>(wl, w, C, lpr);

  const int DWT = TW / 2 + 2;  // tile pitch in dy pixels
  const int spt = TW / SW;
  const int trow = rowoff / spt;
  const int tcol = (rowoff - trow * spt) * SW;
  const bool odd = trow & 1;  // ih0 is even
  const int nr = odd ? 2 : 3;

  const int i0 = blockIdx.y * chunk_items;
  const int i1 = items - i0 < chunk_items ? items : i0 + chunk_items;
  for (int item = i0; item < i1; ++item) {
    int n, ih0, iw0;
    d5_tile_of(item, tiles_h, tiles_w, TH, TW, n, ih0, iw0);
    d5_sync();
    d5_stage<T>(tile, dy, inb, (int64_t)n * OH, OH, OW, C, c, ih0 / 2 - 1,
                iw0 / 2 - 1, TH / 2 + 2, DWT, lpr, lane, rowoff, rpi);
    d5_sync();

    const int ih = ih0 + trow, iw = iw0 + tcol;
    if (inb && ih < H && iw < W) {
      float acc[SW][V];
#pragma unroll
      for (int j = 0; j < SW; ++j)
#pragma unroll
        for (int k = 0; k < V; ++k) acc[j][k] = 0.f;
      for (int r = 0; r < nr; ++r) {
        const int kh = (odd ? 3 : 4) - 2 * r;
        float wf[5][V];
#pragma unroll
        for (int kw = 0; kw < 5; ++kw)
          d5_to_f<T>(wf[kw], wl[(kh * 5 + kw) * lpr + lane]);
        const d5_vec* row =
            tile + ((trow / 2 + (odd ? 1 : 0) + r) * DWT + tcol / 2) * lpr +
            lane;
        // dy column q is ow = iw/2 - 1 + q; it reaches dx column j of the
        // strip through kw = j + 4 - 2 q
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          float gf[V];
          d5_to_f<T>(gf, row[q * lpr]);
#pragma unroll
          for (int j = 0; j < SW; ++j) {
            const int kw = j + 4 - 2 * q;
            if (kw >= 0 && kw < 5) {
#pragma unroll
              for (int k = 0; k < V; ++k) acc[j][k] += gf[k] * wf[kw][k];
            }
          }
        }
      }
      const int nvalid = W - iw < SW ? W - iw : SW;  // >= 1
      T* dxp = dx + (((int64_t)n * H + ih) * W + iw) * C + c;
#pragma unroll
      for (int j = 0; j < SW; ++j) {
        if (j < nvalid) {
          D5Pack<T> out;
#pragma unroll
          for (int k = 0; k < V; ++k) out.pk.v[k] = from_f<T>(acc[j][k]);
          nt_store<T, V>(dxp + (int64_t)j * C, out.pk);
        }
      }
    }
  }
}

// =====================================================================
// Weight gradient, partial stage.  grid (nchunks, ctiles) block 256
// x [N][H][W][C], dy [N][OH][OW][C], ws [C][25][nchunks]
// tiles of TH x TW dy pixels; x tile + dy tile <= 4096 packs
// =====================================================================
template <typename T, int S>
__global__ __launch_bounds__(MSBN_BLOCK, 2) void dwconv5x5_wgrad_partial_nhwc(
    const T* __restrict__ x, const T* __restrict__ dy, double* __restrict__ ws,
    int H, int W, int C, int OH, int OW, int TH, int TW, int tiles_h,
    int tiles_w, int items, int chunk_items, int lpr, int nchunks) {
  constexpr int V = kD5V;
  constexpr int SW = d5_strip(S);
  constexpr int NC = (SW - 1) * S + 5;
  const int rpi = MSBN_BLOCK / lpr;
  const int lane = threadIdx.x & (lpr - 1);
  const int rowoff = threadIdx.x / lpr;
  const int c = (blockIdx.y * lpr + lane) * V;
  const bool inb = c < C;

  __shared__ d5_vec smem[kD5WgradPacks];

  const int IHT = (TH - 1) * S + 5, IWT = (TW - 1) * S + 5;
  d5_vec* xt = smem;
  d5_vec* gt = smem + IHT * IWT * lpr;
  float* stg = reinterpret_cast<float*>(smem);  // [group][tap][lane][k]

  const int ngroups = rpi / 5;
  const int kh = rowoff % 5;
  const int grp = rowoff / 5;
  const bool active = grp < ngroups;  // rpi % 5 thread rows only stage
  const int spt = TW / SW;
  const int strips = TH * spt;
  const int E = kD5Taps * lpr * V;  // (tap, channel) entries of the block

  float acc[5][V];  // [kw][k] of this thread's kh
#pragma unroll
  for (int kw = 0; kw < 5; ++kw)
#pragma unroll
    for (int k = 0; k < V; ++k) acc[kw][k] = 0.f;
  double tot[kD5Tot];  // entries tid, tid + 256, ..
#pragma unroll
  for (int i = 0; i < kD5Tot; ++i) tot[i] = 0.0;

  const int i0 = blockIdx.x * chunk_items;
  const int i1 = items - i0 < chunk_items ? items : i0 + chunk_items;
  for (int item = i0; item < i1; ++item) {
    int n, oh0, ow0;
    d5_tile_of(item, tiles_h, tiles_w, TH, TW, n, oh0, ow0);
    d5_sync();  // the previous round's table reads are done
    d5_stage<T>(xt, x, inb, (int64_t)n * H, H, W, C, c, oh0 * S - 2,
                ow0 * S - 2, IHT, IWT, lpr, lane, rowoff, rpi);
    d5_stage<T>(gt, dy, inb, (int64_t)n * OH, OH, OW, C, c, oh0, ow0, TH, TW,
                lpr, lane, rowoff, rpi);
    d5_sync();

    if (active) {
      for (int s = grp; s < strips; s += ngroups) {
        const int trow = s / spt;
        const int tcol = (s - trow * spt) * SW;
        if (oh0 + trow >= OH || ow0 + tcol >= OW) continue;  // dy all zero
        float gv[SW][V];
#pragma unroll
        for (int o = 0; o < SW; ++o)
          d5_to_f<T>(gv[o], gt[(trow * TW + tcol + o) * lpr + lane]);
        const d5_vec* row =
            xt + ((trow * S + kh) * IWT + tcol * S) * lpr + lane;
        // columns past OW are not terms: their dy is a staged zero, but x
        // there may be in the image and need not be finite.  A full strip
        // runs without the test.
        const int nvalid = OW - (ow0 + tcol) < SW ? OW - (ow0 + tcol) : SW;
        auto fma = [&](auto full) {
#pragma unroll
          for (int j = 0; j < NC; ++j) {
            float xf[V];
            d5_to_f<T>(xf, row[j * lpr]);
#pragma unroll
            for (int o = 0; o < SW; ++o) {
              const int kw = j - o * S;
              if (kw >= 0 && kw < 5 && (decltype(full)::value || o < nvalid)) {
#pragma unroll
                for (int k = 0; k < V; ++k) acc[kw][k] += xf[k] * gv[o][k];
              }
            }
          }
        };
        if (nvalid == SW)
          fma(std::true_type{});
        else
          fma(std::false_type{});
      }
    }
    d5_sync();  // the tiles' reads are done: the table reuses their LDS
    if (active) {
#pragma unroll
      for (int kw = 0; kw < 5; ++kw)
#pragma unroll
        for (int k = 0; k < V; ++k) {
          stg[((grp * kD5Taps + kh * 5 + kw) * lpr + lane) * V + k] =
              acc[kw][k];
          acc[kw][k] = 0.f;
        }
    }
    d5_sync();
#pragma unroll
    for (int i = 0; i < kD5Tot; ++i) {
      const int e = threadIdx.x + i * MSBN_BLOCK;
      if (e < E)
        for (int g = 0; g < ngroups; ++g) tot[i] += (double)stg[g * E + e];
    }
  }

#pragma unroll
  for (int i = 0; i < kD5Tot; ++i) {
    const int e = threadIdx.x + i * MSBN_BLOCK;
    if (e < E) {
      const int t = e / (lpr * V);
      const int ch = blockIdx.y * lpr * V + (e - t * lpr * V);
      if (ch < C)
        ws[((int64_t)ch * kD5Taps + t) * nchunks + blockIdx.x] = tot[i];
    }
  }
}

// fp64 -> T with one rounding (dwconv_grad_kernels.hip dg_round_once): the
// fp32 nearest to s, stepped back to the truncated value where it was rounded
// away from zero, last bit set when inexact (round to odd).
template <typename T>
__device__ __forceinline__ T d5_round_once(double s) {
  float f = (float)s;
  if ((double)f != s) {
    unsigned bits = __float_as_uint(f);
    if (fabs((double)f) > fabs(s)) bits -= 1;
    f = __uint_as_float(bits | 1u);
  }
  return from_f<T>(f);
}

// grid ceil(25 C / 4) block 256: one wave per (channel, tap)
template <typename T>
__global__ __launch_bounds__(MSBN_BLOCK) void dwconv5x5_wgrad_finalize(
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
  if (lane == 0) dw[o] = d5_round_once<T>(s);
}

inline int64_t d5_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

void d5_check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "dwconv5x5: ", what, ": ",
              hipGetErrorString(e));
}

// The checks on (x, weight, stride) and the geometry every plan shares.
DwConv5x5Plan d5_base_plan(const at::Tensor& input, const at::Tensor& weight,
                           int64_t stride) {
  DwConv5x5Plan p{};
  if (stride != 1 && stride != 2) return p;
  if (!input.defined() || !weight.defined()) return p;
  if (input.dim() != 4 || weight.dim() != 4 || input.numel() == 0) return p;
  const auto dt = input.scalar_type();
  if (dt != at::kBFloat16 && dt != at::kHalf) return p;
  if (weight.scalar_type() != dt || weight.device() != input.device()) return p;
  if (!input.is_contiguous(at::MemoryFormat::ChannelsLast)) return p;
  const int64_t C = input.size(1);
  if (weight.size(0) != C || weight.size(1) != 1 || weight.size(2) != 5 ||
      weight.size(3) != 5 || !weight.is_contiguous())
    return p;
  if (C % kD5V != 0 || C > (1 << 24)) return p;
  if ((uintptr_t)input.data_ptr() % 16 != 0 ||
      (uintptr_t)weight.data_ptr() % 16 != 0)
    return p;
  p.n = input.size(0);
  p.c = C;
  p.h = input.size(2);
  p.w = input.size(3);
  if (p.h >= (1 << 30) || p.w >= (1 << 30)) return p;
  p.stride = (int)stride;
  p.oh = (p.h - 1) / stride + 1;
  p.ow = (p.w - 1) / stride + 1;
  p.v = kD5V;
  p.lpr = std::min(nhwc_lanes_per_row(C, kD5V), kD5MaxLpr);
  p.ctiles = (int)d5_cdiv(C, (int64_t)p.lpr * kD5V);
  p.ok = true;
  return p;
}

// grad_y: a dense channels-last [N, C, OH, OW] of x's dtype and device at a
// 16-byte aligned address
bool d5_grad_ok(const DwConv5x5Plan& p, const at::Tensor& input,
                const at::Tensor& grad_y) {
  if (!grad_y.defined() || grad_y.dim() != 4) return false;
  if (grad_y.size(0) != p.n || grad_y.size(1) != p.c ||
      grad_y.size(2) != p.oh || grad_y.size(3) != p.ow)
    return false;
  if (grad_y.scalar_type() != input.scalar_type() ||
      grad_y.device() != input.device())
    return false;
  if (!grad_y.is_contiguous(at::MemoryFormat::ChannelsLast)) return false;
  return (uintptr_t)grad_y.data_ptr() % 16 == 0;
}

// Tiles of tile_h x tile_w over rows x cols pixels per image, and the chunks:
// about kD5TargetBlocks blocks, a chunk a contiguous run of tiles.
void d5_tiles(DwConv5x5Plan& p, int th, int tw, int64_t rows, int64_t cols) {
  p.tile_h = th;
  p.tile_w = tw;
  p.items = p.n * d5_cdiv(rows, th) * d5_cdiv(cols, tw);
  if (p.items >= (int64_t)INT32_MAX - MSBN_BLOCK) {
    p.ok = false;
    return;
  }
  const int64_t per_tile = std::max<int64_t>(1, kD5TargetBlocks / p.ctiles);
  const int64_t nchunks = std::min(per_tile, p.items);
  p.chunk_items = d5_cdiv(p.items, nchunks);
  p.nchunks = (int)d5_cdiv(p.items, p.chunk_items);
}

template <typename T, int S, bool FLIP, bool STATS>
void d5_launch_tile(const DwConv5x5Plan& p, const at::Tensor& x,
                    const at::Tensor& w, at::Tensor& y, double* ws,
                    const char* what) {
  // FLIP is the stride-1 data gradient: x is dy and y is dx, of one size
  hipLaunchKernelGGL((dwconv5x5_tile_nhwc<T, S, FLIP, STATS>),
                     dim3((unsigned)p.ctiles, (unsigned)p.nchunks),
                     dim3(MSBN_BLOCK), 0,
                     c10::hip::getCurrentHIPStream().stream(),
                     reinterpret_cast<const T*>(x.data_ptr()),
                     reinterpret_cast<const T*>(w.data_ptr()),
                     reinterpret_cast<T*>(y.data_ptr()), ws, (int)p.h,
                     (int)p.w, (int)p.c, (int)p.oh, (int)p.ow, p.tile_h,
                     p.tile_w, (int)d5_cdiv(p.oh, p.tile_h),
                     (int)d5_cdiv(p.ow, p.tile_w), (int)p.items,
                     (int)p.chunk_items, p.lpr, p.nchunks);
  d5_check_launch(what);
}

}  // namespace

DwConv5x5Plan dwconv5x5_plan(const at::Tensor& input, const at::Tensor& weight,
                             int64_t stride) {
  DwConv5x5Plan p = d5_base_plan(input, weight, stride);
  if (!p.ok) return p;
  p.strip = d5_strip(p.stride);
  // TH * TW / strip == 256 / lpr, and the halo tile within 60 KiB
  if (p.stride == 1)
    d5_tiles(p, p.lpr == 8 ? 16 : 8, 16, p.oh, p.ow);
  else
    d5_tiles(p, p.lpr == 8 ? 8 : 4, 8, p.oh, p.ow);
  p.trips = (int)p.chunk_items;
  p.flush_every = kD5FlushTiles * p.strip;
  p.lds_bytes = (kD5TilePacks + kD5Taps * kD5MaxLpr) * sizeof(d5_vec);
  return p;
}

DwConv5x5Plan dwconv5x5_dgrad_plan(const at::Tensor& input,
                                   const at::Tensor& weight,
                                   const at::Tensor& grad_y, int64_t stride) {
  DwConv5x5Plan p = d5_base_plan(input, weight, stride);
  if (!p.ok) return p;
  if (!d5_grad_ok(p, input, grad_y)) {
    p.ok = false;
    return p;
  }
  // tiles of dx; both strides give a thread row a strip of 8 dx columns
  p.strip = 8;
  d5_tiles(p, p.lpr == 8 ? 16 : 8, 16, p.h, p.w);
  p.trips = (int)p.chunk_items;
  p.flush_every = kD5Taps;  // the taps of one element; nothing is summed on
  p.lds_bytes = ((p.stride == 1 ? kD5TilePacks : kD5TilePacks / 4) +
                 kD5Taps * kD5MaxLpr) * sizeof(d5_vec);
  return p;
}

DwConv5x5Plan dwconv5x5_wgrad_plan(const at::Tensor& input,
                                   const at::Tensor& weight,
                                   const at::Tensor& grad_y, int64_t stride) {
  DwConv5x5Plan p = d5_base_plan(input, weight, stride);
  if (!p.ok) return p;
  if (!d5_grad_ok(p, input, grad_y)) {
    p.ok = false;
    return p;
  }
  p.strip = d5_strip(p.stride);
  // tiles of dy; the x halo tile and the dy tile within 64 KiB
  if (p.stride == 1)
    d5_tiles(p, 8, p.lpr == 8 ? 16 : 8, p.oh, p.ow);
  else
    d5_tiles(p, p.lpr == 8 ? 8 : 4, 8, p.oh, p.ow);
  // one round per tile: a thread visits at most `trips` strips of it, so an
  // fp32 accumulator takes trips * strip terms before it moves to fp64
  const int groups = MSBN_BLOCK / p.lpr / 5;
  p.trips = (int)d5_cdiv((int64_t)p.tile_h * p.tile_w / p.strip, groups);
  p.flush_every = MSBN_ACC_FLUSH;
  if (p.trips * p.strip > p.flush_every) p.ok = false;
  p.lds_bytes = kD5WgradPacks * sizeof(d5_vec);
  return p;
}

std::tuple<at::Tensor, at::Tensor, int64_t> dwconv5x5_stats(
    const at::Tensor& input, const at::Tensor& weight, int64_t stride) {
  if (!input.defined() || !input.is_cuda())
    return {at::Tensor(), at::Tensor(), 0};
  const DwConv5x5Plan p = dwconv5x5_plan(input, weight, stride);
  if (!p.ok) return {at::Tensor(), at::Tensor(), 0};
  at::Tensor y = at::empty(
      {p.n, p.c, p.oh, p.ow},
      input.options().memory_format(at::MemoryFormat::ChannelsLast));
  at::Tensor ws = at::empty({p.c, (int64_t)p.nchunks, 2},
                            input.options().dtype(at::kDouble));
  auto go = [&](auto tag) {
    using T = decltype(tag);
    if (p.stride == 1)
      d5_launch_tile<T, 1, false, true>(p, input, weight, y,
                                        ws.data_ptr<double>(), "stats launch");
    else
      d5_launch_tile<T, 2, false, true>(p, input, weight, y,
                                        ws.data_ptr<double>(), "stats launch");
  };
  if (input.scalar_type() == at::kBFloat16)
    go(__hip_bfloat16{});
  else
    go(__half{});
  return {y, ws, (int64_t)p.nchunks};
}

std::tuple<at::Tensor, at::Tensor> dwconv5x5_backward(
    const at::Tensor& grad_y, const at::Tensor& input,
    const at::Tensor& weight, int64_t stride, bool want_dx, bool want_dw) {
  at::Tensor dx, dw;
  if (!input.defined() || !input.is_cuda()) return {dx, dw};
  const DwConv5x5Plan pd = dwconv5x5_dgrad_plan(input, weight, grad_y, stride);
  const DwConv5x5Plan pw = dwconv5x5_wgrad_plan(input, weight, grad_y, stride);
  if (!pd.ok || !pw.ok) return {dx, dw};
  at::Tensor ws;
  if (want_dx)
    dx = at::empty(
        {pd.n, pd.c, pd.h, pd.w},
        input.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (want_dw) {
    dw = at::empty({pw.c, 1, 5, 5}, weight.options());
    ws = at::empty({pw.c, kD5Taps, (int64_t)pw.nchunks},
                   input.options().dtype(at::kDouble));
  }
  auto stream = c10::hip::getCurrentHIPStream().stream();
  auto go = [&](auto tag) {
    using T = decltype(tag);
    if (want_dx && pd.stride == 1) {
      // the forward over dy (p.h x p.w both ways) with flipped weights
      DwConv5x5Plan q = pd;
      q.oh = pd.h;
      q.ow = pd.w;
      d5_launch_tile<T, 1, true, false>(q, grad_y, weight, dx, nullptr,
                                        "dgrad launch");
    } else if (want_dx) {
      hipLaunchKernelGGL(
          (dwconv5x5s2_dgrad_nhwc<T>),
          dim3((unsigned)pd.ctiles, (unsigned)pd.nchunks), dim3(MSBN_BLOCK), 0,
          stream, reinterpret_cast<const T*>(grad_y.data_ptr()),
          reinterpret_cast<const T*>(weight.data_ptr()),
          reinterpret_cast<T*>(dx.data_ptr()), (int)pd.h, (int)pd.w, (int)pd.c,
          (int)pd.oh, (int)pd.ow, pd.tile_h, pd.tile_w,
          (int)d5_cdiv(pd.h, pd.tile_h), (int)d5_cdiv(pd.w, pd.tile_w),
          (int)pd.items, (int)pd.chunk_items, pd.lpr);
      d5_check_launch("dgrad launch");
    }
    if (want_dw) {
      auto partial = pw.stride == 1 ? dwconv5x5_wgrad_partial_nhwc<T, 1>
                                    : dwconv5x5_wgrad_partial_nhwc<T, 2>;
      hipLaunchKernelGGL(
          partial, dim3((unsigned)pw.nchunks, (unsigned)pw.ctiles),
          dim3(MSBN_BLOCK), 0, stream,
          reinterpret_cast<const T*>(input.data_ptr()),
          reinterpret_cast<const T*>(grad_y.data_ptr()), ws.data_ptr<double>(),
          (int)pw.h, (int)pw.w, (int)pw.c, (int)pw.oh, (int)pw.ow, pw.tile_h,
          pw.tile_w, (int)d5_cdiv(pw.oh, pw.tile_h),
          (int)d5_cdiv(pw.ow, pw.tile_w), (int)pw.items, (int)pw.chunk_items,
          pw.lpr, pw.nchunks);
      d5_check_launch("wgrad partial launch");
      const int64_t total = pw.c * kD5Taps;
      hipLaunchKernelGGL((dwconv5x5_wgrad_finalize<T>),
                         dim3((unsigned)d5_cdiv(total, MSBN_BLOCK / MSBN_WAVE)),
                         dim3(MSBN_BLOCK), 0, stream, ws.data_ptr<double>(),
                         reinterpret_cast<T*>(dw.data_ptr()), total,
                         pw.nchunks);
      d5_check_launch("wgrad finalize launch");
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
