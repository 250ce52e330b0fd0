// 1x1 stride-1 convolution that also emits the following BatchNorm's
// statistics (gfx950, CDNA4).  docs/KERNEL_DESIGN.md "Conv + statistics".
//
// Channels-last, such a convolution is the GEMM  Y[M, Cout] = X[M, Cin] .
// W[Cout, Cin]^T  with M = N*H*W and both operands contiguous along K.  At
// BatchNorm shapes it is memory-bound, so the kernel is built to stream X in
// and Y out once and to form the per-channel {sum y, sum y^2} from the
// accumulator registers on the way: the statistics pass over Y
// (bn_stats_partial_nhwc) never runs.
//
//  * grid (column slabs, row runs), slab index fastest: the blocks that read
//    one X tile are neighbours.  A block owns a slab of BN = 32*NB output
//    channels and a contiguous run of 128-row tiles.
//  * the block's W slab is loaded once (cached loads) into LDS, zero-padded
//    to whole k-trips and whole slabs, and stays there for the run.
//  * each of the 4 waves owns 32 rows of a tile.  X goes from HBM straight
//    into the MFMA A-operand registers with 16-byte nontemporal loads, one
//    k-trip (128 elements) ahead of the matrix instructions that consume it
//    (two register buffers).  v_mfma_f32_32x32x16: lane (j = lane % 32,
//    g = lane / 32) supplies row j, k = 16*s + 8*g .. +7 of step s; the B
//    operand is the same k range of slab column j, one ds_read_b128.
//  * epilogue per tile: the fp32 accumulators are rounded to T once; the
//    statistics are taken over those rounded values, shifted by a pivot (the
//    wave's first row of the tile) and un-shifted in fp64 per lane; the
//    rounded tile goes through a per-wave LDS stage so that Y leaves in
//    16-byte nontemporal stores.
//  * at the end of the run the fp64 sums of the two lane groups of the four
//    waves are added through LDS in a fixed order and the block writes one
//    {sum y, sum y^2} pair per channel: ws[C][nchunks][2], the workspace
//    bn_stats_finalize consumes.  No atomics.
#include "bn_ops.hpp"
#include "common.hpp"

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>

// Scalar fp32 arithmetic only in this file's device code: the epilogue's
// independent per-row adds and multiplies are what the vectorizer turns
// into packed fp32 instructions.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace msbn {

namespace {

constexpr int kCsRows = 128;      // rows of a tile: 4 waves x 32
constexpr int kCsWaveRows = 32;   // the MFMA's M
constexpr int kCsKTrip = 128;     // K elements per trip: 8 MFMA steps of 16
constexpr int kCsSteps = kCsKTrip / 16;
constexpr int kCsPad = 16;        // bytes added to every LDS row (bank spread)
constexpr int kCsLdsBytes = 160 * 1024;  // LDS of one CU
constexpr int kCsTargetBlocks = 2048;    // as the BN reductions' kTargetBlocks

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename T>
struct Mfma;
template <>
struct Mfma<__hip_bfloat16> {
  using frag = bf16x8;
  static __device__ __forceinline__ f32x16 run(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Mfma<__half> {
  using frag = f16x8;
  static __device__ __forceinline__ f32x16 run(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

// 16 bytes of operand: a Pack in memory, an MFMA fragment in registers
template <typename T>
union Frag {
  Pack<T, 8> pk;
  typename Mfma<T>::frag f;
  int __attribute__((vector_size(16))) raw;
  __device__ __forceinline__ Frag() : raw{0, 0, 0, 0} {}
};

// The runtime header's __syncthreads and shuffles were declared before the
// attribute above and would be called, not inlined, from code that carries
// it: the block barrier is spelled out here, and the kernel exchanges lane
// values through LDS.
__device__ __forceinline__ void cs_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// LDS bytes of one W slab row / of one stage row
__host__ __device__ inline int cs_w_row_bytes(int ktrips) {
  return ktrips * kCsKTrip * 2 + kCsPad;
}
__host__ __device__ inline int cs_stage_row_bytes(int bn) {
  return bn * 2 + kCsPad;
}

// =====================================================================
// grid (nslabs, nchunks) block 256, dynamic LDS:
//   [BN rows of W, cs_w_row_bytes each][4 waves x 32 stage rows]
// ws layout: [Cout][nchunks][2] fp64, chunk = blockIdx.y
// =====================================================================
template <typename T, int NB>
__global__ __launch_bounds__(MSBN_BLOCK) void conv1x1_stats_nhwc(
    const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y,
    double* __restrict__ ws, int64_t M, int Cin, int Cout, int ktrips,
    int tiles_per_block, int nchunks) {
  constexpr int BN = NB * 32;
  constexpr int PPR = BN / 8;  // 16-byte packs per stage row
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & (MSBN_WAVE - 1);
  const int wave = tid >> 6;
  const int j = lane & 31;  // A row / B column / D column of this lane
  const int g = lane >> 5;  // k half of a step; D rows 4g..4g+3 of each 8
  const int col0 = blockIdx.x * BN;
  const int run = blockIdx.y;
  const int wrs = cs_w_row_bytes(ktrips);
  constexpr int srs = BN * 2 + kCsPad;
  unsigned char* wl = smem;
  unsigned char* stage_all = smem + BN * wrs;
  unsigned char* stage = stage_all + wave * kCsWaveRows * srs;

  // ---- W slab -> LDS, zero beyond Cin / Cout ----
  {
    const int ppr = ktrips * (kCsKTrip / 8);
    for (int idx = tid; idx < BN * ppr; idx += MSBN_BLOCK) {
      const int row = idx / ppr;
      const int k = (idx - row * ppr) * 8;
      const int col = col0 + row;
      Frag<T> v;
      if (col < Cout && k < Cin)
        v.pk = *reinterpret_cast<const Pack<T, 8>*>(w + (int64_t)col * Cin + k);
      *reinterpret_cast<Pack<T, 8>*>(wl + row * wrs + k * 2) = v.pk;
    }
  }

  const int64_t ntiles = (M + kCsRows - 1) / kCsRows;
  const int64_t t0 = (int64_t)run * tiles_per_block;
  const int64_t t1 = i64min(t0 + tiles_per_block, ntiles);

  // one k-trip of this lane's X row: 8 packs, 32 bytes apart
  auto load_trip = [&](Frag<T>(&buf)[kCsSteps], int64_t tile, int kt) {
    const int64_t row = tile * kCsRows + wave * kCsWaveRows + j;
    const int kb = kt * kCsKTrip + g * 8;
    const T* p = x + row * Cin + kb;
#pragma unroll
    for (int s = 0; s < kCsSteps; ++s) {
      Frag<T> v;
      if (row < M && kb + s * 16 < Cin) v.pk = nt_load<T, 8>(p + s * 16);
      buf[s] = v;
    }
  };

  Frag<T> a_cur[kCsSteps], a_nxt[kCsSteps];
  f32x16 acc[NB];
  double sum[NB], sumsq[NB];  // this lane's rows of one column, whole run
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) sum[nb] = sumsq[nb] = 0.0;

  int64_t tile = t0;
  int kt = 0;
  if (tile < t1) load_trip(a_cur, tile, 0);
  cs_sync();  // the W slab is in place

  while (tile < t1) {
    int nkt = kt + 1;
    int64_t ntile = tile;
    if (nkt == ktrips) {
      nkt = 0;
      ++ntile;
    }
    if (ntile < t1) load_trip(a_nxt, ntile, nkt);  // block-uniform

    if (kt == 0) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    }
    const int left = Cin - kt * kCsKTrip;  // > 0
    const int ksteps = left >= kCsKTrip ? kCsSteps : (left + 15) / 16;
    const unsigned char* wb = wl + j * wrs + (kt * kCsKTrip + g * 8) * 2;
#pragma unroll
    for (int s = 0; s < kCsSteps; ++s) {
      if (s < ksteps) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          Frag<T> b;
          b.pk = *reinterpret_cast<const Pack<T, 8>*>(wb + nb * 32 * wrs +
                                                      s * 32);
          acc[nb] = Mfma<T>::run(a_cur[s].f, b.f, acc[nb]);
        }
      }
    }

    if (kt == ktrips - 1) {
      // ---- epilogue of this tile ----
      const int64_t wrow0 = tile * kCsRows + wave * kCsWaveRows;
      const int64_t rem = M - wrow0;
      const int nvalid = rem >= kCsWaveRows ? kCsWaveRows : (rem > 0 ? (int)rem : 0);
      // D register r of lane (j, g): row 8*(r/4) + 4*g + r%4, column j.
      // Round once; the rounded tile goes to the wave's stage.
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int lrow = 8 * (r >> 2) + 4 * g + (r & 3);
          *reinterpret_cast<T*>(stage + lrow * srs + (nb * 32 + j) * 2) =
              from_f<T>(acc[nb][r]);
        }
      }
      cs_sync();
      if (nvalid > 0) {  // wave-uniform
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          // pivot: the stored value of the wave's first row of this column
          // (a valid row here), read back from the stage
          const float pivot =
              to_f(*reinterpret_cast<const T*>(stage + (nb * 32 + j) * 2));
          float fa = 0.f, fb = 0.f;
          int cnt = 0;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int lrow = 8 * (r >> 2) + 4 * g + (r & 3);
            if (lrow < nvalid) {
              const float d = to_f(from_f<T>(acc[nb][r])) - pivot;
              fa += d;
              fb += d * d;
              ++cnt;
            }
          }
          double da = (double)fa, db = (double)fb;
          unshift_pair(da, db, pivot, (double)cnt);
          sum[nb] += da;
          sumsq[nb] += db;
        }
      }
      // the wave's 32 x BN stage -> Y, 16 bytes per lane
#pragma unroll
      for (int it = 0; it < kCsWaveRows * PPR / MSBN_WAVE; ++it) {
        const int idx = it * MSBN_WAVE + lane;
        const int row = idx / PPR;
        const int pk = idx - row * PPR;
        const int c = col0 + pk * 8;
        if (row < nvalid && c < Cout) {
          nt_store<T, 8>(
              y + (wrow0 + row) * Cout + c,
              *reinterpret_cast<const Pack<T, 8>*>(stage + row * srs + pk * 16));
        }
      }
      cs_sync();  // stage free for the next tile / the final combine
    }

#pragma unroll
    for (int s = 0; s < kCsSteps; ++s) a_cur[s] = a_nxt[s];
    tile = ntile;
    kt = nkt;
  }

  // ---- run totals: the 8 (wave, lane group) sums of a column through LDS,
  // added in a fixed order ----
  double* red = reinterpret_cast<double*>(stage_all);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    red[((wave * 2 + g) * BN + nb * 32 + j) * 2] = sum[nb];
    red[((wave * 2 + g) * BN + nb * 32 + j) * 2 + 1] = sumsq[nb];
  }
  cs_sync();
  if (tid < BN && col0 + tid < Cout) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int part = 0; part < 2 * (MSBN_BLOCK / MSBN_WAVE); ++part) {
      a += red[(part * BN + tid) * 2];
      b += red[(part * BN + tid) * 2 + 1];
    }
    const int64_t o = ((int64_t)(col0 + tid) * nchunks + run) * 2;
    ws[o] = a;
    ws[o + 1] = b;
  }
}

size_t cs_lds_bytes(int bn, int ktrips) {
  return (size_t)bn * cs_w_row_bytes(ktrips) +
         (size_t)kCsRows * cs_stage_row_bytes(bn);
}

inline int64_t cs_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

template <typename T, int NB>
void cs_launch(const Conv1x1Plan& p, const at::Tensor& x, const at::Tensor& w,
               at::Tensor& y, at::Tensor& ws) {
  auto kern = conv1x1_stats_nhwc<T, NB>;
  // a long W row needs more dynamic LDS than a launch gets by default
  static bool raised = false;
  if (!raised && p.lds_bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern),
        hipFuncAttributeMaxDynamicSharedMemorySize, kCsLdsBytes);
    TORCH_CHECK(e == hipSuccess, "conv1x1_stats: LDS attribute: ",
                hipGetErrorString(e));
    raised = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)p.nslabs, (unsigned)p.nchunks),
                     dim3(MSBN_BLOCK), p.lds_bytes,
                     c10::hip::getCurrentHIPStream().stream(),
                     reinterpret_cast<const T*>(x.data_ptr()),
                     reinterpret_cast<const T*>(w.data_ptr()),
                     reinterpret_cast<T*>(y.data_ptr()), ws.data_ptr<double>(),
                     p.rows, (int)p.cin, (int)p.cout, p.k_trips,
                     p.tiles_per_block, p.nchunks);
  const hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "conv1x1_stats: launch: ", hipGetErrorString(e));
}

}  // namespace

Conv1x1Plan conv1x1_plan(const at::Tensor& input, const at::Tensor& weight) {
  Conv1x1Plan p{};
  if (!input.defined() || !weight.defined()) return p;
  if (input.dim() != 4 || weight.dim() != 4 || input.numel() == 0) return p;
  const auto dt = input.scalar_type();
  if (dt != at::kBFloat16 && dt != at::kHalf) return p;
  if (weight.scalar_type() != dt || weight.device() != input.device()) return p;
  if (!input.is_contiguous(at::MemoryFormat::ChannelsLast)) return p;
  if (weight.size(2) != 1 || weight.size(3) != 1 ||
      weight.size(1) != input.size(1) || !weight.is_contiguous())
    return p;
  const int64_t cin = input.size(1), cout = weight.size(0);
  if (cin == 0 || cout == 0 || cin % 8 != 0 || cout % 8 != 0) return p;
  if (cin > (1 << 20) || cout > (1 << 20)) return p;
  if ((uintptr_t)input.data_ptr() % 16 != 0 ||
      (uintptr_t)weight.data_ptr() % 16 != 0)
    return p;
  p.cin = cin;
  p.cout = cout;
  p.rows = input.numel() / cin;
  p.k_trips = (int)cs_cdiv(cin, kCsKTrip);
  // widest slab that Cout can use and whose W rows fit the LDS next to the
  // stage; a Cin too long for a 32-column slab is declined
  int bn = cout > 64 ? 128 : (cout > 32 ? 64 : 32);
  while (bn > 32 && cs_lds_bytes(bn, p.k_trips) > (size_t)kCsLdsBytes) bn /= 2;
  if (cs_lds_bytes(bn, p.k_trips) > (size_t)kCsLdsBytes) return p;
  p.slab = bn;
  p.lds_bytes = cs_lds_bytes(bn, p.k_trips);
  p.nslabs = (int)cs_cdiv(cout, bn);
  p.row_tile = kCsRows;
  const int64_t ntiles = cs_cdiv(p.rows, kCsRows);
  // row runs: as many blocks as the BN reductions aim for, shared out among
  // the slabs; every run has at least one tile
  const int64_t runs = std::min<int64_t>(
      ntiles, std::max<int64_t>(1, kCsTargetBlocks / p.nslabs));
  p.tiles_per_block = (int)cs_cdiv(ntiles, runs);
  p.nchunks = (int)cs_cdiv(ntiles, p.tiles_per_block);
  p.ok = true;
  return p;
}

std::tuple<at::Tensor, at::Tensor, int64_t> conv1x1_stats(
    const at::Tensor& input, const at::Tensor& weight) {
  if (!input.defined() || !input.is_cuda()) return {at::Tensor(), at::Tensor(), 0};
  const Conv1x1Plan p = conv1x1_plan(input, weight);
  if (!p.ok) return {at::Tensor(), at::Tensor(), 0};
  // allocator-aligned outputs
  at::Tensor y = at::empty(
      {input.size(0), p.cout, input.size(2), input.size(3)},
      input.options().memory_format(at::MemoryFormat::ChannelsLast));
  at::Tensor ws = at::empty({p.cout, (int64_t)p.nchunks, 2},
                            input.options().dtype(at::kDouble));
  auto go = [&](auto tag) {
    using T = decltype(tag);
    switch (p.slab) {
      case 128:
        cs_launch<T, 4>(p, input, weight, y, ws);
        break;
      case 64:
        cs_launch<T, 2>(p, input, weight, y, ws);
        break;
      default:
        cs_launch<T, 1>(p, input, weight, y, ws);
    }
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
