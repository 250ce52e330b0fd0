// Host-side API of the msbn gfx950 BatchNorm kernel set (bn_kernels.hip).
// Semantics: SURVEY.md §2.3 (the five stock SyncBatchNorm ATen ops), re-designed
// for MI355X (two-stage deterministic fp64 reductions sized for 256 CUs,
// NCHW + channels-last layouts, packed stat buffers for single-collective sync).
#pragma once

#include <ATen/ATen.h>

#include <map>
#include <string>
#include <tuple>
#include <vector>

namespace msbn {

// (mean, invstd) fp32 [C]; invstd = 1/sqrt(biased_var + eps).
std::tuple<at::Tensor, at::Tensor> batch_norm_stats(const at::Tensor& input,
                                                    double eps);

// Fused: write [mean(C) | invstd(C) | count(1)] into `out` (fp32, 2C+1).
void batch_norm_stats_packed(const at::Tensor& input, double eps,
                             at::Tensor& out);

// Combine per-rank stats; counts-weighted Chan merge; in-place running update.
std::tuple<at::Tensor, at::Tensor> batch_norm_gather_stats_with_counts(
    const at::Tensor& mean_all, const at::Tensor& invstd_all,
    const c10::optional<at::Tensor>& running_mean,
    const c10::optional<at::Tensor>& running_var, double momentum, double eps,
    const at::Tensor& counts);

// Packed variant: packed_all is [W, 2C+1]; returns (mean, invstd, count_sum[1]).
// Zero-count ranks masked in-kernel (no GPU->CPU sync; hipGraph-safe).
std::tuple<at::Tensor, at::Tensor, at::Tensor> batch_norm_gather_stats_packed(
    const at::Tensor& packed_all, const c10::optional<at::Tensor>& running_mean,
    const c10::optional<at::Tensor>& running_var, double momentum, double eps);

// As above but ALSO emits the per-channel [scale | shift] coefs (one launch).
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_gather_stats_packed_coefs(
    const at::Tensor& packed_all, const c10::optional<at::Tensor>& running_mean,
    const c10::optional<at::Tensor>& running_var, double momentum, double eps,
    const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, bool want_coefs);

// Fused local (world_size==1) stats: running-stats update + coefs emitted by
// the finalize kernel -> (mean, invstd, count_sum[1], coefs-or-undefined).
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_stats_local(const at::Tensor& input, double eps,
                       const c10::optional<at::Tensor>& running_mean,
                       const c10::optional<at::Tensor>& running_var,
                       double momentum,
                       const c10::optional<at::Tensor>& weight,
                       const c10::optional<at::Tensor>& bias, bool want_coefs);

// y = (x - mean) * invstd * weight + bias (scale/shift precomputed per channel).
at::Tensor batch_norm_elemt(const at::Tensor& input,
                            const c10::optional<at::Tensor>& weight,
                            const c10::optional<at::Tensor>& bias,
                            const at::Tensor& mean, const at::Tensor& invstd,
                            double eps);

// (sum_dy, sum_dy_xmu, grad_weight, grad_bias); sum_dy / sum_dy_xmu are views
// into ONE contiguous [2C] fp32 buffer so the cross-rank all_reduce is a single
// message (S6) with no cat() kernel.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_backward_reduce(const at::Tensor& grad_out, const at::Tensor& input,
                           const at::Tensor& mean, const at::Tensor& invstd,
                           const c10::optional<at::Tensor>& weight, bool input_g,
                           bool weight_g, bool bias_g);

// grad_input; `count` is a device tensor: [1] fp32 total count, or [W]
// per-rank counts (any int/float dtype) which are summed on device.
at::Tensor batch_norm_backward_elemt(
    const at::Tensor& grad_out, const at::Tensor& input, const at::Tensor& mean,
    const at::Tensor& invstd, const c10::optional<at::Tensor>& weight,
    const at::Tensor& sum_dy, const at::Tensor& sum_dy_xmu,
    const at::Tensor& count);

// ---- fused BN(+residual add)(+ReLU) epilogue path -------------------------
// Forward: y = relu?(x*scale + shift [+ residual]).  Backward recomputes the
// ReLU gate in-kernel from (x, scale, shift[, residual]) — no mask tensor and
// no separate clamp/add/threshold_backward kernels or their full-tensor
// round trips.
// coefs = packed [scale(C) | shift(C)] fp32 (bn_make_coefs); pass it to the
// act ops to avoid recomputing the per-channel affine in each of them.
// negative_slope generalises the activation to LeakyReLU: forward
// z>0 ? z : slope*z, gate z>0 ? dy : slope*dy.  It is only consulted when
// the relu / relu_mask flag is set, and 0.0 runs the plain ReLU kernels.
// act (trailing, "" by default) names an activation the pair cannot: "silu"
// is y = z*sigmoid(z), backward g = dy*s*(1 + z*(1 - s)) with s = sigmoid(z)
// recomputed from z like the gate.  It needs the flag set and a zero slope,
// has no gate bits, and exists in the two-stage and frozen ops only.
at::Tensor bn_make_coefs(const at::Tensor& mean, const at::Tensor& invstd,
                         const c10::optional<at::Tensor>& weight,
                         const c10::optional<at::Tensor>& bias);

// gate_out: uint8[ceil(numel/8)], bit (e & 7) of byte (e >> 3) = "the
// activation passes the gradient at storage offset e" (gate bits,
// docs/KERNEL_DESIGN.md).  The kernels store them only for an activated
// layer with a residual that runs at 8 elements per thread (bf16 / half,
// C or S a multiple of 8, 16-byte aligned tensors); the returned flag says
// whether they did.  y does not depend on gate_out.
std::tuple<at::Tensor, bool> batch_norm_elemt_act(
    const at::Tensor& input, const c10::optional<at::Tensor>& residual,
    const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, const at::Tensor& mean,
    const at::Tensor& invstd, bool relu,
    const c10::optional<at::Tensor>& coefs_in, double negative_slope,
    const c10::optional<at::Tensor>& gate_out, const std::string& act = "");

// grad_out2: second gradient of a forked output (residual block: conv1 and
// the skip path), delivered unsummed.  The kernel uses
// round_T(grad_out + grad_out2) as the incoming gradient — bit for bit the
// tensor an eager add would have stored — without that add's pass over
// memory.  Requires gm_out (the second pass then reads gm alone).
// gate: the bits batch_norm_elemt_act stored for this layer, given INSTEAD
// of its residual: the gate is taken from them, at any pack width.  Requires
// relu_mask, gm_out and a bf16 / half input.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_backward_reduce_act(
    const at::Tensor& grad_out, const at::Tensor& input,
    const c10::optional<at::Tensor>& residual, const at::Tensor& mean,
    const at::Tensor& invstd, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, bool relu_mask, bool input_g,
    bool weight_g, bool bias_g, const c10::optional<at::Tensor>& coefs_in,
    const c10::optional<at::Tensor>& gm_out, double negative_slope,
    const c10::optional<at::Tensor>& grad_out2,
    const c10::optional<at::Tensor>& gate, const std::string& act = "");

// ---- frozen path (normalize with running stats, autograd on) --------------
// One launch: (running_mean, running_var, eps, weight?, bias?) -> packed fp32
// [scale(C) | shift(C)], the buffer batch_norm_elemt_act(coefs_in=) consumes.
at::Tensor bn_frozen_coefs(const at::Tensor& running_mean,
                           const at::Tensor& running_var, double eps,
                           const c10::optional<at::Tensor>& weight,
                           const c10::optional<at::Tensor>& bias);

// dx = scale[c]*g, dres = g with g = grad_out * 1[z > 0], or for a non-zero
// negative_slope g = z > 0 ? grad_out : negative_slope*grad_out (gate
// recomputed from input/residual when relu_mask; input is not touched
// otherwise).
// Returns (dx-or-undefined, dres-or-undefined); without the gate dres is
// grad_out itself.
std::tuple<at::Tensor, at::Tensor> batch_norm_frozen_backward_elemt(
    const at::Tensor& grad_out, const c10::optional<at::Tensor>& input,
    const c10::optional<at::Tensor>& residual, const at::Tensor& coefs,
    bool relu_mask, bool want_input_grad, bool want_res_grad,
    double negative_slope, const std::string& act = "");

// ---- small-plane world-1 fused path (single launch fwd / bwd) -------------
// Stock K10-style block-per-channel kernels gated to small NCHW planes
// (GAN / small-per-GPU-batch regime): one kernel does stats + running
// update + normalize(+res)(+relu); one kernel does the whole backward.
bool bn_fused_local_eligible(const at::Tensor& input,
                             const c10::optional<at::Tensor>& weight,
                             const c10::optional<at::Tensor>& bias,
                             const c10::optional<at::Tensor>& running_mean,
                             const c10::optional<at::Tensor>& running_var);

// returns (y, mean, invstd, count[1], coefs[2C])
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_fwd_fused_local(const at::Tensor& input,
                           const c10::optional<at::Tensor>& residual,
                           const c10::optional<at::Tensor>& weight,
                           const c10::optional<at::Tensor>& bias, double eps,
                           double momentum,
                           const c10::optional<at::Tensor>& running_mean,
                           const c10::optional<at::Tensor>& running_var,
                           bool relu, double negative_slope);

// returns (dx, grad_weight?, grad_bias?, dres?)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_bwd_fused_local(const at::Tensor& grad_out, const at::Tensor& input,
                           const c10::optional<at::Tensor>& residual,
                           const at::Tensor& mean, const at::Tensor& invstd,
                           const c10::optional<at::Tensor>& weight,
                           const c10::optional<at::Tensor>& coefs,
                           bool relu_mask, bool want_res_grad, bool weight_g,
                           bool bias_g, double negative_slope);

// returns (grad_input, grad_residual-or-undefined)
std::tuple<at::Tensor, at::Tensor> batch_norm_backward_elemt_act(
    const at::Tensor& grad_out, const at::Tensor& input,
    const c10::optional<at::Tensor>& residual, const at::Tensor& mean,
    const at::Tensor& invstd, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, const at::Tensor& sum_dy,
    const at::Tensor& sum_dy_xmu, const at::Tensor& count, bool relu_mask,
    bool want_res_grad, const c10::optional<at::Tensor>& coefs_in,
    double negative_slope, const std::string& act = "");

// ---- stem pool fusion: bn + act + MaxPool2d(3, 2, 1) -----------------------
// Channels-last 4-D input only; the pool geometry is fixed (kernel 3,
// stride 2, padding 1, dilation 1, floor mode: OH = (H-1)/2 + 1).  The
// forward returns (pooled, codes): pooled = maxpool(act(x*scale + shift))
// with the maximum taken over the values rounded to the input dtype, and one
// uint8 window code kh*3 + kw per pooled element (first maximum in kh, kw
// order, NaN wins), both channels-last [N, C, OH, OW].  The activation
// tensor itself is never stored.  The backward ops take the POOLED
// gradient(s) and the codes in the place of batch_norm_backward_*_act's
// grad_out: each x element's gradient is gathered from the windows that
// chose it (fp32 sum in ascending window order, rounded to the input dtype
// once -- the tensor the pool's own backward would have stored).  grad_out2
// is the second gradient of a forked pooled output, as in
// batch_norm_backward_reduce_act.  Results are bit-identical to the unfused
// composition.
std::tuple<at::Tensor, at::Tensor> batch_norm_elemt_act_pool(
    const at::Tensor& input, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, const at::Tensor& mean,
    const at::Tensor& invstd, bool relu,
    const c10::optional<at::Tensor>& coefs_in, double negative_slope);

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_backward_reduce_act_pool(
    const at::Tensor& grad_out, const c10::optional<at::Tensor>& grad_out2,
    const at::Tensor& codes, const at::Tensor& input, const at::Tensor& mean,
    const at::Tensor& invstd, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, bool relu_mask, bool input_g,
    bool weight_g, bool bias_g, const c10::optional<at::Tensor>& coefs_in,
    double negative_slope);

at::Tensor batch_norm_backward_elemt_act_pool(
    const at::Tensor& grad_out, const c10::optional<at::Tensor>& grad_out2,
    const at::Tensor& codes, const at::Tensor& input, const at::Tensor& mean,
    const at::Tensor& invstd, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, const at::Tensor& sum_dy,
    const at::Tensor& sum_dy_xmu, const at::Tensor& count, bool relu_mask,
    const c10::optional<at::Tensor>& coefs_in, double negative_slope);

// ---- in-place activated path (forward over x, backward from y) ------------
// The forward writes y = act(x*scale + shift) over `input` and returns it;
// the backward ops take that stored y instead of x and invert the activation
// (identity, or LeakyReLU with negative_slope > 0: `act` with any other slope
// is an error) and the affine map:  z = y > 0 ? y : y/slope,
// x - mean = (z - bias)/scale.  Needs weight*invstd != 0 in every channel; a
// zero gives finite but wrong gradients for that channel.  Two-stage kernels
// only (no small-plane variant).  sum_dy / sum_dy_xmu / grad_weight /
// grad_bias mean what batch_norm_backward_reduce_act returns.
at::Tensor batch_norm_elemt_act_(at::Tensor& input,
                                 const c10::optional<at::Tensor>& weight,
                                 const c10::optional<at::Tensor>& bias,
                                 const at::Tensor& mean,
                                 const at::Tensor& invstd, bool act,
                                 const c10::optional<at::Tensor>& coefs_in,
                                 double negative_slope);

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_backward_reduce_inplace(
    const at::Tensor& grad_out, const at::Tensor& output,
    const at::Tensor& invstd, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, bool act, bool input_g,
    bool weight_g, bool bias_g, const c10::optional<at::Tensor>& coefs_in,
    double negative_slope);

at::Tensor batch_norm_backward_elemt_inplace(
    const at::Tensor& grad_out, const at::Tensor& output,
    const at::Tensor& mean, const at::Tensor& invstd,
    const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, const at::Tensor& sum_dy,
    const at::Tensor& sum_dy_xmu, const at::Tensor& count, bool act,
    const c10::optional<at::Tensor>& coefs_in, double negative_slope);

// ---- dual BN: relu(bn(x) + bn_d(x_d)) in three kernels ---------------------
// The first block of a ResNet stage normalises its skip path too.  These ops
// run the pair of layers with one forward kernel, one backward reduce and one
// backward elemt kernel: the skip BN's output is never stored and gm is read
// once per pass for both layers.  Dense channels-last 4-D bf16 / half, C a
// multiple of 8, 16-byte aligned tensors, plain ReLU, gate bits.  Results are
// bit-identical to batch_norm_elemt + batch_norm_elemt_act(residual,
// gate_out) / the gated reduce + batch_norm_backward_reduce on gm / two
// batch_norm_backward_elemt calls.
//
// coefs / coefs2: packed [scale | shift] of the main / skip layer.  Returns
// (y, stored); stored == false means the kernel declined: y is undefined and
// nothing was written (gate_out included).
std::tuple<at::Tensor, bool> batch_norm_elemt_act_dual(
    const at::Tensor& input, const at::Tensor& input2, const at::Tensor& coefs,
    const at::Tensor& coefs2, bool relu, double negative_slope,
    const at::Tensor& gate_out);

// (sums, grad_weight, grad_bias, grad_weight2, grad_bias2); sums is ONE
// contiguous fp32 [4C] buffer [sum_dy | sum_dy_xmu | sum_dy_2 | sum_dy_xmu_2]
// (a single all_reduce for the pair).  gm_out receives the gated gradient.
// Inputs the dual kernel declines run the two single reduces instead.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_backward_reduce_act_dual(
    const at::Tensor& grad_out, const at::Tensor& input,
    const at::Tensor& input2, const at::Tensor& mean, const at::Tensor& mean2,
    const at::Tensor& invstd, const at::Tensor& invstd2,
    const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& weight2, bool weight_g, bool bias_g,
    bool weight2_g, bool bias2_g, const at::Tensor& gm_out,
    const c10::optional<at::Tensor>& grad_out2, const at::Tensor& gate);

// (dx, dx2) from one read of gm; sums is the [4C] buffer above.
std::tuple<at::Tensor, at::Tensor> batch_norm_backward_elemt_dual(
    const at::Tensor& gm, const at::Tensor& input, const at::Tensor& input2,
    const at::Tensor& mean, const at::Tensor& mean2, const at::Tensor& invstd,
    const at::Tensor& invstd2, const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& weight2, const at::Tensor& sums,
    const at::Tensor& count);

// ---- 1x1 conv + statistics (conv_stats_kernels.hip) ------------------------
// A 1x1, stride-1, unpadded, ungrouped, bias-free convolution of a dense
// channels-last 4-D bf16 / half input, run as one MFMA GEMM kernel that also
// forms the per-channel {sum y, sum y^2} of the output it stores (fp32
// accumulation, rounded to the input dtype once; the statistics are those of
// the rounded values).  Returns (y, partials, nchunks): y channels-last
// [N, Cout, H, W]; partials the fp64 workspace [Cout][nchunks][2] that the
// *_from_partials ops below finalize.
//
// Declines -- (undefined, undefined, 0), nothing launched -- for anything
// else: a CPU, fp32, empty or not dense channels-last input, a weight of
// another dtype / device / shape or not contiguous, Cin or Cout not a
// multiple of 8, a pointer off 16-byte alignment, and a Cin whose 32-column
// weight slab does not fit the LDS (Cin > 2304).
std::tuple<at::Tensor, at::Tensor, int64_t> conv1x1_stats(
    const at::Tensor& input, const at::Tensor& weight);

// The launch conv1x1_stats would make (device not considered); ok == false
// where it declines.
struct Conv1x1Plan {
  bool ok;
  int64_t rows, cin, cout;
  int row_tile;         // rows of a tile
  int slab;             // output channels of a block
  int nslabs;           // grid.x
  int nchunks;          // grid.y: row runs = partials per channel
  int tiles_per_block;  // most row tiles one block visits
  int k_trips;          // 128-element trips of the K loop
  size_t lds_bytes;
};
Conv1x1Plan conv1x1_plan(const at::Tensor& input, const at::Tensor& weight);

// ---- depthwise 3x3 conv + statistics (dwconv_stats_kernels.hip) ------------
// y[n, c, oh, ow] = sum_{kh, kw} x[n, c, oh*s - 1 + kh, ow*s - 1 + kw] *
// w[c, 0, kh, kw]: kernel 3x3, padding 1, dilation 1, stride s in {1, 2},
// groups == Cin == Cout, no bias, OH = (H - 1)/s + 1, OW = (W - 1)/s + 1.
// Products and sums in fp32, kh then kw ascending into one accumulator,
// rounded to the input dtype once; the statistics are those of the rounded
// values.  Returns (y, partials, nchunks) as conv1x1_stats does.
//
// Declines -- (undefined, undefined, 0), nothing launched -- for anything
// but a non-empty dense channels-last 4-D bf16 / half GPU input with a
// contiguous [C, 1, 3, 3] weight of the same dtype and device, C a multiple
// of 8, 16-byte aligned pointers and a stride of 1 or 2.
std::tuple<at::Tensor, at::Tensor, int64_t> dwconv3x3_stats(
    const at::Tensor& input, const at::Tensor& weight, int64_t stride);

// The launch dwconv3x3_stats would make (device not considered); ok == false
// where it declines.
struct DwConvPlan {
  bool ok;
  int64_t n, c, h, w, oh, ow;
  int stride;
  int v;                // channels of a lane
  int lpr;              // lanes across the channel axis
  int ctiles;           // grid.x
  int strip;            // output columns of a work item
  int64_t items;        // work items: N * OH * ceil(OW / strip)
  int64_t chunk_items;  // items of a chunk (block)
  int nchunks;          // grid.y = partials per channel
  int trips;            // most items one thread visits
  int flush_every;      // most fp32 terms between two flushes
};
DwConvPlan dwconv3x3_plan(const at::Tensor& input, const at::Tensor& weight,
                          int64_t stride);

// ---- depthwise 3x3 conv gradients (dwconv_grad_kernels.hip) ---------------
// Both gradients of the convolution above from grad_y [N, C, OH, OW]:
//   dx[n,c,ih,iw] = sum dy[n,c,oh,ow] * w[c,0,kh,kw] over the taps with
//                   ih = oh*s - 1 + kh, iw = ow*s - 1 + kw inside dy
//   dw[c,0,kh,kw] = sum over (n,oh,ow) dy[n,c,oh,ow] * x[n,c,oh*s-1+kh,
//                   ow*s-1+kw] inside x
// dx: fp32 products and sums, dy rows then dy columns ascending into one
// accumulator, rounded once, channels-last like x.  dw: at most
// MSBN_ACC_FLUSH fp32 terms per accumulator, then fp64 (a deterministic
// two-stage reduction, no atomics), rounded once, contiguous [C, 1, 3, 3].
// Returns (dx, dw), each undefined where not wanted.
//
// Declines -- (undefined, undefined), nothing launched -- for whatever
// dwconv3x3_stats declines and for a grad_y that is not a dense channels-last
// [N, C, OH, OW] of the input's dtype and device at a 16-byte aligned address.
std::tuple<at::Tensor, at::Tensor> dwconv3x3_backward(
    const at::Tensor& grad_y, const at::Tensor& input,
    const at::Tensor& weight, int64_t stride, bool want_dx, bool want_dw);

// The launches dwconv3x3_backward would make (device not considered), in
// DwConvPlan's terms.  dgrad: items = N * H * ceil(W / strip) dx strips,
// flush_every = 9 (the taps of an element).  wgrad: items = N * OH *
// ceil(OW / strip) dy strips, nchunks = partials per (channel, tap), and
// trips * strip <= flush_every = MSBN_ACC_FLUSH by construction.
DwConvPlan dwconv3x3_dgrad_plan(const at::Tensor& input,
                                const at::Tensor& weight,
                                const at::Tensor& grad_y, int64_t stride);
DwConvPlan dwconv3x3_wgrad_plan(const at::Tensor& input,
                                const at::Tensor& weight,
                                const at::Tensor& grad_y, int64_t stride);

// ---- depthwise 5x5 conv + statistics, gradients (dwconv5x5_kernels.hip) ----
// The 3x3 ops above at kernel 5x5, padding 2:
//   y[n,c,oh,ow]  = sum_{kh,kw} x[n,c,oh*s-2+kh,ow*s-2+kw] * w[c,0,kh,kw]
//   dx[n,c,ih,iw] = sum dy[n,c,oh,ow] * w[c,0,kh,kw] over the taps with
//                   ih = oh*s-2+kh, iw = ow*s-2+kw inside dy
//   dw[c,0,kh,kw] = sum over (n,oh,ow) dy[n,c,oh,ow] * x[n,c,oh*s-2+kh,
//                   ow*s-2+kw] inside x
// y: fp32, kh then kw ascending into one accumulator, rounded once; the
// statistics are those of the rounded values.  dx: fp32, dy rows then dy
// columns ascending, rounded once.  dw: at most MSBN_ACC_FLUSH fp32 terms
// per accumulator, then fp64 (deterministic, no atomics), rounded once,
// contiguous [C, 1, 5, 5].  Same returns and the same declines as the 3x3
// ops, the weight being a contiguous [C, 1, 5, 5].
std::tuple<at::Tensor, at::Tensor, int64_t> dwconv5x5_stats(
    const at::Tensor& input, const at::Tensor& weight, int64_t stride);
std::tuple<at::Tensor, at::Tensor> dwconv5x5_backward(
    const at::Tensor& grad_y, const at::Tensor& input,
    const at::Tensor& weight, int64_t stride, bool want_dx, bool want_dw);

// The launches these ops would make (device not considered); ok == false
// where they decline.  A work item is a tile of tile_h x tile_w pixels of one
// image (of y for the forward and wgrad, of dx for dgrad); a thread row owns
// strips of `strip` columns of it.  trips: tiles a block visits (forward,
// dgrad), or strips of one tile a wgrad thread visits, whose fp32
// accumulators move to fp64 after every tile: trips * strip <= flush_every.
struct DwConv5x5Plan {
  bool ok;
  int64_t n, c, h, w, oh, ow;
  int stride;
  int v;                // channels of a lane
  int lpr;              // lanes across the channel axis (8 or 16)
  int ctiles;           // channel tiles
  int tile_h, tile_w;   // pixels of a work item
  int strip;            // columns of a thread row's strip
  int64_t items;        // tiles
  int64_t chunk_items;  // tiles of a chunk (block)
  int nchunks;          // partials per channel (and tap)
  int trips;
  int flush_every;      // most fp32 terms between two flushes
  size_t lds_bytes;     // static LDS of a block
};
DwConv5x5Plan dwconv5x5_plan(const at::Tensor& input, const at::Tensor& weight,
                             int64_t stride);
DwConv5x5Plan dwconv5x5_dgrad_plan(const at::Tensor& input,
                                   const at::Tensor& weight,
                                   const at::Tensor& grad_y, int64_t stride);
DwConv5x5Plan dwconv5x5_wgrad_plan(const at::Tensor& input,
                                   const at::Tensor& weight,
                                   const at::Tensor& grad_y, int64_t stride);

// batch_norm_stats_local / batch_norm_stats_packed with the partial stage
// already done: they run bn_stats_finalize alone over `partials`
// (fp64 [C][nchunks][2] of {sum x, sum x^2}, `count` elements per channel)
// and give their siblings' outputs, running-stat update and coefs.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_stats_local_from_partials(
    const at::Tensor& partials, int64_t nchunks, int64_t count, double eps,
    const c10::optional<at::Tensor>& running_mean,
    const c10::optional<at::Tensor>& running_var, double momentum,
    const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias, bool want_coefs);

void batch_norm_stats_packed_from_partials(const at::Tensor& partials,
                                           int64_t nchunks, int64_t count,
                                           double eps, at::Tensor& out);

// ---- grouped BN (grouped_bn_kernels.hip) -----------------------------------
// One training BatchNorm applied to S tensors ("segments": the levels of a
// feature pyramid under a shared head), each normalised with its own batch
// statistics, at a launch count that does not depend on S
// (docs/KERNEL_DESIGN.md "Grouped BN").  Served: 1 <= S <= 8 dense
// channels-last 4-D GPU tensors of one dtype (fp32 / bf16 / half) and one C,
// C a multiple of the 16-byte pack (8, or 4 for fp32), 16-byte aligned
// pointers, fp32 (or absent) weight / bias / running statistics.  Everything
// else is an error here: callers ask launch_plan first.  A segment may be
// empty; a group whose segments are all empty launches nothing.
//
// (mean[S,C], invstd[S,C], count[S], coefs[S,2C] = per segment
// [scale | shift]); the running statistics receive S successive momentum
// updates in segment order, each with that segment's unbiased variance.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_stats_local_grouped(const std::vector<at::Tensor>& inputs,
                               double eps,
                               const c10::optional<at::Tensor>& running_mean,
                               const c10::optional<at::Tensor>& running_var,
                               double momentum,
                               const c10::optional<at::Tensor>& weight,
                               const c10::optional<at::Tensor>& bias);

// out: fp32 [S, 2C+1], per segment [mean | invstd | count]: the message of
// ONE all_gather for the group.
void batch_norm_stats_packed_grouped(const std::vector<at::Tensor>& inputs,
                                     double eps, at::Tensor& out);

// packed_all: [W, S, 2C+1].  Count-weighted combine per segment (zero-count
// ranks masked in-kernel), the sequential running update, the coefs.
// Returns what batch_norm_stats_local_grouped returns.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
batch_norm_gather_stats_packed_grouped(
    const at::Tensor& packed_all, const c10::optional<at::Tensor>& running_mean,
    const c10::optional<at::Tensor>& running_var, double momentum, double eps,
    const c10::optional<at::Tensor>& weight,
    const c10::optional<at::Tensor>& bias);

// y_s = act(scale_s * x_s + shift_s), act = ReLU or none; the outputs are
// views of one allocation.
std::vector<at::Tensor> batch_norm_elemt_act_grouped(
    const std::vector<at::Tensor>& inputs, const at::Tensor& coefs, bool relu);

// (sums[S,2C] = per segment [sum_dy | sum_dy_xmu], grad_weight[C],
// grad_bias[C]); the ReLU gate is recomputed from x and coefs.  grad_weight
// / grad_bias are summed over the segments in ascending order (undefined
// where not asked for).
std::tuple<at::Tensor, at::Tensor, at::Tensor>
batch_norm_backward_reduce_act_grouped(
    const std::vector<at::Tensor>& grad_outs,
    const std::vector<at::Tensor>& inputs, const at::Tensor& mean,
    const at::Tensor& invstd, const at::Tensor& coefs, bool relu,
    bool weight_g, bool bias_g);

// dx_s from sums[s] (after the group's one all_reduce) and count[s].
std::vector<at::Tensor> batch_norm_backward_elemt_act_grouped(
    const std::vector<at::Tensor>& grad_outs,
    const std::vector<at::Tensor>& inputs, const at::Tensor& mean,
    const at::Tensor& invstd, const at::Tensor& coefs, const at::Tensor& sums,
    const at::Tensor& count, bool relu);

// launch_plan for the kinds "stats_grouped", "elemt_grouped",
// "bwd_reduce_grouped" and "bwd_elemt_grouped".
std::tuple<std::string, std::map<std::string, int64_t>> launch_plan_grouped(
    const std::string& kind, const at::Tensor& input,
    const std::vector<c10::optional<at::Tensor>>& others);

// ---- squeeze-excite after BN+SiLU (se_kernels.hip) -------------------------
// For y a dense channels-last bf16 / half [N, C, H, W] (the depthwise conv
// output), coefs = [scale(C) | shift(C)] fp32 of the training BatchNorm:
//   z = scale*y + shift, a = silu(z) (fp32, never stored)
//   s[n,c] = mean_hw a, h = silu(W1 s + b1), g = sigmoid(W2 h + b2)
//   out = a * g[n,c], rounded once
// docs/KERNEL_DESIGN.md "Squeeze-excite".  Every fp32 table below is
// contiguous; reductions are deterministic (no atomics).
//
// The streaming ops decline -- an undefined tensor, nothing launched -- for
// whatever se_plan declines (and a grad_out that is not y's twin); the small
// ops (gate, gate backward, BN finalize, parameter gradients) decline with a
// tuple of four undefined tensors for anything but what their comments name.

// How the streaming kernels tile y; ok == false where they decline: anything
// but a non-empty dense channels-last 4-D bf16 / half tensor with C a
// multiple of 8 at a 16-byte aligned address and N <= 65535.
struct SePlan {
  bool ok;
  int64_t n, c, hw;
  int v;                 // channels of a lane
  int lpr;               // lanes across the channel axis
  int ctiles;            // channel tiles
  int chunk_rows;        // pixels of a chunk (a multiple of 256 / lpr)
  int chunks_per_image;  // blocks (and partials) per image and channel tile
  int trips;             // pixels one thread visits
  int flush_every;       // most fp32 terms between two flushes
};
SePlan se_plan(const at::Tensor& y);

// C and Cr within the gate kernels' LDS tables
bool se_gate_fits(int64_t C, int64_t Cr);

// Partials fp64 [N, chunks, C, 3].  Without grad_out: {S = sum a, Q1 = sum
// silu'(z), Q2 = sum silu'(z)(y - mean)} per image and channel; with
// grad_out (y's twin): {R = sum dout a, P1 = sum dout silu'(z), P2 = sum dout
// silu'(z)(y - mean)}.
at::Tensor se_squeeze(const at::Tensor& y, const at::Tensor& coefs,
                      const at::Tensor& mean,
                      const c10::optional<at::Tensor>& grad_out);

// (s[N,C], hpre[N,Cr], g[N,C], Q[N,C,2]) from the forward partials of images
// of hw pixels.  w1 [Cr, C(, 1, 1)], b1 [Cr], w2 [C, Cr(, 1, 1)], b2 [C]:
// contiguous, one dtype (fp32 / bf16 / half); C <= 4096, 1 <= Cr <= 1024.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> se_gate(
    const at::Tensor& partials, int64_t hw, const at::Tensor& w1,
    const at::Tensor& b1, const at::Tensor& w2, const at::Tensor& b2);

at::Tensor se_scale(const at::Tensor& y, const at::Tensor& coefs,
                    const at::Tensor& g);

// (dpool[N,C], dz2[N,C], dz1[N,Cr], P[N,C,2]) from the backward partials:
// dz2 = R g (1 - g), dz1 = (W2^T dz2) silu'(hpre), dpool = W1^T dz1 / hw.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> se_gate_backward(
    const at::Tensor& partials, int64_t hw, const at::Tensor& g,
    const at::Tensor& hpre, const at::Tensor& w1, const at::Tensor& w2);

// (sum_dy, sum_dy_xmu, grad_weight, grad_bias) of the BatchNorm, the two sums
// views of one fp32 [2C] buffer:
//   sum_dy = sum_n g*P1 + dpool*Q1, sum_dy_xmu = sum_n g*P2 + dpool*Q2 (fp64)
//   grad_weight = sum_dy_xmu * invstd, grad_bias = sum_dy (fp32, or undefined)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
se_bn_finalize_backward(const at::Tensor& g, const at::Tensor& dpool,
                        const at::Tensor& p, const at::Tensor& q,
                        const at::Tensor& invstd, bool weight_g, bool bias_g);

// (dW1, db1, dW2, db2) of the SE block in the weights' dtype, each undefined
// where not wanted: dW2 = dz2^T silu(hpre), db2 = sum_n dz2, dW1 = dz1^T s,
// db1 = sum_n dz1; fp64 over n ascending, rounded once.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> se_param_backward(
    const at::Tensor& dz2, const at::Tensor& dz1, const at::Tensor& hpre,
    const at::Tensor& s, const at::Tensor& w1, const at::Tensor& w2,
    bool want_w1, bool want_b1, bool want_w2, bool want_b2);

// dy = A*gz + B*y + D with gz = (grad_out*g + dpool) * silu'(z) and the
// coefficients of batch_norm_backward_elemt (fp32 weight or none); sum_dy /
// sum_dy_xmu are the sums over all ranks, count a 1-element fp32 tensor.
at::Tensor se_backward_elemt(const at::Tensor& grad_out, const at::Tensor& y,
                             const at::Tensor& coefs, const at::Tensor& g,
                             const at::Tensor& dpool, const at::Tensor& mean,
                             const at::Tensor& invstd,
                             const c10::optional<at::Tensor>& weight,
                             const at::Tensor& sum_dy,
                             const at::Tensor& sum_dy_xmu,
                             const at::Tensor& count);

// launch_plan for the kinds "se_squeeze", "se_scale" (input = y),
// "se_bwd_reduce", "se_bwd_elemt" (others = {grad_out}): path "se"; and
// "se_gate", "se_gate_bwd" (input = y, others = {w1, w2}): path "se_gate"
// with Cr and lds_bytes.  All report V, lpr, ctiles, chunk_rows,
// chunks_per_image, trips, flush_every and finalize_trips (the trips of the
// per-channel sum over the images), or "ineligible".
std::tuple<std::string, std::map<std::string, int64_t>> launch_plan_se(
    const std::string& kind, const at::Tensor& input,
    const std::vector<c10::optional<at::Tensor>>& others);

// ---- launch plan (host only, launches nothing) ----------------------------
// Which kernel path a call would take and how far its loops run, decided by
// the same host code the ops launch with.  kind / tensors:
//   "stats"            input = x
//   "bwd_reduce"       input = x,        others = {grad_out, residual, gm_out,
//                                              grad_out2}
//   "elemt"            input = x,        others = {residual},  coefs
//   "bwd_elemt"        input = x,        others = {grad_out, residual}, coefs
//   "frozen_bwd_elemt" input = grad_out, others = {x, residual}, coefs
//   "fused_local"      input = x,        others = {residual}
//   "elemt_inplace"      input = x,      coefs
//   "bwd_reduce_inplace" input = y,      others = {grad_out}
//   "bwd_elemt_inplace"  input = y,      others = {grad_out}
//   "elemt_pool"         input = x,      others = {pooled, codes}, coefs
//   "bwd_reduce_pool"    input = x,      others = {grad_out, grad_out2, codes}
//   "bwd_elemt_pool"     input = x,      others = {grad_out, grad_out2, codes},
//                                        coefs
//   "elemt_dual"         input = x,      others = {x2[, coefs2]}, coefs
//   "bwd_reduce_dual"    input = x,      others = {grad_out, x2, gm_out,
//                                                  grad_out2, gate}
//   "bwd_elemt_dual"     input = x,      others = {gm, x2}
//   "conv1x1_stats"      input = x,      others = {weight}: path "mfma" with
//                        nchunks, row_tile, slab, nslabs, tiles_per_block,
//                        k_trips and lds_bytes, or "ineligible"
//   "dwconv3x3_stats" (stride 1) / "dwconv3x3s2_stats" (stride 2)
//                        input = x,      others = {weight}: path "dwconv" with
//                        V, lpr, ctiles, strip, items, chunk_items, nchunks,
//                        trips, flush_every and finalize_trips, or
//                        "ineligible"
//   "dwconv3x3_dgrad" / "dwconv3x3_wgrad" (stride 1), "dwconv3x3s2_dgrad" /
//   "dwconv3x3s2_wgrad" (stride 2)
//                        input = x,      others = {weight, grad_y}: path
//                        "dwconv" with the same numbers (finalize_trips for
//                        wgrad alone), or "ineligible"
//   "dwconv5x5_stats" / "dwconv5x5_dgrad" / "dwconv5x5_wgrad" (stride 1),
//   "dwconv5x5s2_stats" / "dwconv5x5s2_dgrad" / "dwconv5x5s2_wgrad" (stride 2)
//                        the same tensors as their 3x3 namesakes: path
//                        "dwconv" with DwConv5x5Plan's numbers (V, lpr, ctiles,
//                        tile_h, tile_w, strip, items, chunk_items, nchunks,
//                        trips, flush_every, lds_bytes; finalize_trips for
//                        stats and wgrad), or "ineligible"
//   "stats_grouped" / "elemt_grouped"          input = x_0, others = {x_1 ..
//                        x_{S-1}}; "bwd_reduce_grouped" / "bwd_elemt_grouped"
//                        others = {x_1 .. x_{S-1}, dy_0 .. dy_{S-1}}: path
//                        "nhwc" or "ineligible" (launch_plan_grouped)
//   "se_squeeze" / "se_scale" / "se_bwd_reduce" / "se_bwd_elemt" / "se_gate" /
//   "se_gate_bwd"        launch_plan_se
// (pass only what the op itself would dereference).  Returns (path, numbers):
// path is "nchw_vec" | "nchw_flat" | "nhwc" | "small_plane" | "ineligible";
// the dual kinds report "nhwc" with their single counterparts' numbers plus
// dual = 1, or "ineligible" for inputs the dual kernels decline;
// numbers always hold V and trips (most loop iterations of one thread);
// reductions add nchunks, flush_every, finalize_trips and the chunk sizes,
// elementwise ops add grid, packs and multi_trip.
std::tuple<std::string, std::map<std::string, int64_t>> launch_plan(
    const std::string& kind, const at::Tensor& input,
    const std::vector<c10::optional<at::Tensor>>& others,
    const c10::optional<at::Tensor>& coefs);

}  // namespace msbn
