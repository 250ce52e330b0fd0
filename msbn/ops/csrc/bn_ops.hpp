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
    const c10::optional<at::Tensor>& gate_out);

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
    const c10::optional<at::Tensor>& gate);

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
    double negative_slope);

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
    double negative_slope);

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
