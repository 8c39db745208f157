/*
 * libganinpaint — C-ABI of the MI355X (gfx950) backend for the GAN-inpainting hot path.
 *
 * The reference (abeytheo/gan-inpainting) is pure Python and has NO FFI of its own; the
 * interfaces this library stands behind are the Python ones cited next to each group below
 * (paths are relative to the upstream repository). INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every entry point returns 0 on success, a negative gi_status otherwise; the message of the
 *     last error on the calling thread is returned by gi_last_error(); nothing throws.
 *   - all pointers are DEVICE pointers unless the name ends in _host; the caller owns every
 *     buffer (it hands device memory to the handle with the *_bind calls, sizes come from the
 *     matching *_bytes / *_count queries); the handle owns no device memory.
 *   - calls are asynchronous on the hipStream_t given to gi_ctx_create (passed as void*);
 *     a handle is bound to one device and one stream and is not thread-safe.
 *   - public image tensors are fp32 (N,1,H,W) contiguous (NCHW == NHWC for one channel).
 *   - conv / transposed-conv weights are fp32 in physical order [a][ky][kx][b] where
 *     a = Conv2d out-channels (resp. ConvTranspose2d in-channels) and b the other channel
 *     axis, i.e. the torch "channels_last" image of the reference's [a,b,4,4] tensors
 *     (lib/models/networks.py:285, :293-309, :337-352), so state_dict() values are zero-copy.
 */
#ifndef GANINPAINT_H
#define GANINPAINT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  GI_OK = 0,
  GI_ERR_INVALID = -1,      /* bad argument / unsupported shape */
  GI_ERR_HIP = -2,          /* a HIP runtime call or kernel launch failed */
  GI_ERR_STATE = -3,        /* call order violated (e.g. backward without forward) */
  GI_ERR_UNSUPPORTED = -4
} gi_status;

typedef enum { GI_F32 = 0, GI_F16 = 1 } gi_dtype;      /* internal compute/storage type */
typedef enum { GI_ACT_NONE = 0, GI_ACT_RELU = 1, GI_ACT_LRELU = 2 } gi_act;

typedef struct gi_ctx gi_ctx;
typedef struct gi_net gi_net;

const char* gi_last_error(void);
int gi_version(void);

/* ---- run-time options (process-wide): which kernel family serves a layer. Every shape is served under every setting
 * (the alternatives are the fallbacks for shapes the default kernels do not take, e.g. tensors beyond 2^31 bytes); results
 * agree to rounding (tests/test_options_gpu.py runs each). value < 0 restores the default, which is the environment
 * variable of the same name if set (read once), else the number in brackets. Nothing here exists in the reference.
 *   GI_IGEMM5 [7]         bit 0 / 1 / 2: halo-resident implicit GEMM for sub-pixel phases / 4x4-s2 gather / 3x3-s1 (else igemm3)
 *   GI_IGEMM6 [1]         0: first-generation halo kernels (igemm5) instead of the buffer-descriptor LDS-DMA ones (igemm6 AND igemm8)
 *   GI_IGEMM8 [1]         0: never the four-wave / two-workgroups-per-CU halo kernel (igemm8); 1: on layers with >= 512
 *                         workgroups; 2: on every eligible layer
 *   GI_IGEMM7 [1]         0: small-M layers on the generic kernel (igemm.hip) instead of the four-stage ring kernel
 *   GI_IGEMM_FIXUP [1]    0: split-K partial sums added by a finish launch instead of the last arriver inside the GEMM
 *   GI_IGEMM_VARIANT [3]  1: fp16 layers on the register-staged generic kernel only
 *   GI_BN_ACC [1]         0: BatchNorm statistics through partial rows + finalize launches (read at net creation)
 *   GI_FUSE_HEAD [1]      0: last norm + activation in front of a network's head as a separate pass (read at net creation)
 *   GI_HEAD_FAST [1]      0: PatchGAN head on the generic kernels
 *   GI_BN_BWD_FUSE [1]    0: BatchNorm-backward reduction as its own launch instead of the producing GEMM's epilogue
 *   GI_BN_BWD_SMALL [512] largest pixel count served by the one-launch BatchNorm backward (0: never)
 *   GI_WGRAD2 [1]         0: weight gradients on the register-staged kernel (wgrad.hip) only
 *   GI_WGRAD3 [1]         0: the unpipelined two-tap-row weight-gradient kernel instead of wgrad3
 *   GI_BN_FOLD [0]        1: the BatchNorm + activation (+ dropout) pass of the generator's small layers inside the GEMM that produces
 *                         the layer (igemm7's last finisher per channel column) instead of as its own launch; bit-identical results.
 *                         Off by default: measured SLOWER (+8 .. 10 us per folded layer at the headline shape)
 *   GI_C1_FUSED [1]       0: the single-channel transposed convolution (generator u1, d1's input gradient) as two launches through a
 *                         col tensor in memory instead of one launch with the col rows in LDS; bit-identical results
 *   GI_WGRAD_STREAM [1]   0: the weight-gradient GEMMs of gi_net_backward[_phase] on the context's stream, in line with the
 *                         input-gradient chain, instead of on the network's second HIP stream beside it (the entry joins the two
 *                         before it returns; same kernels, same operands, same results)
 *   GI_MASK_BITS [1]      0: the LeakyReLU backward of the first layer, fused into the second layer's input-gradient GEMM, reads the
 *                         layer's fp16 activation (128 bytes per pixel) instead of the 64-bit sign word per pixel the forward wrote
 *                         beside it, and applies the slope to the fp16-rounded gradient instead of the fp32 accumulator
 *   GI_C1W_FUSE [1]       0: the weight gradient of the first (single-channel) layer as its own launch reading the gradient at the
 *                         layer's output from memory, instead of from the tiles of the second layer's input-gradient GEMM while they
 *                         are in LDS (that gradient is then not stored at all unless the network's input gradient is asked for).
 *                         Needs GI_MASK_BITS = 1
 *   GI_IGEMM7_WAVES [8]   4: the small-M ring kernel (igemm7) as four-wave workgroups (one wave per SIMD, 64 x BN/2 wave tiles)
 *                         instead of eight-wave ones (two per SIMD); sums agree to fp32 rounding */
int gi_set_option(const char* name, int value);
int gi_get_option(const char* name, int* value);
/* name of the GEMM / weight-gradient kernel family and instantiation launched most recently by this process, e.g.
 * "igemm6<1,128,relu>", "igemm7<0,64>", "wgrad3<4>" (tests assert which kernel served a shape); "" before the first. */
const char* gi_debug_last_kernel(void);
/* number of GEMM launches of this process that normalised their own output (GI_BN_FOLD; tests count folded layers with it) */
int gi_debug_fold_count(void);

/* ---- context ------------------------------------------------------------------------------ */
int gi_ctx_create(int device_id, void* hip_stream, gi_ctx** out);
int gi_ctx_destroy(gi_ctx* ctx);
int gi_ctx_sync(gi_ctx* ctx);

/* ---- networks: lib/models/networks.py:13-28 get_network, :216-253 UnetGenerator,
 *      :331-363 PatchGANDiscriminator ------------------------------------------------------- */
/* UnetGenerator(in_c=1,out_c=1,num_downs,ngf,BatchNorm2d,use_dropout truthy): dropout_p is 0.5
 * for the reference's get_network (networks.py:18-19), 0 disables it. n_slots = number of
 * independent activation sets (forward calls that may be live before their backward). */
int gi_unet_create(gi_ctx* ctx, int num_downs, int ngf, float dropout_p, int H, int W, int max_n,
                   int dtype, int n_slots, gi_net** out);
/* UnetGenerator(1, out_c, ...) with out_c in 1..64 output channels (the frozen face-parsing network
 * UnetGenerator(1,4,7,ngf=32), train.py:171-172; Tanh head as in networks.py:293-298). out_c > 1 nets
 * are forward + input-gradient only (gi_net_backward with need_param_grads = 0, also after an eval-mode
 * forward: running-statistics BatchNorm). y / dy are (n,out_c,H,W). ngf must be a multiple of 64 for a
 * bound handle; an inventory-only handle (ctx NULL) accepts multiples of 8 (Python embeds ngf=32 in 64). */
int gi_unet_create_ex(gi_ctx* ctx, int num_downs, int ngf, int out_c, float dropout_p, int H, int W,
                      int max_n, int dtype, int n_slots, gi_net** out);
/* The same with the generator's norm layer chosen as get_norm_layer does (lib/models/networks.py:29-45):
 * norm_kind 0 = BatchNorm2d(affine, running statistics) - gi_unet_create_ex -, 1 = InstanceNorm2d(affine=False,
 * track_running_stats=False): statistics per image and channel in train AND eval mode, and every convolution carries a
 * bias (use_bias, networks.py:270-273; inventory names "<conv>.bias"), 2 = none (Identity). Kinds 1 and 2 run on the
 * unfused building blocks (no inference folding, no fused head). */
int gi_unet_create_norm(gi_ctx* ctx, int num_downs, int ngf, int out_c, int norm_kind, float dropout_p, int H,
                        int W, int max_n, int dtype, int n_slots, gi_net** out);
/* The same with level 1 (the outermost block's ngf channels) computed ch1 channels wide, ch1 a multiple of 64 >= ngf
 * (0: ngf): the inventory then reports [ch1, 1, 4, 4], [2 ngf, ch1, 4, 4], ... for the tensors that touch level 1; a
 * caller holding a narrower network (UnetGenerator(1, 4, 7, ngf=32), train.py:171-172) zero-fills the extra rows /
 * columns - zero channels stay zero through BatchNorm (beta 0) and the activations -, every other level runs at its
 * true width. */
int gi_unet_create_padded(gi_ctx* ctx, int num_downs, int ngf, int ch1, int out_c, int norm_kind, float dropout_p,
                          int H, int W, int max_n, int dtype, int n_slots, gi_net** out);
/* PatchGANDiscriminator(c=1, sigmoid): Linear(25,1) generalised to ((H/16-3)*(W/16-3),1). */
int gi_patchgan_create(gi_ctx* ctx, int H, int W, int sigmoid, int max_n, int dtype, int n_slots,
                       gi_net** out);
/* The same critic with SPECTRAL NORMALISATION (spectral_norm != 0; 0 is gi_patchgan_create) of the five convolution weights and
 * the Linear weight, with the semantics of torch.nn.utils.spectral_norm (eps 1e-12). Each weight, viewed as the ca x K matrix
 * W = weight.view(ca, -1), keeps persistent vectors u (ca) and v (K, torch's column order). A train-mode forward runs
 * n_power_iterations (>= 1) times v = W^T u / max(|W^T u|, eps), u = W v / max(|W v|, eps) in place, an eval-mode forward none;
 * both then use W / sigma, sigma = u . (W v). The backward treats u, v as constants and differentiates sigma through W:
 * dL/dW = (G - <G, W/sigma>_F u v^T) / sigma, G the gradient with respect to W / sigma. BatchNorm parameters and the Linear
 * bias are not normalised. Inventory: the six weights are named "<layer>.weight_orig", and "<layer>.weight_u" / ".weight_v"
 * are kind-4 buffers behind the running statistics. All of it is fp32 whatever the compute type.
 * One forward call is one power iteration round, so a stacked [real | fake] forward (gi_net_set_bn_groups 2) runs one where two
 * separate calls run two; gi_patchgan_gradient_penalty runs one more for its own primal forward. Every backward (and the
 * penalty) uses the u, v, sigma of ITS forward, kept per slot. CONTRACT: the caller does not write the parameters between a
 * forward and its backward (as for the packed copies). gi_net_sync_weights on such a handle only marks the derived copies
 * stale: every forward re-derives them. Without spectral norm nothing is allocated, launched or named differently. */
int gi_patchgan_create_sn(gi_ctx* ctx, int H, int W, int sigmoid, int spectral_norm, int n_power_iterations, int max_n,
                          int dtype, int n_slots, gi_net** out);
/* Parity tests: the six sigma (model.0, 2, 5, 8, 11, 13) of the forward held in `slot` (0 .. n_slots - 1, or n_slots: the last
 * gradient penalty's own forward) to sigma6, and the effective parameters in the workspace - the flat parameter buffer with
 * the six weights divided by sigma, count = gi_net_param_floats() - to eff_params; fails when those belong to another forward
 * than the slot's. Device pointers, either may be NULL. Asynchronous on the context's stream. */
int gi_net_sn_read(gi_net* net, int slot, float* sigma6, float* eff_params, int64_t count);
/* DCGANDiscriminator() (reference lib/models/networks.py:162-212; get_network('discriminator', 'dcgan'), :23-24):
 * 4 x [Conv2d 5x5 s1 p1 + bias, ReLU, MaxPool 2/2], Linear 36864 -> 4096 -> 512 -> 2 (ReLU between), Softmax over the
 * two logits, view(-1, 1): y is (2n, 1), row 2i + j = p_j of image i. H = W = 128 only (Linear 12's 36864 = 1024*6*6
 * inputs). Conv weights are kind 0 of shape [a,b,5,5] (physical [a][ky][kx][b]), the Linears kind 1; no buffers. The
 * generic gi_net_* entries apply; gi_net_set_bn_groups is accepted and has no effect (no BatchNorm), set_train /
 * set_inference change nothing (train and eval forwards are the same). Backward phases: 1 = softmax .. Linear 12 (range
 * [gi_net_phase_split(), end)), 2 = the convolutions. gi_net_saved_activation kinds: 0 = pooled map of conv `level`
 * (1..4, (n,C,h,w)); 1 = its pool decisions, sub-position (dy*2+dx) of the window's maximum + 4 if that pre-activation
 * was > 0; 2 = level 1 ReLU(Linear 12) (n,4096), level 2 ReLU(Linear 14) (n,512), level 3 the probabilities (n,2).
 * The convolutions' pre-activations are not kept: the forward stores only the pooled maps, and the decision byte already
 * holds every choice the backward makes there (which window element wins and whether it passes the ReLU). A parity test
 * measures the ambiguity bands on the reference's own pre-activations and imposes these decisions inside them. */
int gi_dcgan_create(gi_ctx* ctx, int H, int W, int max_n, int dtype, int n_slots, gi_net** out);
/* Debug (tests: which kernel serves the convolution forward): the four convolution blocks of a forward of n images into
 * `slot`, nothing after them; the slot then holds no forward that a backward could use. */
int gi_dcgan_debug_forward_convs(gi_net* net, int slot, const float* x, int n);
int gi_net_destroy(gi_net* net);

/* parameter / buffer inventory, in the reference's named_parameters() order, then buffers.
 * kind: 0 conv weight (shape [a,b,4,4], physical [a][ky][kx][b]), 1 bias / BN affine / Linear
 * (contiguous), 2 BN running_mean, 3 BN running_var, 4 plain buffer (spectral norm: weight_u, weight_v). offset is in
 * floats into the flat param (kind 0,1) or flat buffer (kind 2,3,4) allocation. */
int gi_net_tensor_count(gi_net* net);
int gi_net_tensor_desc(gi_net* net, int index, char* name, int name_cap, int* kind, int64_t* shape4,
                       int* ndim, int64_t* offset, int64_t* numel);
int64_t gi_net_param_floats(gi_net* net);      /* flat fp32 params (and grads, optimizer states) */
int64_t gi_net_buffer_floats(gi_net* net);     /* flat fp32 BN running stats */
int64_t gi_net_workspace_bytes(gi_net* net);   /* activations, packed weights, scratch */
int gi_net_bind(gi_net* net, float* params, float* grads, float* buffers, void* workspace,
                int64_t workspace_bytes);
/* re-derive the packed (fp16 / transposed) weight copies after params were written by the caller */
int gi_net_sync_weights(gi_net* net);
int gi_net_set_train(gi_net* net, int train);
/* Inference hint (generators): with train = 0, forwards will never be differentiated. BatchNorm layers are then folded
 * into the neighbouring convolutions (scale into a second weight copy, shift as the GEMM bias, activation in the
 * epilogue); gi_net_backward on such a forward fails. What eval.py:94 / evaluate.py:127-158 run under no_grad. */
int gi_net_set_inference(gi_net* net, int inference);
int gi_net_set_loss_scale(gi_net* net, float scale);
/* discriminator only: the next forward/backward batches hold `groups` (1 or 2) consecutive, equally sized image
 * groups with INDEPENDENT BatchNorm batch statistics (running statistics updated group by group). groups = 2 runs
 * the reference's two critic calls D(ground), D(inpainted) (wgan_l1.py:134-135) as one stacked batch. */
int gi_net_set_bn_groups(gi_net* net, int groups);   /* fp16 backward scaling, default 65536 */
int gi_net_set_dropout_seed(gi_net* net, uint64_t seed);   /* also resets the counter to 0 */
/* the dropout stream is (seed, counter): each train-mode forward that draws masks advances the counter by one.
 * Saved and restored by resumable training, so that a resumed run draws the masks of the uninterrupted one. */
int gi_net_get_dropout_state(gi_net* net, uint64_t* seed, uint64_t* counter);
int gi_net_set_dropout_state(gi_net* net, uint64_t seed, uint64_t counter);
/* keep-mask of dropout level `level` used by the last train-mode forward of `slot`,
 * as uint8 in (N,C,H,W) order (what the oracle consumes); count = N*C*H*W */
int gi_net_dropout_mask(gi_net* net, int slot, int level, uint8_t* out_nchw, int64_t count);
/* impose external keep-masks (uint8 NCHW, device) for the next forward of slot; null clears */
int gi_net_set_dropout_mask(gi_net* net, int slot, int level, const uint8_t* mask_nchw);

/* Activations the forward held in `slot` saved for its backward, as fp32 (N,C,h,w): which side of every ReLU / LeakyReLU
 * kink the forward took (parity tests hand these decisions to the oracle for units whose pre-activation is within fp32
 * rounding distance of zero). Generator, level k = 1..num_downs: kind 0 = the skip a_k = LeakyReLU(norm(conv_k(.)))
 * (networks.py:287; k = num_downs: ReLU of the innermost convolution, :299-305); kind 1 (k < num_downs) = the decoder half
 * ReLU(dropout(norm(up_{k+1}(.)))) concatenated beside it (:289, :324). Discriminator, kind 0, level i = 1..4:
 * LeakyReLU(BatchNorm(conv_i(.))) (:335-345). count = N*C*h*w. */
int gi_net_saved_activation(gi_net* net, int slot, int kind, int level, float* out_nchw, int64_t count);
/* Debug: number of split-K tile tickets of this network that are not zero between launches (must be 0: every launch leaves
 * them zero; anything else means a launch was cut short). Synchronises the stream. */
int gi_net_debug_nonzero_tickets(gi_net* net, int* count);

/* forward: x (n,1,H,W) fp32 -> y: generator (n,1,H,W) fp32, discriminator (n,1) fp32 */
int gi_net_forward(gi_net* net, int slot, const float* x, float* y, int n);
/* backward of the forward held in `slot`: dy like y; dx like x or NULL; need_wgrad=0 is the
 * frozen-net case of util.set_requires_grad(nets, False) (lib/models/util.py:19-22): only input
 * gradients are produced. Parameter gradients ACCUMULATE into the bound grads. */
int gi_net_backward(gi_net* net, int slot, const float* dy, float* dx, int need_wgrad);

/* backward in pieces so the host can overlap a gradient all-reduce with compute (phase 0 = everything).
 * Generator: phase 1 = decoder (its parameter gradients are the flat range [gi_net_phase_split(), end), complete
 * on return); phase 2 = encoder (range [0, split)), or split once more: phase 3 = innermost .. level 5 (range
 * [gi_net_phase_split2(), split): 12.6 of the encoder's 15.3 M gradients, finished first), phase 4 = levels 4 .. 1.
 * Discriminator: phase 1 = head + conv4 block (range [gi_net_phase_split(), end)), phase 2 = conv3 .. conv1. */
int gi_net_backward_phase(gi_net* net, int slot, const float* dy, float* dx, int need_wgrad, int phase);
int64_t gi_net_phase_split(gi_net* net);
int64_t gi_net_phase_split2(gi_net* net);

/* ---- data-parallel gradient exchange (NOT in the reference, which is single-device: train.py:44-46).
 * One process per GPU, replicated networks, per-rank minibatch; before every optimizer update the flat fp32 gradient
 * buffer of the network is SUM-all-reduced over RCCL (xGMI) and the optimizer divides by the world size (grad_scale).
 * The communicator is created from a 128-byte unique id (rank 0 draws it with gi_comm_unique_id, the host carries it to
 * the other ranks - e.g. torch.distributed.broadcast, MPI, a file). All calls are asynchronous on the given streams;
 * gi_net_allreduce_grads_async takes a range [begin, end) of the flat buffer (end < 0: to the end) so that ranges whose
 * gradients are final (gi_net_backward_phase / gi_net_phase_split) can be reduced while the backward still runs;
 * gi_allreduce_wait makes compute_stream wait for everything issued on comm_stream so far. librccl is loaded on
 * first use: GI_ERR_UNSUPPORTED when it is not installed. */
typedef struct gi_comm gi_comm;
int gi_comm_unique_id(char* id128_host);
int gi_comm_create(const char* id128_host, int rank, int world, int device_id, gi_comm** out);
int gi_comm_destroy(gi_comm* comm);
int gi_allreduce_sum_f32(gi_comm* comm, float* buf, int64_t count, void* hip_comm_stream);
int gi_net_allreduce_grads_async(gi_net* net, gi_comm* comm, int64_t begin, int64_t end, void* hip_comm_stream);
int gi_allreduce_wait(gi_comm* comm, void* hip_comm_stream, void* hip_compute_stream);

/* WGAN-GP EXTENSION (not in the reference, which clips weights: wgan_l1.py:151-153): accumulates the
 * parameter gradient of  lam * mean_n (||grad_x D(xhat)_n||_2 - 1)^2  into the bound grads and writes the
 * penalty to penalty_out[0] (device). xhat: (n,1,H,W) interpolates, e.g. from gi_interpolate.
 * fp16 or fp32 critics without sigmoid, train mode. Uses a private activation set (no user slot is touched).
 * Scaling: the tangent (Jacobian-vector) pass runs on v * s, v = d(penalty)/d(grad_x D), with ONE power of two
 * s = 2^k per call derived on the device so that max|v * s| lies in [1, 2) (s = 1 when v is zero, e.g. lam = 0);
 * the reverse passes are seeded with the network's loss scale (gi_net_set_loss_scale). Both are removed before the
 * gradients are added to the bound ones; an overflow leaves inf / NaN there for the fp16 overflow guard. No sync. */
int gi_patchgan_gradient_penalty(gi_net* net, const float* xhat, int n, float lam, float* penalty_out);
/* The activations of the last gi_patchgan_gradient_penalty's own primal forward (its private activation set), as
 * gi_net_saved_activation of a critic with kind 0: level 1..4, fp32 (N,C,h,w), count = N*C*h*w. Parity tests only. */
int gi_patchgan_gp_saved_activation(gi_net* net, int level, float* out_nchw, int64_t count);
/* out[n] = eps[n]*real[n] + (1-eps[n])*fake[n] */
int gi_interpolate(gi_ctx* ctx, const float* real, const float* fake, const float* eps, int n, int64_t hw, float* out);

/* ---- mask pipeline: experiment_list/minimaxgan_l1.py:113-122 ------------------------------ */
/* mask_c = ceil(mask) if (flags & 1) else mask ; if (flags & 2) mask_c = 1 - mask_c (is_flip_mask of
 * evaluate.py:130-132) ; masked = ground * (1 - mask_c) */
int gi_mask_apply(gi_ctx* ctx, const float* ground, const float* mask, float* mask_c, float* masked,
                  int64_t count, int flags);
/* inpainted = masked + gen * mask_c */
int gi_mask_composite(gi_ctx* ctx, const float* masked, const float* gen, const float* mask_c,
                      float* inpainted, int64_t count);
/* out = a * b (the composite backward d_gen = d_inpainted * mask_c, and mask*x products) */
int gi_mul(gi_ctx* ctx, const float* a, const float* b, float* out, int64_t count);
/* out = a + alpha * b (sums the adversarial and reconstruction gradients of g_loss, minimaxgan_l1.py:168) */
int gi_add(gi_ctx* ctx, const float* a, const float* b, float* out, int64_t count, float alpha);

/* ---- losses. Each writes the scalar loss to loss_out[0] (device) and, when grad_a != NULL, the
 *      gradient w.r.t. `a` multiplied by gscale. nn.L1Loss (minimaxgan_l1.py:62,166);
 *      RMSELoss sqrt(mse+1e-16) (lib/models/loss.py:11-19); LocalLoss (loss.py:24-47,
 *      kind 0 = L1, 1 = MSE, 2 = sqrt extension); scratch: >= 4096 floats ---------------------- */
int gi_loss_l1(gi_ctx* ctx, const float* a, const float* b, int64_t count, float* loss_out,
               float* grad_a, float gscale, float* scratch);
int gi_loss_rmse(gi_ctx* ctx, const float* a, const float* b, int64_t count, float eps, float* loss_out,
                 float* grad_a, float gscale, float* scratch);
int gi_loss_mse(gi_ctx* ctx, const float* a, const float* b, int64_t count, float* loss_out,
                float* grad_a, float gscale, float* scratch);
int gi_loss_local(gi_ctx* ctx, const float* yhat, const float* y, const float* mask, int64_t count,
                  int kind, float* loss_out, float* grad_yhat, float gscale, float* scratch);
/* adversarial scalar losses on (n,) predictions: kind 0 BCE vs constant target
 * (minimaxgan_l1.py:135,141,162), 1 MSE vs constant target (experiment1_global_local_D.py:162),
 * 2 mean (wgan_l1.py:137-143,177; gscale carries the +1/-1 of backward(one/mone)) */
int gi_loss_adv(gi_ctx* ctx, const float* pred, int n, int kind, float target, float* loss_out,
                float* grad_pred, float gscale);
/* the two calls of a batch on a stacked [a | b] prediction vector (2 * n_each values: D(ground) | D(inpainted),
 * wgan_l1.py:134-143) in ONE launch: the same arithmetic per half, each with its own target, loss slot and gradient sign */
int gi_loss_adv_pair(gi_ctx* ctx, const float* pred2, int n_each, int kind, float target_a, float target_b, float* loss_a,
                     float* loss_b, float* grad_pred2, float gscale_a, float gscale_b);

/* ---- optimizers over flat fp32 buffers: optim.Adam(lr=2e-4,betas=(.5,.999))
 *      (minimaxgan_l1.py:64-65), optim.RMSprop(lr=5e-5) + p.data.clamp_(-c,c)
 *      (wgan_l1.py:64-65,151-153; clamp<=0 disables) ---------------------------------------- */
int gi_adam_step(gi_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t count, float lr,
                 float beta1, float beta2, float eps, int step, float grad_scale);
int gi_rmsprop_step(gi_ctx* ctx, float* p, const float* g, float* sq, int64_t count, float lr,
                    float alpha, float eps, float clamp, float grad_scale);
int gi_clamp(gi_ctx* ctx, float* p, int64_t count, float lo, float hi);
/* fp16 overflow guard (backend addition; the reference trains in fp32): gi_check_finite scans a flat gradient
 * buffer; flag3 is 3 device ints {running count of bad updates, verdict of this scan (0/1), scratch}. The
 * *_guarded optimizer steps do nothing when guard[1] != 0 (pass the same flag3, or NULL for the plain step). */
int gi_check_finite(gi_ctx* ctx, const float* g, int64_t count, int* flag3);
/* the same in two steps, for ONE optimizer over several flat buffers (Adam over itertools.chain(D_local, D_global),
 * experiment1_global_local_D.py:123): scan every buffer into the same flag3, then finish once - all networks of the
 * update share one verdict (all skip or none) and the running count advances by one per skipped update. */
int gi_check_finite_scan(gi_ctx* ctx, const float* g, int64_t count, int* flag3);
int gi_check_finite_finish(gi_ctx* ctx, int* flag3);
int gi_adam_step_guarded(gi_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t count, float lr,
                         float beta1, float beta2, float eps, int step, float grad_scale, const int* guard);
/* skipped_seen >= 0: `step` counts every call since the start minus the skipped updates the host has already learned of
 * (skipped_seen of them, read back from guard[0] at its own cadence); the kernel subtracts the rest, guard[0] - skipped_seen,
 * before it forms the bias corrections, so a skipped update never advances them whenever the host polls. < 0: `step` as is. */
int gi_adam_step_guarded2(gi_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t count, float lr,
                          float beta1, float beta2, float eps, int step, int skipped_seen, float grad_scale, const int* guard);
int gi_rmsprop_step_guarded(gi_ctx* ctx, float* p, const float* g, float* sq, int64_t count, float lr,
                            float alpha, float eps, float clamp, float grad_scale, const int* guard);
/* Without the finish launch: flag4 is 4 device ints {running count, verdict of the latest update, scan word, scan word}. An update
 * scans its buffers into flag4[word] (word = 2 or 3, the other one than the previous update used) and passes the same word to the
 * *_scan optimizer steps, which take their verdict from it; the FIRST step of the update (finish = 1) also records it (flag4[1],
 * flag4[0]) and clears the other word for the next update. word = 0: the *_guarded behaviour (verdict from flag4[1]). */
int gi_check_finite_scan_word(gi_ctx* ctx, const float* g, int64_t count, int* flag4, int word);
int gi_adam_step_scan(gi_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t count, float lr, float beta1, float beta2,
                      float eps, int step, int skipped_seen, float grad_scale, int* guard, int word, int finish);
int gi_rmsprop_step_scan(gi_ctx* ctx, float* p, const float* g, float* sq, int64_t count, float lr, float alpha, float eps,
                         float clamp, float grad_scale, int* guard, int word, int finish);
/* exponential moving average of a flat parameter buffer, one launch on the context's stream (optim.EMA):
 *   om = 1.0f - decay (fp32, on the host); per element diff = p - ema (rounded to fp32), ema = fmaf(om, diff, ema).
 * 0 <= decay <= 1. guard (may be NULL): the flag4 of the optimizer that just updated p; when guard[1] != 0 - that update
 * was skipped - ema is left untouched. ema and p may start at any float offset (16-byte accesses where both allow them). */
int gi_ema_update(gi_ctx* ctx, float* ema, const float* p, int64_t count, float decay, const int* guard);
/* mean(|g|) of `nseg` segments [off[i], off[i]+len[i]) of g -> out[i]
 * (gradient-flow statistics, minimaxgan_l1.py:180-182); offsets/lengths are device int64 */
int gi_grad_absmean(gi_ctx* ctx, const float* g, const int64_t* seg_off, const int64_t* seg_len,
                    int nseg, float* out);

/* ---- SSIM metric. lib/pytorch_ssim/__init__.py:20-40 `_ssim`, :68-76 `ssim()`,
 *      called per batch at experiment1_global_local_D.py:209. img1/img2: (n,c,H,W) fp32 contiguous on
 *      the device; depthwise window_size^2 Gaussian (sigma 1.5, zero padding window_size/2; window_size
 *      odd, <= 31), C1 = 0.01^2, C2 = 0.03^2. per_sample (n floats, may be NULL) = size_average=False;
 *      mean_out (1 float, may be NULL) = size_average=True. window_host: the 1-D window as
 *      `window_size` HOST floats, or NULL for the reference's gaussian(window_size, 1.5). scratch:
 *      gi_ssim_scratch_floats(...) device floats, 8-byte aligned (returns -1 for unsupported sizes) -- */
int64_t gi_ssim_scratch_floats(int n, int c, int H, int W, int window_size);
int gi_ssim(gi_ctx* ctx, const float* img1, const float* img2, int n, int c, int H, int W, int window_size,
            const float* window_host, float* per_sample, float* mean_out, float* scratch);

/* ---- evaluation pass ------------------------------------------------------
 * lib/models/evaluate.py:127-158: per batch  out = gen*m + ground*(1-m)  (m = mask_c from
 * gi_mask_apply: ceil, optionally flipped) and
 *   rmse_global = sqrt(mean (ground-out)^2 + eps)      l1_global = mean |ground-out|
 *   rmse_local  = sqrt(sum (out*m-ground*m)^2 / count(m!=0) + eps)   l1_local = sum |out*m-ground*m| / count(m!=0)
 * acc (device, 5 floats, may be NULL): acc[0..3] += {rmse_global, l1_global, rmse_local, l1_local},
 * acc[4] += 1 (the reference divides its running sums by the number of batches, :160-165);
 * batch_out (4 floats, may be NULL) receives this batch's values; inpainted_out (count floats, may be
 * NULL) the composite. scratch: gi_eval_recon_scratch_floats(count) floats, 8-byte aligned. */
int64_t gi_eval_recon_scratch_floats(int64_t count);
int gi_eval_recon(gi_ctx* ctx, const float* ground, const float* gen, const float* mask_c, int64_t count, float eps,
                  float* inpainted_out, float* acc, float* batch_out, float* scratch);
/* lib/models/evaluate.py:179-224 calculate_segmentation_eval_metric: prediction = argmax over the
 * class axis of logits (n,num_classes,hw) fp32; for each u of unique_labels_host[nu] (HOST ints, nu<=16):
 * precision / recall / IoU per sample from the pixel counts (eps 1e-32), mean over the n samples.
 * per_class: nu*3 floats {precision, recall, iou}; across: 3 floats (mean over classes).
 * labels: (n,hw) int64. scratch_counts: n*16*3 ints. */
int gi_seg_metrics(gi_ctx* ctx, const int64_t* labels, const float* logits, int n, int num_classes, int64_t hw,
                   const int* unique_labels_host, int nu, float* per_class, float* across, int* scratch_counts);

/* ---- config-5 generator-loss extras ------------------------------------
 * tv_loss (lib/models/loss.py:138-151): tv_weight * (mean_h-diff^2 + mean_w-diff^2) over `planes` = n*c
 * planes of H x W fp32; grad (may be NULL) = d loss / d img * gscale. loss_out: 1 float.
 * scratch: >= 4096 floats, 8-byte aligned. */
int gi_loss_tv(gi_ctx* ctx, const float* img, int planes, int H, int W, float tv_weight, float* loss_out,
               float* grad, float gscale, float* scratch);
/* nn.CrossEntropyLoss(weight=w) on (n,num_classes,hw) fp32 logits and (n,hw) int64 labels
 * (wgan_perceptual_style_faceparsing.py:67-68,212-213): sum_p w[y_p] * nll_p / sum_p w[y_p]; labels equal
 * to ignore_index (torch default -100) carry no weight. class_weight_host: num_classes HOST floats or NULL
 * (ones). num_classes in {2,3,4,8,16}. loss_out: 2 floats {loss, sum of weights}; grad_logits may be NULL. */
int gi_loss_cross_entropy(gi_ctx* ctx, const float* logits, const int64_t* labels, int n, int num_classes,
                          int64_t hw, const float* class_weight_host, int ignore_index, float* loss_out,
                          float* grad_logits, float gscale, float* scratch);

/* VGG-19 features for perceptual_loss / style_loss / perceptual_and_style_loss (lib/models/loss.py:50-115)
 * and gram_matrix (:117-136): taps relu1_1, relu2_1, relu3_1, relu4_1, relu5_1 (features[1,6,11,20,29]) of
 * the grey image repeated over 3 channels (:54-55). The reference runs it under no_grad; the backward below is
 * opt-in and needs a workspace of its own.
 * params: fp32, torchvision layout, the 13 convolutions up to features.28 (gi_vgg19_tensor_desc gives
 * name "features.<i>.weight|bias", shape, offset); fp16 MFMA compute. max_pairs = largest n. */
typedef struct gi_vgg gi_vgg;
int gi_vgg19_create(gi_ctx* ctx, int H, int W, int max_pairs, gi_vgg** out);
void gi_vgg19_destroy(gi_vgg* v);
int64_t gi_vgg19_param_floats(const gi_vgg* v);
int64_t gi_vgg19_workspace_bytes(const gi_vgg* v);
int gi_vgg19_num_tensors(const gi_vgg* v);
int gi_vgg19_tensor_desc(const gi_vgg* v, int index, char* name, int name_cap, int* shape4, int64_t* offset);
int gi_vgg19_bind(gi_vgg* v, const float* params, void* ws, int64_t ws_bytes);   /* ws 256-byte aligned */
int gi_vgg19_sync_weights(gi_vgg* v);                                            /* after params change */
/* out2 = { weight_p * sum_taps mean((F_o-F_t)^2), weight_s * sum_taps mean((G_o-G_t)^2) }, G = F F^T/(HWC);
 * output/target: (n,1,H,W) fp32; per_tap10 (may be NULL): the 5 perceptual then the 5 style terms. */
int gi_vgg19_perceptual_style(gi_vgg* v, const float* output, const float* target, int n, float weight_p,
                              float weight_s, float* out2, float* per_tap10);
/* feature map of tap 0..4 as (n,C,h,w) fp32 (parity checks) */
int gi_vgg19_features(gi_vgg* v, const float* x, int n, int tap, float* out_nchw);
/* Opt-in backward of the two terms w.r.t. `output` (target is a constant; the reference never back-propagates them).
 * It keeps the forward's feature maps in a separate workspace: query, bind after gi_vgg19_bind (256-byte aligned), then
 * gi_vgg19_sync_weights. A handle that never binds it allocates and runs exactly as without these entries; every entry
 * below fails with GI_ERR_INVALID on such a handle.
 * gi_vgg19_perceptual_style_grad: out2 / per_tap10 as gi_vgg19_perceptual_style (same kernels, same values);
 * grad_out: n*H*W floats = gscale * d(out2[0] + out2[1]) / d(output). fp16 with fp32 accumulation at a power-of-two scale
 * chosen on the device; bit-reproducible (no float atomics).
 * gi_vgg19_grad_layer (parity / debugging): the gradient w.r.t. the post-ReLU map of convolution `layer` (0..12) of the
 * last grad call as (n,C,h,w) fp32, gscale not applied; replays that call's backward from the workspace. */
int64_t gi_vgg19_grad_workspace_bytes(const gi_vgg* v);
int gi_vgg19_bind_grad(gi_vgg* v, void* ws, int64_t ws_bytes);
int gi_vgg19_perceptual_style_grad(gi_vgg* v, const float* output, const float* target, int n, float weight_p,
                                   float weight_s, float* out2, float* per_tap10, float* grad_out, float gscale);
int gi_vgg19_grad_layer(gi_vgg* v, int layer, float* out_nchw_f32);

/* LPIPS (Zhang et al. 2018; `lpips` v0.1 with net = 'vgg', normalize = True, spatial = False) between grey images repeated
 * over 3 channels: VGG-16 taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3, each before its max pool. The entries of this block are
 * the forward (the metric); the opt-in backward follows below.
 * H, W: multiples of 16, >= 16; 2 * max_pairs * H * W * 64 < 2^31. params (fp32, gi_lpips_tensor_desc gives name, shape, offset):
 * the 13 convolutions "features.<i>.weight|bias" (torchvision vgg16 indices 0,2,5,7,10,12,14,17,19,21,24,26,28), the five
 * "lin<k>.model.1.weight" vectors (64,128,256,512,512), "scaling_layer.shift" and "scaling_layer.scale" (3 each). The scaling
 * layer is folded into the first convolution at gi_lpips_sync_weights, exactly: the zero padding applies to the scaled input.
 * gi_lpips_distance: a, b (n,1,H,W) fp32 in [0,1], n <= max_pairs; out_n[i] = sum_l d_l[i],
 * d_l[i] = mean over pixels of sum_c lin_lc (fa / (|fa|_2 + 1e-10) - fb / (|fb|_2 + 1e-10))^2, norms over the channels of a pixel;
 * per_layer_5n (may be NULL): d_l[i] at [l * n + i]. fp16 MFMA convolutions, fp32 per pixel, fp64 spatial sums in a fixed order:
 * bit-reproducible, identical inputs give exactly 0, and the first layer and the tap kernels give an image the same bits wherever it
 * sits in the batch and whatever n is. Bit-equality ACROSS different n is not guaranteed through the twelve 3x3 convolutions: which
 * implicit-GEMM kernel serves a layer depends on its grid, which grows with n (calls with the same n always agree).
 * gi_lpips_features: the map of tap 0..4 as (n,C,h,w) fp32 (parity checks). */
typedef struct gi_lpips gi_lpips;
int gi_lpips_create(gi_ctx* ctx, int H, int W, int max_pairs, gi_lpips** out);
void gi_lpips_destroy(gi_lpips* v);
int64_t gi_lpips_param_floats(const gi_lpips* v);
int64_t gi_lpips_workspace_bytes(const gi_lpips* v);
int gi_lpips_num_tensors(const gi_lpips* v);
int gi_lpips_tensor_desc(const gi_lpips* v, int index, char* name, int name_cap, int* shape4, int64_t* offset);
int gi_lpips_bind(gi_lpips* v, const float* params, void* ws, int64_t ws_bytes);   /* ws 256-byte, params 16-byte aligned */
int gi_lpips_sync_weights(gi_lpips* v);                                            /* after params change */
int gi_lpips_distance(gi_lpips* v, const float* a, const float* b, int n, float* out_n, float* per_layer_5n);
int gi_lpips_features(gi_lpips* v, const float* x, int n, int tap, float* out_nchw);
/* Opt-in backward of the distance w.r.t. `a` (b is a constant). It keeps the forward's feature maps in a separate workspace: query,
 * bind after gi_lpips_bind (256-byte aligned), then gi_lpips_sync_weights. A handle that never binds it reports the same
 * gi_lpips_workspace_bytes and runs exactly as without these entries; every entry below fails with GI_ERR_INVALID on such a handle.
 * gi_lpips_distance_grad: out_n / per_layer_5n as gi_lpips_distance (same kernels, same bits); grad_a: n*H*W floats,
 * grad_a[i] = gscale * d out_n[i] / d a[i]. fp16 with fp32 accumulation at one power-of-two scale PER IMAGE, chosen on the device
 * from the image's largest seed and removed in fp32 by the last kernel; bit-reproducible (no float atomics); a[i] == b[i] gives an
 * exactly zero gradient. A pixel whose tap vector of `a` is all zero contributes no seed (autograd's 0 * inf there is NaN): the ReLU
 * mask below removes every channel of such a vector anyway.
 * gi_lpips_grad_tap (parity / debugging): the gradient w.r.t. the post-ReLU map of tap 0..4 of the last grad call as (n,C,h,w)
 * fp32, gscale not applied; replays that call's backward from the workspace. */
int64_t gi_lpips_grad_workspace_bytes(const gi_lpips* v);
int gi_lpips_bind_grad(gi_lpips* v, void* ws, int64_t ws_bytes);
int gi_lpips_distance_grad(gi_lpips* v, const float* a, const float* b, int n, float* out_n, float* per_layer_5n, float* grad_a,
                           float gscale);
int gi_lpips_grad_tap(gi_lpips* v, int tap, float* out_nchw_f32);

/* ---- Frechet Inception Distance (reference lib/fid/): Inception-V3 pool3 features + streaming statistics ----
 * The FID variant of Inception-V3 (lib/fid/inception.py: average pools that do not count padding in Mixed_5b..5d,
 * 6b..6e, 7b; a max pool in Mixed_7c), forward only, up to the 2048-wide global average (output block 3).
 * dtype GI_F16 / GI_F32 is the compute type (MFMA, fp32 accumulation). params: fp32, the published state
 * dict's layout per BasicConv2d: "<layer>.conv.weight" (O,I,kh,kw), "<layer>.bn.weight|bias|running_mean|
 * running_var" (gi_inception_tensor_desc: name, shape, float offset); BatchNorm (eps 0.001, running statistics)
 * is folded into weight and bias by gi_inception_sync_weights. ctx may be NULL for the inventory alone
 * (param_floats / num_tensors / tensor_desc / workspace_bytes); every other call on such a handle fails. */
typedef struct gi_inception gi_inception;
int gi_inception_create(gi_ctx* ctx, int dtype, int max_batch, gi_inception** out);
void gi_inception_destroy(gi_inception* v);
int64_t gi_inception_param_floats(const gi_inception* v);
int64_t gi_inception_workspace_bytes(const gi_inception* v);
int gi_inception_num_tensors(const gi_inception* v);
int gi_inception_tensor_desc(const gi_inception* v, int index, char* name, int name_cap, int* shape4, int64_t* offset);
int gi_inception_bind(gi_inception* v, const float* params, void* ws, int64_t ws_bytes);   /* ws 256-byte aligned */
int gi_inception_sync_weights(gi_inception* v);                                            /* after params change */
/* x: (n,c,H,W) fp32 in [0,1], c = 1 (replicated over 3 channels) or 3, any H, W: resized to 299x299 (bilinear,
 * align_corners = False) and mapped to 2x - 1 on the device. out: (n,2048) fp32. n <= max_batch. */
int gi_inception_features(gi_inception* v, const float* x, int n, int c, int H, int W, float* out);
/* runs the input kernel and the first nconvs convolutions (with the pools between them) only: tests read
 * gi_debug_last_kernel() to see which kernel served convolution nconvs - 1 */
int gi_inception_debug_forward_convs(gi_inception* v, const float* x, int n, int c, int H, int W, int nconvs);
/* Step-level test seam. The forward program has gi_inception_num_steps() = 107 steps in program order: 94
 * convolutions and 13 pools. step_desc: kind 0 convolution, 1 max pool 3x3 stride 2, 2 average pool 3x3 stride 1
 * padding 1 (padding not counted), 3 max pool 3x3 stride 1 padding 1; conv: the convolution's index (tensor_desc
 * index / 5) or -1; in_chw / out_chw: (C, H, W) of the step's input and output view (step 0 reads the resized
 * input with its 3 channels padded to 8); route4: {source buffer (-1: the resized input), destination buffer,
 * channels per destination row, channel offset of the output view in that row}. Works on a context-free handle.
 * debug_forward_steps: the input kernel and the first nsteps steps (0: the input kernel alone).
 * debug_read: fp32 NCHW copy (exact) of step's input view (which = 0), output view (1) or whole destination rows
 * (2: all route4[2] channels). Valid only directly after debug_forward_steps(..., nsteps = step + 1) on the same
 * n; anything else is refused on the host before any launch. */
int gi_inception_num_steps(const gi_inception* v);
int gi_inception_step_desc(const gi_inception* v, int step, int* kind, int* conv, int* in_chw, int* out_chw, int* route4);
int gi_inception_debug_forward_steps(gi_inception* v, const float* x, int n, int c, int H, int W, int nsteps);
int gi_inception_debug_read(gi_inception* v, int step, int which, int n, float* out_nchw_f32);
/* Streaming mean / covariance of d-wide fp32 feature rows in fp64 (lib/fid/fid_score.py:202-203 np.mean /
 * np.cov(rowvar=False)). acc: gi_fid_stats_acc_doubles(d) = 1 + d + d*d device doubles {count, sum, X^T X},
 * zeroed by the caller before the first update. Every element is accumulated row by row in arrival order, so
 * the result does not depend on how the rows were split into calls. finish: mu (d), sigma (d,d), divisor n-1. */
int64_t gi_fid_stats_acc_doubles(int d);
int gi_fid_stats_update(gi_ctx* ctx, double* acc, const float* feats, int n, int d);
int gi_fid_stats_finish(gi_ctx* ctx, const double* acc, double* mu, double* sigma, int d);

/* ---- distribution metrics on the pool3 features (csrc/featmetrics.hip): the sums of the Kernel Inception
 *      Distance and the k-NN manifolds of improved precision / recall ------------------------------------------------
 * All of it reduces a Gram matrix G[i][j] = sum_k A[ia[i]][k] * B[ib[j]][k] of fp32 feature rows (row stride d floats,
 * 1 <= d <= 8192) that is computed in fp64 (v_mfma_f64_16x16x4_f64, 64 x 64 tiles, K in ascending groups of four) and
 * never stored. An element's bits depend on its two feature rows only; every reduction has one fixed order; there
 * are no float atomics: results are the same bits run to run and do not depend on how a call was chunked.
 * Every pointer is device memory, index lists are int32. The entries TRUST the indices (0 <= index < rows of the
 * matrix): the caller checks them on the host (lib/fid/dist_metrics.py does). Asynchronous on the context's stream.
 * Workspace (8-byte aligned device memory, supplied by the caller), T(n) = ceil(n / 64):
 *   GI_FEAT_WS_KID      n = m, count = n_subsets:  8 * 3 * n_subsets * T(m)^2 bytes   one partial sum per tile
 *   GI_FEAT_WS_RADIUS   n, count = k:              8 * (n + n * T(n) * min(k, 64))    row norms + per-tile candidates
 *   GI_FEAT_WS_MEMBERS  n = na, n2 = nb:           8 * (na + nb)                      row norms
 * (-1 for arguments the entries would refuse). No n x n matrix is ever held. */
#define GI_FEAT_WS_KID 0
#define GI_FEAT_WS_RADIUS 1
#define GI_FEAT_WS_MEMBERS 2
int64_t gi_featmetrics_workspace_bytes(int op, int64_t n, int64_t n2, int count);
/* ix, iy: [n_subsets][m] rows of X / Y. sums[s] = { sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i,j} k(x_i, y_j) },
 * k(a, b) = (a.b / d + 1)^3 evaluated as t = G / (double)d + 1.0, t * t * t; the diagonal is skipped by position in the
 * list (a row drawn twice still pairs with its copy). One launch sequence for all subsets. m >= 2, n_subsets <= 21845. */
int gi_kid_subset_sums(gi_ctx* ctx, const float* X, const float* Y, const int* ix, const int* iy, int n_subsets, int m, int d,
                       void* ws, int64_t ws_bytes, double* sums);
/* radii[i] = the k-th smallest D_ij = max(0, |a_i|^2 + |a_j|^2 - 2 G_ij) over j != i (self excluded by index; duplicates of
 * a row count as neighbours at their computed distance). 1 <= k < n. */
int gi_feat_knn_radius(gi_ctx* ctx, const float* A, int n, int d, int k, void* ws, int64_t ws_bytes, double* radii);
/* member[j] = 1 when D(a_i, b_j) <= radii[i] for some row i of A, else 0 (nb bytes); *count (device) = how many are 1. */
int gi_feat_manifold_members(gi_ctx* ctx, const float* A, int na, const double* radii, const float* B, int nb, int d, void* ws,
                             int64_t ws_bytes, uint8_t* member, int* count);
/* test seam: the gathered Gram matrix itself, G (na, nb) fp64. ia / ib may be NULL (the identity). */
int gi_debug_feat_gram(gi_ctx* ctx, const float* A, const int* ia, int na, const float* B, const int* ib, int nb, int d, double* G);

/* ---- input transform: transforms.Resize(size) + ToTensor() of train.py:69-72 on decoded
 *      8-bit grey images (lib/data/dataset.py:6-12). Bit-exact restatement of Pillow's antialiased bilinear
 *      resampler (22-bit fixed point, horizontal pass first, uint8 intermediate), then /255. ------------- */
int gi_resize_output_size(int in_h, int in_w, int size, int* out_h, int* out_w);   /* Resize(int): smaller edge */
int64_t gi_resize_table_bytes(int in_h, int in_w, int out_h, int out_w);
/* host-computed coefficient tables -> tables_dev (device, gi_resize_table_bytes); once per geometry; synchronises */
int gi_resize_build_tables(gi_ctx* ctx, int in_h, int in_w, int out_h, int out_w, void* tables_dev);
/* src: n x in_h x in_w uint8 (device). dst_f32 (n,out_h,out_w) in [0,1] and/or dst_u8 (either may be NULL).
 * tmp: n*in_h*out_w bytes (device). */
int gi_resize_to_tensor(gi_ctx* ctx, const void* tables_dev, const uint8_t* src, int n, int in_h, int in_w,
                        int out_h, int out_w, float* dst_f32, uint8_t* dst_u8, uint8_t* tmp);

/* ---- device mask generator (NOT in the reference, whose masks are files): the hole masks of a batch
 *      as a pure integer function of (kind, seed, key, H, W) - not of the batch, the image's place in it or n.
 *      Counter-based draws on the dropout hash: stream = mix(seed + G*(key+1)), draw(k) = mix(stream + G*(k+1)) >> 32,
 *      uni(k, lo, hi) = lo + ((draw(k) * (hi-lo+1)) >> 32). kind 0: one rectangle, h = uni(0, H/8, H/2), w = uni(1, W/8, W/2),
 *      y0 = uni(2, 0, H-h), x0 = uni(3, 0, W-w) (the benchmark's distribution). kind 1: the union of 2..5 thick polylines of
 *      3..11 segments each (at most 55 capsules, exact integer point-in-capsule test); DESIGN 4.1e-2 is the normative text
 *      and tests/maskgen_ref.py its numpy restatement, bit-exact with this entry.
 *      keys_dev: n int64 on the device; mask_out: (n,1,H,W) fp32 of {0,1}, 4-byte aligned; coverage_out (may be NULL):
 *      n ints, the number of ones per image (zeroed by the call, integer adds: deterministic). 16 <= H, W <= 4096, any
 *      value in between; n > 0. Invalid arguments return GI_ERR_INVALID before anything is launched; asynchronous on
 *      the context's stream. */
int gi_mask_generate(gi_ctx* ctx, int kind, uint64_t seed, const int64_t* keys_dev, int n, int H, int W, float* mask_out,
                     int* coverage_out);

/* ---- image output (NOT in the reference): fp32 tensors back to 8-bit pictures, and a repaired window back into a
 *      photograph of any size. All exact (integer arithmetic, or one fp32 multiply and rintf); tests/imageout_ref.py is the numpy
 *      restatement, bit-exact with every entry. All asynchronous on the context's stream; invalid arguments return
 *      GI_ERR_INVALID before anything is launched. Images are single-channel, row-major, dense. */
/* dst[i] = (uint8) rintf(min(max(src[i], 0), 1) * 255.0f), NaN -> 0: round to nearest even, so every byte v round-trips through
 * v / 255.0f (the truncating (x * 255).astype(uint8) of evaluate.py:156 stays with the FID path). Any count > 0, any dst
 * alignment; src 4-byte aligned. */
int gi_image_quantize(gi_ctx* ctx, const float* src, int64_t count, uint8_t* dst);
/* cols_host: a HOST array of ncol (1 .. 8) device pointers, each a (n,1,H,W) fp32 batch. canvas: (n*(H+g)+g) x (ncol*(W+g)+g)
 * uint8, g = gutter >= 0; tile (i, c) at row g + i*(H+g), column g + c*(W+g) holds the quantised cols[c][i], every other byte
 * is 255; one launch writes every canvas byte exactly once. */
int gi_panel_assemble(gi_ctx* ctx, const float* const* cols_host, int ncol, int n, int H, int W, int gutter, uint8_t* canvas);
/* bbox_out[4 i ..] = (y0, x0, y1, x1), the inclusive bounding box of the bytes != 0 of mask i of (n,H,W) uint8; an empty mask
 * gives (H, W, -1, -1). Integer min / max only: independent of any order. n <= 65535, H * W < 2^31 - 32. */
int gi_mask_bbox(gi_ctx* ctx, const uint8_t* mask, int n, int H, int W, int* bbox_out);
/* dst (wh, ww) = src[wy .. wy+wh)[wx .. wx+ww) of the (H, W) image; binarize != 0: every nonzero byte becomes 255. The window
 * lies inside the image. */
int gi_window_crop(gi_ctx* ctx, const uint8_t* src, int H, int W, int wy, int wx, int wh, int ww, int binarize, uint8_t* dst);
/* Writes the window's bytes of dst (H, W) and no others (the caller has copied orig there): with A = (2r+1)^2, a(p) the number
 * of hole pixels (mask != 0) in the (2r+1)^2 box around window pixel p (pixels outside the WINDOW count as 0) and
 * alpha(p) = A on a hole pixel, else min(A, 2 a(p)):  dst(p) = (alpha * patch(p) + (A - alpha) * orig(p) + A / 2) / A  in
 * integers. patch is dense (wh, ww); 0 <= r <= 63, r = 0 is a hard paste. At a straight hole edge the weight of the patch
 * falls linearly from 1 to 0 at distance r + 1. */
int gi_feather_paste(gi_ctx* ctx, const uint8_t* orig, const uint8_t* mask, int H, int W, int wy, int wx, int wh, int ww,
                     const uint8_t* patch, int r, uint8_t* dst);
/* Connected components of a hole mask (tests/components_ref.py is the restatement, exact in every output). mask: (H, W)
 * uint8, dense, any byte alignment, a byte != 0 is a hole pixel; connectivity 4 or 8; 1 <= cap <= 65536; H * W < 2^31 - 32.
 * labels_out (H, W) int32: -1 on background, on a hole pixel the smallest linear index y * W + x of any pixel of its component;
 * always complete, whatever cap is. count_out: one int, the true number of components, also when it exceeds cap. table_out
 * (cap, 6) int32: row k < min(count, cap) = (label, y0, x0, y1, x1, area) of the component with the k-th smallest label, the box
 * inclusive; the rows beyond are left untouched. workspace: gi_mask_components_workspace_bytes(H, W, cap) bytes on the device (0
 * for arguments the entry refuses); it and the three outputs are 4-byte aligned. Integer atomics only: every output is a pure
 * function of the mask, identical from run to run. */
size_t gi_mask_components_workspace_bytes(int H, int W, int cap);
int gi_mask_components(gi_ctx* ctx, const uint8_t* mask, int H, int W, int connectivity, int cap, int* labels_out, int* count_out,
                       int* table_out, void* workspace);

/* ---- batch assembly from a device-resident image store (lib/data/cache.py): store is (n_store,h,w) uint8 on
 *      the device, rows_dev n int64 on the device, out (n,h,w) of out_kind: 0 fp32 (float)v / 255.0f (the ToTensor quotient of
 *      gi_resize_to_tensor), 1 int64 v (segmentation labels), 2 uint8 v. out[i][y][x] = f(store[rows[i]][y][flip_i ? w-1-x : x]).
 *      flip_keys_dev (n int64 on the device; NULL: no flips): flip_i = mix(stream + G) >> 63 with
 *      stream = mix((flip_seed ^ 0x666C6970) + G * (key_i + 1)) on the dropout hash, independent of the mask draws of the same
 *      key (tests/batchgather_ref.py is the numpy restatement, bit-exact with this entry). A row outside [0, n_store) reads
 *      nothing and yields zeros. out is aligned to its element; 16-byte alignment (4 for uint8) with w % 4 == 0 takes the
 *      vector path. h * w < 2^31. Invalid arguments return GI_ERR_INVALID before anything is launched; asynchronous on the
 *      context's stream. */
int gi_batch_gather(gi_ctx* ctx, const uint8_t* store, int64_t n_store, int h, int w, const int64_t* rows_dev, int n,
                    const int64_t* flip_keys_dev, uint64_t flip_seed, int out_kind, void* out);

/* ---- differentiable augmentation of the critic's inputs (NOT in the reference): per sample of a (n,1,H,W) fp32
 *      batch, in this order, colour  v = c (x - m) + (m + b)  with m the sample's mean, an integer translation t = (ty, tx) with
 *      zero fill, and a cutout window set to zero:  y[q] = v[q - t] if q - t is inside the image and q outside the window, else 0.
 *      The adjoint is  dv[p] = dy[p + t] if p + t is inside the image and outside the window, else 0;  dx = c dv + (1 - c) mean(dv).
 *      policy: bits 1 colour, 2 translation, 4 cutout (any non-empty subset). The parameters are draws of the mask generator's
 *      scheme above with seed' = seed ^ 0x4449464641554721 and key_i = key0 + i for sample i:  b = (draw(0) >> 8) 2^-24 - 0.5,
 *      c = 0.5 + (draw(1) >> 9) 2^-23,  ty = uni(2, -(H/8), H/8), tx = uni(3, -(W/8), W/8),  cy = uni(4, 0, H), cx = uni(5, 0, W);
 *      the window is ch = H/2 by cw = W/2 from y0 = cy - ch/2, x0 = cx - cw/2 (integer divisions). A disabled operation leaves
 *      b = 0, c = 1 / t = 0 / ch = cw = 0 and does not change the other operations' draws.
 *      table: n rows of 8 32-bit words on the device, {b, c (fp32), ty, tx, y0, x0, ch, cw (int32)}, the window unclipped.
 *      gi_diffaug_fwd / _bwd take a table (hand-written ones included) and `colour` (0: the values are moved bit for bit, b and c
 *      are not read; else the fp32 arithmetic above, every operation rounded once, the means summed in fp64 in a fixed order:
 *      deterministic, independent of n and of the sample's row). gi_diffaug_apply / _apply_bwd draw the parameters themselves
 *      (no table launch): the production entries. x / y (dy / dx): n samples each, 4-byte aligned, not overlapping, any n-row
 *      slices of larger buffers; W % 4 == 0 with 16-byte aligned buffers takes the 128-bit path. n > 0, H, W >= 1,
 *      H * W < 2^31. Invalid arguments return GI_ERR_INVALID before anything is launched; asynchronous on the context's stream. */
int gi_diffaug_params(gi_ctx* ctx, int policy, uint64_t seed, uint64_t key0, int n, int H, int W, void* table);
int gi_diffaug_fwd(gi_ctx* ctx, const float* x, const void* table, int n, int H, int W, int colour, float* y);
int gi_diffaug_bwd(gi_ctx* ctx, const float* dy, const void* table, int n, int H, int W, int colour, float* dx);
int gi_diffaug_apply(gi_ctx* ctx, int policy, uint64_t seed, uint64_t key0, const float* x, int n, int H, int W, float* y);
int gi_diffaug_apply_bwd(gi_ctx* ctx, int policy, uint64_t seed, uint64_t key0, const float* dy, int n, int H, int W, float* dx);

/* ---- single-layer entry points (unit parity tests and kernel roofline measurements) -------- */
/* out[n,y,x,a] = act( sum_{ky,kx,b} in[n,2y-1+ky,2x-1+kx,b] * w[a][ky][kx][b] ), NHWC, dtype T.
 * in: (n,H,W,cb) ld=ldin; out: (n,H/2,W/2,ca) ld=ldout. w_packed is T [ca][16*cb].
 * partials (may be NULL) receives per-tile column sum / sum of squares; ws: split-K scratch */
int gi_conv_s2_forward(gi_ctx* ctx, int dtype, const void* in, const void* w_packed, void* out,
                       int n, int H, int W, int cb, int ldin, int ca, int ldout, int relu_in,
                       int act_out, float* ws, int64_t ws_bytes);
/* out[n,2y-1+ky,2x-1+kx,b] += in[n,y,x,a]*w[a][ky][kx][b] (transposed conv k4 s2 p1) as four
 * sub-pixel 2x2 convolutions. in: (n,H,W,ca); out: (n,2H,2W,cb); w_phase is T [4][cb][4*ca]
 * produced by gi_pack_weights */
int gi_convT_s2_forward(gi_ctx* ctx, int dtype, const void* in, const void* w_phase, void* out,
                        int n, int H, int W, int ca, int ldin, int cb, int ldout, int relu_in,
                        int act_out, float* ws, int64_t ws_bytes);
/* The same two layers with the fused epilogues the networks use (all optional, zero = absent; nothing here exists in the
 * reference: these are the seams at which its separate BatchNorm / activation modules, networks.py:285-318, are folded into the
 * GEMMs). Fields marked (returned) say whether the kernel that served the shape implemented the fusion; if not, the caller
 * runs the separate pass. */
typedef struct gi_igemm_ex {
  int relu_cend;                 /* with relu_in: only input channels [0, relu_cend) need the ReLU (0 = all). A hint for inputs whose
                                  * channels from relu_cend on are already non-negative (the decoder half of a concat buffer): kernels
                                  * may apply the ReLU to more channels. Must be a multiple of 64 and <= the input channels. */
  /* activation backward on the result: out = (out + [mask > 0] * add) * (mask > 0 ? 1 : mask_slope); mask / add laid out
   * like out with leading dimensions ldmask / ldadd (the LeakyReLU backward of a norm-free layer, networks.py:287) */
  const void* mask; int ldmask; float mask_slope;
  const void* add; int ldadd;
  /* with mask, optional: one 64-bit sign word per output pixel, bit c = [mask[p][c] > 0] for its first 64 channels. The kernel
   * that takes them (sub-pixel phases with 64 output channels) reads 8 bytes per pixel instead of 128 and applies the slope to
   * its fp32 accumulators (one rounding: within fp16 rounding of the result without them) */
  const unsigned long long* mask_bits;
  /* BatchNorm batch statistics of the result: every tile adds its column sum / sum of squares to the exact accumulator
   * block stat_acc (gi_stat_acc_words(ca) zeroed 64-bit words; tile t -> replica t mod stat_reps, a power of two <= 4;
   * stat_pg > 0: GEMM rows >= stat_pg belong to a second population). partials: per-tile rows instead, [tiles][2][c] */
  unsigned long long* stat_acc; int stat_reps; int stat_pg;
  float* partials;
  /* BatchNorm-backward reduction of the layer whose output gradient this GEMM produces: with x = bwd_x (raw convolution
   * output, ld bwd_ldx), dz = g * (fma(x, scale, shift) > 0 ? 1 : bwd_slope), xhat = (x - mean) * inv, every tile adds
   * sum dz and sum dz * xhat to bwd_acc (layout as stat_acc; populations of bwd_pg output pixels, vectors bwd_stride apart) */
  const void* bwd_x; int bwd_ldx;
  const float* bwd_scale; const float* bwd_shift; const float* bwd_mean; const float* bwd_inv; int bwd_stride;
  float bwd_slope; unsigned long long* bwd_acc; int bwd_reps; int64_t bwd_pg;
  /* bwd_c > 0: only the output columns [bwd_c0, bwd_c0 + bwd_c) carry that gradient (multiples of 128; the decoder half of a U-Net
   * concat gradient): bwd_x, the vectors and bwd_acc hold bwd_c channels, indexed by column - bwd_c0. Taken by the kernels that
   * serve layers of >= 512 workgroups; otherwise bwd_applied stays 0 */
  int bwd_c0, bwd_c;
  int mask_applied, bwd_applied, stat_used, ntiles_out;   /* (returned) */
} gi_igemm_ex;
int gi_conv_s2_forward_ex(gi_ctx* ctx, int dtype, const void* in, const void* w_packed, void* out,
                          int n, int H, int W, int cb, int ldin, int ca, int ldout, int relu_in,
                          int act_out, float* ws, int64_t ws_bytes, gi_igemm_ex* ex);
int gi_convT_s2_forward_ex(gi_ctx* ctx, int dtype, const void* in, const void* w_phase, void* out,
                           int n, int H, int W, int ca, int ldin, int cb, int ldout, int relu_in,
                           int act_out, float* ws, int64_t ws_bytes, gi_igemm_ex* ex);
/* Which kernel the two entries above (mode 0 / 1) or a 3x3 / s1 VGG convolution (mode 2) would launch for a layer, without launching
 * it: the same decision function on the same arguments, host arithmetic only - no HIP call, works without a GPU. n, Hs, Ws: the small
 * grid (mode 0: the output, H / 2 x W / 2); ws_bytes > 0: a workspace of that size is passed, has_tickets: and the split-K ticket
 * counters; ex as above (pointers are only tested for null; may be null); offered: what the networks can add to a launch -
 * 1 the folded normalisation (with ex->stat_acc), 2 the first layer's weight gradient (with ex->mask_bits), 4 the pooled store,
 * 8 a bias. Returns as the entries do (GI_ERR_INVALID with gi_last_error set; mode 2: GI_ERR_UNSUPPORTED when no kernel serves it). */
typedef struct gi_igemm_plan_info {
  char name[48];                 /* what gi_debug_last_kernel would say after the launch */
  int grid, splitk, ntiles_out;  /* workgroups, K splits */
  int mask_applied, bwd_applied, stat_used, c1w_applied, c1w_blocks, pool_applied, fold_applied;
} gi_igemm_plan_info;
int gi_debug_igemm_plan(int dtype, int mode, int n, int Hs, int Ws, int cin, int ldin, int cout, int ldout, int relu_in,
                        int act_out, int64_t ws_bytes, int has_tickets, const gi_igemm_ex* ex, int offered,
                        gi_igemm_plan_info* out);
/* exact accumulator blocks (csrc/stat_acc.h): words per block of c channels; totals of the two quantities of a population
 * as doubles, out_dev[2][c] (device) */
int64_t gi_stat_acc_words(int c);
int gi_stat_acc_read(gi_ctx* ctx, const unsigned long long* acc, int c, int reps, int group, double* out_dev);
/* dW[a][ky][kx][b] += scale * sum_{n,y,x} S[n,y,x,a] * L[n,2y-1+ky,2x-1+kx,b] */
int gi_wgrad_s2(gi_ctx* ctx, int dtype, const void* S, const void* L, float* dW, int n, int Hs, int Ws,
                int ca, int ldS, int cb, int ldL, int relu_S, float scale);
/* the same with a scratch buffer of gi_wgrad_s2_scratch_bytes(...) bytes: the pixel-range splits write their partial
 * tiles with plain stores and a fixed-order pass adds them to dW - deterministic and faster than the fp32 atomics
 * gi_wgrad_s2 uses (scratch NULL or too small falls back to them) */
int64_t gi_wgrad_s2_scratch_bytes(int dtype, int n, int Hs, int Ws, int ca, int cb);
int gi_wgrad_s2_ws(gi_ctx* ctx, int dtype, const void* S, const void* L, float* dW, int n, int Hs, int Ws,
                   int ca, int ldS, int cb, int ldL, int relu_S, float scale, float* scratch, int64_t scratch_bytes);
/* ---- the single-channel layers on their own (test seam) ------------------------------------------------------------------
 * The layers whose large side has ONE channel: img is fp32 (n,1,2Hs,2Ws), the feature side NHWC of type T with row pitch ld and
 * channel offset coff, w the fp32 master [c][16] (tap = ky*4 + kx). Each call runs the dispatcher of csrc/c1.hip on the
 * context's stream; gi_debug_last_kernel() names the form that served it ("c1_gather_mfma<4|8>", "c1_gather_strip", "c1_gather",
 * "c1_scatter_fused<2|4>", "c1_col+col2im<2|4>", "c1_scatter", "c1_wgrad_mfma[,atomics]", "c1_wgrad[,atomics]", "c1_head4",
 * "c1_head4_dgrad").
 * gather: out[p][coffout + ch] = act(bias[ch] + sum_tap img[n,2y-1+ky,2x-1+kx] * in_scale * w[ch][tap]). bits (or NULL): one sign word
 * per pixel (bit ch = [out > 0]) where the serving form writes them (fp16, c = 64); *bits_written says whether it did. */
int gi_c1_gather(gi_ctx* ctx, int dtype, const float* img, const float* w, void* out, int n, int Hs, int Ws, int c,
                 int ldout, int coffout, int act_out, float in_scale, const float* bias, unsigned long long* bits,
                 int* bits_written);
/* scatter: img = post(bias[0] + conv_transpose(relu?(X), w)) * out_scale, post 1 = tanh; img2 (or NULL) a second copy. col_scratch
 * (or NULL): n*Hs*Ws*16 values of type fp16 for the fp16 matrix-core forms. x2 != NULL (fp16, c in {64, 128}, Ws % 32 == 0): channels
 * [c/2, c) are not read from X but are relu(fma(x2[p][ch - c/2], scale2, shift2)) rounded to fp16, x2 of row pitch ld2. */
int gi_c1_scatter(gi_ctx* ctx, int dtype, const void* X, const float* w, const float* bias, float* img, int n, int Hs,
                  int Ws, int c, int ldx, int coffx, int relu_in, int post, float out_scale, void* col_scratch,
                  float* img2, const void* x2, int ld2, const float* scale2, const float* shift2);
/* dW[ch][tap] += scale * sum_p relu?(X[p][ch]) * img[n,2y-1+ky,2x-1+kx] * img_scale; x2 .. shift2 as above. scratch (or NULL,
 * scratch_floats floats): the workgroups' partial sums, added in a fixed order; without it float atomics */
int gi_c1_wgrad(gi_ctx* ctx, int dtype, const void* X, const float* img, float* dW, int n, int Hs, int Ws, int c, int ldx,
                int coffx, int relu_in, float scale, float img_scale, const void* x2, int ld2, const float* scale2,
                const float* shift2, float* scratch, int64_t scratch_floats);
/* dW[i] += sum over `blocks` rows of part[block][count] in a fixed order; scratch (>= 64 * count floats, or NULL): a first
 * stage over row ranges when there are 256 rows or more */
int gi_c1_wgrad_reduce(gi_ctx* ctx, const float* part, float* dW, int count, int blocks, float* scratch,
                       int64_t scratch_floats);
/* the 4-class head (fp16, 128 input channels, w fp32 [c][16][4]): out = tanh(bias + conv_transpose(relu?(X), w)) as (n,4,2Hs,2Ws)
 * fp32 (out2: a second copy or NULL), col_scratch of gi_c1_head4_col_bytes bytes; dgrad: out[p][coffout + ch] from the
 * (n,4,2Hs,2Ws) fp32 gradient g */
int64_t gi_c1_head4_col_bytes(int n, int Hs, int Ws);
int gi_c1_head4_forward(gi_ctx* ctx, const void* X, const float* w, const float* bias, float* out, float* out2, int n,
                        int Hs, int Ws, int ldx, int coffx, int relu_in, void* col_scratch);
int gi_c1_head4_dgrad(gi_ctx* ctx, const float* g, const float* w, void* out, int n, int Hs, int Ws, int ldout,
                      int coffout);
/* ---- the normalisation and activation-backward passes on their own (test seam) ---------------------------------------------
 * Each entry checks what the kernels assume and forwards to the pass of csrc/norm.hip or csrc/elementwise.hip that the networks call; nothing here is
 * on a training path. Tensors are NHWC of the compute type T (pixels x channels, row pitch ld, channel offset coff; both multiples of
 * the 16-byte chunk: 8 channels for fp16, 4 for fp32); vectors are fp32. c / chunk must be a power of two <= 256 except for the
 * InstanceNorm passes (any multiple of the chunk). tests/norm_ref.py restates every one of them in fp64.
 * col_stats: partials[row][2][c] = column sum / sum of squares of a dense (pixels, c) tensor, *rows_out rows
 * (partials: at least (pixels / 32 + 8) * 2 * c floats).
 * bn_finalize: BatchNorm2d from partial rows: scale = gamma * inv, shift = beta - mean * scale, save_mean, save_invstd; train: batch
 * statistics (biased variance), running statistics moved with `momentum` (unbiased variance; count 1: the biased one); eval: the
 * running statistics. groups = 2: two populations, their rows part_stride floats and their outputs out_stride floats apart, the
 * running statistics moved population by population.
 * bn_apply: y[p][coffy + ch] = drop(act(fma(x[p][ch], scale, shift))), drop = keep-mask byte (dense, pixels x c) ? v * drop_scale : 0.
 * 0 < pg < pixels: pixels >= pg take scale / shift at + gstride floats. */
int gi_debug_col_stats(gi_ctx* ctx, int dtype, const void* x, int64_t pixels, int c, float* partials, int* rows_out);
int gi_debug_bn_finalize(gi_ctx* ctx, const float* partials, int rows, int c, int64_t count, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, float* scale, float* shift,
                         float* save_mean, float* save_invstd, int train, float momentum, float eps, int groups,
                         int64_t part_stride, int out_stride);
int gi_debug_bn_apply(gi_ctx* ctx, int dtype, const void* x, void* y, int64_t pixels, int c, int ldy, int coffy,
                      const float* scale, const float* shift, int act, const uint8_t* drop_mask, float drop_scale, int64_t pg,
                      int gstride);
/* The same from an exact accumulator block (csrc/stat_acc.h: quantity 0 = sum x, 1 = sum x^2 per population), train mode only. */
typedef struct gi_bn_acc_args {
  const unsigned long long* acc; int reps;       /* block of gi_stat_acc_words(c) words, `reps` replicas in use (1 .. 4) */
  const float* gamma; const float* beta;
  float* running_mean; float* running_var;
  float* scale; float* shift; float* save_mean; float* save_invstd;   /* [groups], out_stride floats apart */
  int64_t count;                                 /* pixels per population */
  float momentum, eps;
  int groups, out_stride;
  unsigned long long* zero_next; int zero_words; /* optional: 64-bit words the pass clears */
} gi_bn_acc_args;
int gi_debug_bn_finalize_acc(gi_ctx* ctx, int c, const gi_bn_acc_args* b);
/* finalize + bn_apply in one pass over pixels = groups * count. drop_mask with drop_p > 0: the keep-mask is drawn in the pass
 * (gi_debug_fill_dropout's draw for drop_seed) and stored there; drop_p == 0: it is read. side_bytes > 0 (a multiple of 16): side_src
 * is copied to side_dst by the same launch. */
int gi_debug_bn_apply_acc(gi_ctx* ctx, int dtype, const void* x, void* y, int64_t pixels, int c, int ldy, int coffy, int act,
                          uint8_t* drop_mask, float drop_scale, uint64_t drop_seed, float drop_p, const gi_bn_acc_args* b,
                          const void* side_src, void* side_dst, int64_t side_bytes);
/* backward through [dropout] -> activation -> [BatchNorm]: dz = (g1 + g2 * [s > 0]) * (s > 0 ? 1 : slope(act)) * drop_scale with
 * s = y, or fma(x, fwd_scale, fwd_shift) when those are given; slope: 1 / 0 / 0.2 for none / ReLU / LeakyReLU. Without BatchNorm
 * dx = dz. Train-mode BatchNorm: dx = gamma * inv * (dz - mean(dz) - xhat * mean(dz * xhat)) per population, dbeta += sum dz *
 * inv_loss_scale, dgamma += sum dz * xhat * inv_loss_scale; eval_bn: dx = gamma * inv * dz, the parameter gradients untouched.
 * drop_scale != 1 needs act = ReLU: the dropout zeros are taken from y > 0. */
typedef struct gi_act_bn_bwd_args {
  const void* g1; int ldg1, coffg1;              /* may be NULL */
  const void* g2; int ldg2, coffg2;              /* may be NULL */
  const void* y; int ldy, coffy;                 /* saved activation output */
  const void* x;                                 /* raw tensor in front of the norm, dense; NULL without has_bn */
  void* dx;                                      /* dense */
  int64_t pixels; int c;
  int act; float drop_scale;
  int has_bn, eval_bn;
  const float* gamma; const float* save_mean; const float* save_invstd;
  float* dgamma; float* dbeta; float inv_loss_scale;
  float* partials;                               /* scratch (pixels / 32 + 8) * 2 * c floats */
  float* sums;                                   /* scratch groups * 8 * c floats */
  const float* fwd_scale; const float* fwd_shift;
  int groups, stat_stride;                       /* 2: two populations, the second one's vectors at + stat_stride floats */
  unsigned long long* acc; int acc_reps;         /* exact accumulator block (zeroed) for the two sums, or NULL */
  unsigned long long* zero_next; int zero_words;
  int reduce_done;                               /* 1: the sums are in acc already */
} gi_act_bn_bwd_args;
int gi_debug_act_bn_bwd(gi_ctx* ctx, int dtype, const gi_act_bn_bwd_args* a);
/* InstanceNorm2d(affine = False): statistics per (image, channel) over hw pixels, stats[n][c][2] = mean, inv; x dense (n * hw, c).
 * The backward takes g1, g2, y, x, dx, pixels, c, act and drop_scale from the argument block. */
int gi_debug_in_forward(gi_ctx* ctx, int dtype, const void* x, void* y, int n, int hw, int c, int ldy, int coffy, int act,
                        const uint8_t* drop_mask, float drop_scale, float eps, float* stats);
int gi_debug_act_in_bwd(gi_ctx* ctx, int dtype, const gi_act_bn_bwd_args* a, int n, int hw, const float* stats);
/* dbias[ch] += scale * sum_p dz[p][ch] (partials: scratch as for col_stats); dx = dy * (1 - y^2) * scale; keep-mask bytes of the
 * counter-based dropout draw (1 with probability 1 - p); byte masks between (n, c, hw) and (n, hw, c) */
int gi_debug_bias_grad(gi_ctx* ctx, int dtype, const void* dz, int64_t pixels, int c, float scale, float* dbias, float* partials);
int gi_debug_tanh_bwd(gi_ctx* ctx, const float* dy, const float* y, float* dx, int64_t count, float scale);
int gi_debug_fill_dropout(gi_ctx* ctx, uint8_t* mask_nhwc, int64_t count, uint64_t seed, float p);
int gi_debug_mask_layout(gi_ctx* ctx, const uint8_t* src, uint8_t* dst, int n, int c, int hw, int to_nhwc);
/* gradient-penalty helpers: tout = tin * (a > 0 ? 1 : 0.2); the primal-gradient term of a differentiated BatchNorm tangent map
 * (dxp += inj, dgamma += dgamma_scale * A * inv; partials: (pixels / 32 + 8) * 5 * c floats, sums: 5 * c floats); the penalty's
 * direction v = s * d(lam * mean_n (||g_n|| - 1)^2) / dg with s = 2^k so that max|v| is in [1, 2), sc = {s, 1 / s}, sumsq / amax n
 * floats each; dst += src * sc[1] */
int gi_debug_mul_slope(gi_ctx* ctx, int dtype, const void* tin, const void* a, void* tout, int64_t count);
int gi_debug_bn_tangent_inject(gi_ctx* ctx, int dtype, const void* dta, const void* y, const void* tx, const void* x, void* dxp,
                               int64_t pixels, int c, const float* gamma, const float* mean, const float* inv, float* dgamma,
                               float dgamma_scale, float* partials, float* sums);
int gi_debug_gp_direction(gi_ctx* ctx, const float* g, int n, int64_t hw, float lam, float* sumsq, float* amax, float* v,
                          float* penalty, float* sc);
int gi_debug_gp_unscale_add(gi_ctx* ctx, const float* src, const float* sc, float* dst, int64_t count);
/* Spectral normalisation, one op at a time (specnorm.hip), any ca >= 1, K >= 1. w: ca x K row-major; cb > 0: a 4x4 convolution
 * weight in the master layout [a][ky][kx][b] (K = 16 cb) whose memory column kk * cb + b is column b * 16 + kk of v; cb = 0:
 * plain row-major. train: `iters` rounds of the power iteration update u (ca) and v (K) in place; else they are only read.
 * *sigma_out = u . (W v). All device pointers; synchronises the context's stream. */
int gi_debug_sn_power_iteration(gi_ctx* ctx, const float* w, int ca, int K, int cb, float* u, float* v, int iters, int train,
                                float* sigma_out);
/* dst += scale * (g - <g, w_eff>_F u v^T) / sigma; scale = scale_dev ? *scale_dev : 1; sigma: one device float. */
int gi_debug_sn_project_add(gi_ctx* ctx, const float* g, const float* w_eff, const float* u, const float* v, const float* sigma,
                            int ca, int K, int cb, const float* scale_dev, float* dst);
/* adds addends[row][c] (fp32, device) to quantity q of population `group` of an accumulator block, row r into replica r & (reps - 1),
 * one workgroup per row and one lane per channel as the producing kernels do */
int gi_debug_stat_acc_add(gi_ctx* ctx, unsigned long long* acc, int c, int reps, int group, int q, const float* addends,
                          int rows);
/* The weight re-pack that runs after every update, on its own: `n` (1 .. 16) jobs, a HOST array, in ONE launch. Per job w is the fp32
 * master [ca][16][cb]; packed (or NULL) receives T [ca][16][cb], phase (or NULL) T [4][cb][4][ca] as gi_pack_weights writes them;
 * scale (or NULL): ca (scale_on_b = 0) or cb (1) fp32 factors multiplied in before the conversion (the inference-time BatchNorm
 * fold). When every ca and cb is a multiple of 64 the 64 x 64-tile kernel runs (w, a per-b scale and both copies 16-byte aligned,
 * fp16 copies 8-byte), else the 32 x 32-tile one. */
typedef struct gi_pack_job {
  const float* w; void* packed; void* phase;
  int ca, cb, scale_on_b;
  const float* scale;
} gi_pack_job;
int gi_debug_pack_weights_batch(gi_ctx* ctx, int dtype, const gi_pack_job* jobs, int n);
/* ---- the PatchGAN critic head on its own (test seam) ------------------------------------------------------------------------
 * Conv2d(c,1,4,1,0) + Flatten + Linear(P,1) [+ Sigmoid] of csrc/head.hip, forward and backward; each entry checks what the kernels
 * assume (GI_ERR_INVALID before any launch) and forwards to the dispatcher the networks call; nothing here is on a training path.
 * a4 is dense NHWC (n,Hh,Wh,c) of the compute type, c a multiple of the 16-byte chunk, Hh, Wh >= 4; Ph = Hh - 3, Pw = Wh - 3,
 * P = Ph * Pw; w5 fp32 [16][c] (tap = ky*4 + kx), wl fp32 [P], bl fp32 [1]. tests/head_ref.py restates every formula in fp64.
 * forward:  h[i,py,px] = sum_{ky,kx,ch} x[i,py+ky,px+kx,ch] * w5[ky*4+kx][ch];  out[i] = [sigmoid](bl + sum_p wl[p] * h[i,p]); out2
 *           (or NULL) a second copy. x = a4, or with scale4 / shift4 (fp16, c = 512 only) x = fp16(lrelu(fma(a4, scale4[g], shift4[g])))
 *           with slope 0.2, g = i / n_per_group (0: one population), population g's vectors at + g * gstride floats. bn (with scale4):
 *           the vectors are derived from the exact accumulators and published at bn->scale / shift / save_mean / save_invstd, the
 *           running statistics moved population by population and bn->zero_next cleared (bn->out_stride == gstride). tbuf (or NULL):
 *           n * Hh * Wh * 16 floats that let the fp16 c = 512 kernel slice a large map over workgroups.
 * backward: dz[i] = dy[i] * (sigmoid ? out[i] * (1 - out[i]) : 1); dh[i,p] = dz[i] * wl[p];
 *           da4[i,y,x,ch] = T(loss_scale * sum_tap dh[i,y-ky,x-kx] * w5[tap][ch]) over the valid positions;
 *           dw5[tap][ch] += sum_{i,p} dh[i,p] * x[i,p+tap,ch]; dwl[p] += sum_i dz[i] * h[i,p]; dbl += sum_i dz[i]   (NULL: frozen).
 *           dh: (n,P) scratch, written by the generic kernels only. scratch (or NULL): the weight-gradient partials,
 *           gi_debug_head_scratch_bytes(); the fp16 c = 512 kernels fall back to the generic ones when it is too small, the generic
 *           ones to float atomics. bwd_acc with bwd_x (fp16 c = 512): with x = bwd_x (dense raw tensor) and the stored da4,
 *           dz = da4 * (fma(x, bwd_scale, bwd_shift) > 0 ? 1 : bwd_slope), xhat = (x - bwd_mean) * bwd_inv: sum dz (quantity 0) and
 *           sum dz * xhat (quantity 1) per channel are added to the accumulator block, population i / bwd_n_per_group, vectors
 *           bwd_stride floats apart, bwd_reps (1, 2 or 4) replicas; bwd_applied = 1 when the kernel did it.
 * gi_debug_last_kernel() names the path: "head_fwd512", "head_fwd512_sliced", "head_fwd", "head_bwd512", "head_bwd". */
typedef struct gi_head_args {
  const void* a4; const float* w5; const float* wl; const float* bl;
  float* h; float* out;
  int n, Hh, Wh, c, sigmoid;
  float* out2;
  const float* scale4; const float* shift4; int n_per_group, gstride;
  float* tbuf; int64_t tbuf_bytes;
  const gi_bn_acc_args* bn;
} gi_head_args;
typedef struct gi_head_bwd_args {
  const void* a4; const float* w5; const float* wl; const float* h; const float* out;
  const float* dy;
  void* da4;
  float* dw5; float* dwl; float* dbl;
  float* dh;
  int n, Hh, Wh, c, sigmoid;
  float loss_scale;
  float* scratch; int64_t scratch_bytes;
  const float* scale4; const float* shift4; int n_per_group, gstride;
  const void* bwd_x;
  const float* bwd_scale; const float* bwd_shift; const float* bwd_mean; const float* bwd_inv;
  int bwd_stride, bwd_n_per_group, bwd_reps; float bwd_slope;
  unsigned long long* bwd_acc;
  int bwd_applied;                               /* returned */
} gi_head_bwd_args;
int gi_debug_head_forward(gi_ctx* ctx, int dtype, const gi_head_args* a);
int gi_debug_head_backward(gi_ctx* ctx, int dtype, gi_head_bwd_args* a);
int64_t gi_debug_head_scratch_bytes(int max_n, int Hh, int Wh);
/* ---- the VGG-19 loss path's kernels on their own (test seam) ------------------------------------------------------------------
 * Each entry checks what its kernel assumes (GI_ERR_INVALID before any launch) and runs the host launch code of csrc/vgg.hip that the
 * network runners use; nothing here is on a training path. Feature maps are dense NHWC fp16; tests/vgg_ops_ref.py restates every op.
 * conv3x3: one 3x3 / s1 / p1 convolution on the mode-2 implicit GEMMs. w: fp32 master [cout][cin][3][3], packed into w_packed
 * (cout * 9 * cin halves) first. transposed = 0: in (n,H,W,cin) -> out (n,H,W,cout) = act_out(bias + conv). transposed = 1: the input
 * gradient, in (n,H,W,cout) -> out (n,H,W,cin). bias, mask, add (each may be NULL) have the OUTPUT's channels: with mask the result is
 * [mask > 0] * (conv + add) where the serving kernel has that epilogue (*mask_applied = 1), the plain convolution otherwise. pool2:
 * where the kernel can (*pool_applied = 1), `out` receives the (n,H/2,W/2,.) max pool instead. gi_debug_last_kernel() names the kernel. */
int gi_debug_vgg_conv3x3(gi_ctx* ctx, const void* in, const float* w, void* w_packed, void* out, int n, int H, int W, int cin,
                         int cout, int transposed, const float* bias, int act_out, int pool2, const void* mask, const void* add,
                         int* pool_applied, int* mask_applied);
/* conv1_1 on the replicated grey images xa, xb (n,H,W fp32 each): w [64][3][3][3], w1 [64][9] receives the weights summed over the
 * input channel, out [2n][H][W][64] fp16 = relu(bias + conv) */
int gi_debug_vgg_conv1(gi_ctx* ctx, const float* xa, const float* xb, int n, int H, int W, const float* w, const float* bias,
                       float* w1, void* out);
int gi_debug_vgg_maxpool2(gi_ctx* ctx, const void* in, void* out, int nimg, int Ho, int Wo, int C);   /* in (nimg,2Ho,2Wo,C) */
/* both terms of one tap from F [2n][HW][C] (output images, then target images): terms2 = {mean (F_o - F_t)^2, mean (G_o - G_t)^2},
 * G = F^T F / (HW C); with dg / amax (both or neither): the dense dg [n][C][C] = G_o - G_t and the bit pattern of max |dg|.
 * force_split > 0 replaces the first guess of the pixel-range split; *split_out: the split that ran. ws: gi_debug_vgg_tap_ws_bytes()
 * bytes, 256-byte aligned. */
int64_t gi_debug_vgg_tap_ws_bytes(void);
int gi_debug_vgg_tap_terms(gi_ctx* ctx, const void* F, int n, int HW, int C, int force_split, void* ws, int64_t ws_bytes,
                           float* terms2, float* dg, unsigned* amax, int* split_out);
/* seed of a tap, d(weight_p P + weight_s S) / dF_o, from Fo, Ft [n][HW][C], dg [n][C][C] and dmax (bit pattern of max |dg|).
 * store = 0: *smax = max(*smax, max |seed|) as a bit pattern (maps of more than 2048 pixels: over one 256-pixel block of eight);
 * store = 1: sc[0] * seed in fp16 over Ft. scale: sc = {s, 1 / s}, s the power of two that puts *smax into [2^-3, 2^-2). */
int gi_debug_vgg_seed(gi_ctx* ctx, int store, const void* Fo, void* Ft, const float* dg, const unsigned* dmax, unsigned* smax,
                      const float* sc, int n, int HW, int C, float weight_p, float weight_s);
int gi_debug_vgg_scale(gi_ctx* ctx, const unsigned* smax, float* sc);
/* pool = 0: out = [act > 0 or !relu] * (g + seed), g / seed may be NULL, out may be g. pool = 1: g (n,H/2,W/2,C) routed to the first
 * maximum of every 2x2 window of act (n,H,W,C), times [max > 0 or !relu]; zeros elsewhere */
int gi_debug_vgg_act_bwd(gi_ctx* ctx, int pool, const void* g, const void* act, const void* seed, void* out, int n, int H, int W,
                         int C, int relu);
/* dimg (n,H,W fp32) = gscale * sc[1] * adjoint of the 1 -> 64 convolution w1 [64][9] applied to D (n,H,W,64) fp16 */
int gi_debug_vgg_conv1_adjoint(gi_ctx* ctx, const void* D, const float* w1, const float* sc, float gscale, float* dimg, int n,
                               int H, int W);
/* ---- the LPIPS kernels on their own (test seam; csrc/lpips.hip, restated by tests/lpips_ref.py). Each entry checks what its kernel
 * assumes and runs the host launch code the handle uses.
 * conv1: out [2n][H][W][64] fp16 = relu(bias + sum_tap wA[.][tap] x[tap] + sum_tap wB[.][tap] [tap inside the image]) for the images
 * xa, xb (n,H,W fp32 each); wA, wB [64][9], bias [64] fp32; W a multiple of 16.
 * fold: w [64][3][3][3], shift[3], scale[3] -> wA = sum_c w * 2 / scale_c, wB = sum_c w * (-1 - shift_c) / scale_c.
 * tap: F [2n][H][W][C] fp16 (image i pairs with image i + n; C = 64, 128, 256 or 512), lin [C] fp32 -> d_n[i]; with pooled (H, W even):
 * the fused form, which also writes the 2x2 max pool [2n][H/2][W/2][C]. F, lin, pooled 16-byte aligned; ws: gi_debug_lpips_tap_ws_bytes(n)
 * bytes, 8-byte aligned. */
int gi_debug_lpips_conv1(gi_ctx* ctx, const float* xa, const float* xb, int n, int H, int W, const float* wA, const float* wB,
                         const float* bias, void* out);
int gi_debug_lpips_fold(gi_ctx* ctx, const float* w, const float* shift, const float* scale, float* wA, float* wB);
int64_t gi_debug_lpips_tap_ws_bytes(int n);
int gi_debug_lpips_tap(gi_ctx* ctx, const void* F, int n, int H, int W, int C, const float* lin, void* ws, int64_t ws_bytes,
                       float* d_n, void* pooled);
/* the LPIPS backward's kernels (restated by tests/lpips_grad_ref.py).
 * pack_t: w [cout][cin][3][3] fp32 -> fp16 [cin][8 - tap][cout], the weights of the transposed convolution.
 * seed: F [2n][HW][C] fp16 (a images, then b images), lin [C]. store = 0: smax[i] = max(smax[i], max |seed of pair i|) as a bit
 * pattern; store = 1: sc[i] * seed in fp16 over the b half of F. seed = d d_l / d a (see gi_lpips_distance_grad), 0 where a is 0.
 * scale: sc[i] = s_i, the power of two that puts smax[i] into [2^-3, 2^-2) (1 when smax[i] is 0), sc[n + i] = 1 / s_i.
 * act_bwd: pool = 0: out = [act > 0 or !relu] * (g + seed), g / seed may be NULL, out may be g. pool = 1: g (n,H/2,W/2,C) routed to
 * the first maximum of every 2x2 window of act (n,H,W,C), then out = [act > 0 or !relu] * (routed g + seed) (seed may be NULL).
 * conv1_adjoint: dimg (n,H,W fp32) = gscale * sc_inv[i] * adjoint of the 1 -> 64 convolution wA [64][9] applied to D (n,H,W,64) fp16. */
int gi_debug_lpips_pack_t(gi_ctx* ctx, const float* w, void* out, int cout, int cin);
int gi_debug_lpips_seed(gi_ctx* ctx, int store, void* F, int n, int HW, int C, const float* lin, unsigned* smax, const float* sc);
int gi_debug_lpips_scale(gi_ctx* ctx, const unsigned* smax, float* sc, int n);
int gi_debug_lpips_act_bwd(gi_ctx* ctx, int pool, const void* g, const void* act, const void* seed, void* out, int n, int H, int W,
                           int C, int relu);
int gi_debug_lpips_conv1_adjoint(gi_ctx* ctx, const void* D, const float* wA, const float* sc_inv, float gscale, float* dimg, int n,
                                 int H, int W);
/* fp32 master [a][16][b] -> T [a][16*b] (w_packed) and T [4][b][4*a] (w_phase); either may be NULL */
int gi_pack_weights(gi_ctx* ctx, int dtype, const float* w, int ca, int cb, void* w_packed, void* w_phase);
int gi_convert(gi_ctx* ctx, int dtype, const float* src, void* dst, int64_t count);      /* fp32 -> T */
int gi_convert_back(gi_ctx* ctx, int dtype, const void* src, float* dst, int64_t count); /* T -> fp32 */

/* time the dominant kernel `iters` times with hipEvents on the context stream; returns average
 * milliseconds per launch in *ms_out (used by bench.py for the roofline object) */
int gi_time_convT_s2(gi_ctx* ctx, int dtype, const void* in, const void* w_phase, void* out, int n, int H,
                     int W, int ca, int ldin, int cb, int ldout, int iters, float* ms_out_host);
int gi_time_conv_s2(gi_ctx* ctx, int dtype, const void* in, const void* w_packed, void* out, int n, int H, int W,
                    int cb, int ldin, int ca, int ldout, int iters, float* ms_out_host);   /* the same for gi_conv_s2_forward */

#ifdef __cplusplus
}
#endif
#endif /* GANINPAINT_H */
