// What the VGG-19 losses (vgg.hip) and VGG-16 LPIPS (lpips.hip) share (vggtrunk.hip): a trunk of 3x3 / s1 / p1 convolutions + ReLU with
// 2x2 max pools between, NHWC fp16, and its input-gradient chain on s * gradient. The first-layer forward kernels, the taps' own terms and
// seeds and the two forward runners stay in the networks' files.
#pragma once
#include "common.h"

constexpr int VGGTRUNK_MAXCONV = 13;

// workspace carve-up in 256-byte granules; base == nullptr: the sizes alone (off ends as the bytes needed)
struct WsTake {
  char* base;
  int64_t off;
  char* operator()(int64_t bytes) {
    char* p = base ? base + off : nullptr;
    off += gi_align_up(bytes, 256);
    return p;
  }
};

// A trunk and the state of its backward. The tables belong to the network's file; the first convolution (3 -> 64 on a grey image) is the
// network's own kernel, the backward needs only its fp32 weights per output channel and tap.
struct VggTrunk {
  int nconv;
  const int *cin, *cout;        // [nconv]
  const int* tap_after;         // [nconv] tap index after conv i, or -1
  const int* pool_after;        // [nconv] a 2x2 max pool follows conv i
  int H, W, max_pairs;
  half_t* ga[VGGTRUNK_MAXCONV];      // post-ReLU maps of the grad forward, [first half | second half] of the 2n stacked images; the second half
                                     // survives only at the taps, where the seeds replace it
  half_t* gpool[VGGTRUNK_MAXCONV];   // 2x2 max pool of the pooled layers (both halves): the next layer's input
  half_t* wT[VGGTRUNK_MAXCONV];      // [1..nconv) fp16 weights of the transposed convolutions: [cin][reversed tap][cout]
  half_t* gbuf[2];                   // gradient ping-pong (n images)
  float* w1;                         // first layer [64][9] fp32: VGG-19 the weights summed over the input channel, LPIPS the folded image plane wA
  const float* inv;                  // 1 / s of image i at inv[i * inv_stride]: one scale for the batch (stride 0) or one per image (stride 1)
  int inv_stride;
};

// ---- host launch code: one copy of every grid rule, shared by the network runners and the gi_debug_vgg_* / gi_debug_lpips_* entries ----

// fp32 master weights [cout][cin][3][3] -> what the mode-2 kernels read: fp16 [cout][tap][cin], or (transposed) [cin][8 - tap][cout]
int pack3x3(hipStream_t st, bool transposed, const float* w, half_t* out, int cout, int cin);
// one 3x3 / s1 / p1 convolution on the mode-2 kernels; mask (with the optional addend): the ReLU mask of the result's layer in the
// epilogue, where the dispatched kernel has one. `a` returns pool_applied / mask_applied. GI_ERR_UNSUPPORTED (no kernel serves the
// shape) comes back without a message: the caller reports the shape.
int conv3x3(hipStream_t st, const half_t* in, const half_t* w, half_t* out, int nimg, int H, int W, int cin, int cout, const float* bias, int act_out,
            int pool2, const half_t* mask, const half_t* add, IgemmArgs& a);
int maxpool2(hipStream_t st, const half_t* in, half_t* out, int nimg, int Ho, int Wo, int C);
// NHWC fp16 -> NCHW fp32, plain and times the image's 1 / s
int nhwc_to_nchw(hipStream_t st, const half_t* in, float* out, int nimg, int HW, int C);
int nhwc_to_nchw_unscale(hipStream_t st, const half_t* in, const float* inv, int inv_stride, float* out, int nimg, int HW, int C);
// sc[i] = s_i, sc[n + i] = 1 / s_i from the largest |seed| smax[i] (bit patterns) of n images, or of the whole batch (n = 1)
int seed_scale(hipStream_t st, const unsigned* smax, float* sc, int n);
// out = [act > 0] * (g + seed); pool: g lives on the (H/2, W/2) grid and is routed to each window's first maximum of act
int act_bwd(hipStream_t st, bool pool, const half_t* g, const half_t* act, const half_t* seed, half_t* out, int n, int H, int W, int C, int relu);
// dimg[i] = gscale * inv[i * inv_stride] * (adjoint of the first convolution applied to D [n][H][W][64])
int conv1_adjoint(hipStream_t st, const half_t* D, const float* w1, const float* inv, int inv_stride, float gscale, float* dimg, int n, int H, int W);

// ga / gpool (two arenas), wT and gbuf from `take`, for the trunk's H, W and max_pairs
void trunk_gws_layout(VggTrunk& t, WsTake& take);
// The chain from the top convolution down, from what the grad forward and the seed passes left in ga. stop < 0: down to the first layer,
// then its adjoint into grad_out. stop = L: the gradient w.r.t. the post-ReLU map of layer L goes to layer_out as NCHW fp32, de-scaled.
int trunk_backward(const VggTrunk& t, hipStream_t st, int n, int stop, float* layer_out, float* grad_out, float gscale);
