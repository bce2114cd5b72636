/*
 * phendiff_hip.h -- C ABI of libphendiff_hip.so (MI355X / gfx950).
 *
 * The reference (thethomasboyer/PhenDiff) has no FFI of its own: its hot path is Python calling
 * diffusers-0.18.2 modules which dispatch to ATen/cuDNN kernels.  Each entry point below replaces
 * the device work of one such call site; the Python host (phendiff_amd/ *.py) mirrors the reference's
 * object protocol on top of this ABI and INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every pd_<op>() returns 0 on success, a negative pd_status on failure; pd_last_error() gives
 *     the thread-local message.  No exceptions, no allocation, no host sync inside: all launches are
 *     asynchronous on `stream` (a hipStream_t passed as void*) and are hipGraph-capturable.
 *   - all pointers are caller-owned DEVICE pointers (the host takes them from live torch tensors).
 *   - activations are NHWC (channel-contiguous) in `dtype` (PD_F32 or PD_BF16); the model boundary
 *     tensors (UNet input sample / output prediction, scheduler state) are NCHW fp32 exactly as the
 *     reference's tensors are.
 *   - conv / linear weights are passed PRE-PACKED in the MFMA fragment order produced by
 *     phendiff_amd/packing.py (documented at pd_conv_args.w_packed).
 */
#ifndef PHENDIFF_HIP_H_
#define PHENDIFF_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an args struct grows or an entry point is added (a caller built against an older header passes shorter
 * structs): 1 = round 1; 2 = round 2's trailing fields (pd_gn_finalize_args.temb/temb_stride, pd_attn_args.kmax2,
 * pd_linear_args.kmax2_out), PD_F16 and pd_zero / pd_gn_apply / pd_attn_wide; 3 = round 3; 4 = round 4 (pd_comm_query, pd_linear_args.fold_ws /
 * fold_ws_bytes + pd_linear_fold_workspace,
 * pd_conv_args.phase); 5 = pd_conv_args.phase_in, pd_wgrad_args.phase; 6 = round 5: pd_attn_bwd_args.slab / slab_bytes +
 * pd_attn_d8_bwd_workspace (the one-pass backward); 7 = round 6: pd_gn_bwd_args.mod / mod_stride / dmod (scale_shift ResNet blocks train);
 * pd_resize_tf1, pd_conv_rect, pd_pool2d, pd_fc_f32 (the evaluation metrics' feature extractor); pd_pack_weight_args.dst2 / dst2_ct_stride;
 * 8 = pd_geglu_bwd_args.sums / sum_splits / B, pd_layernorm_bwd_args.dxsum (bias gradients without a pass over dY), pd_upsample_phase_weights,
 * pd_token_wgrad_args.stage / pd_wgrad_args.stage.  Entry points added since without a change to any existing struct keep 8 (a caller built
 * against the older header passes nothing shorter): pd_latent_chain_bwd, pd_image_preprocess, pd_attn_hd_bwd, pd_train_sample, pd_sample_stats
 * (+ pd_sample_stats_workspace), pd_kid_mmd (+ pd_kid_mmd_workspace), pd_feature_moments (+ pd_feature_moments_workspace), pd_lp_guidance_scaled, pd_guided_step
 * (+ pd_guided_step_args), pd_image_preprocess_bands (+ pd_image_preprocess_bands_args), pd_image_preprocess_bands16, pd_band_histogram16,
 * pd_postproc_bands16 (+ their args structs), pd_abs_quantile (+ pd_abs_quantile_workspace), pd_ddim_raw_x0, pd_ddim_step_threshold (+ their
 * args structs), pd_tile_gather, pd_tile_blend (+ their args structs), pd_ssim (+ pd_ssim_args, pd_ssim_workspace),
 * pd_knn_radii (+ pd_knn_radii_args, pd_knn_radii_workspace), pd_manifold_query (+ pd_manifold_query_args, pd_manifold_query_workspace),
 * pd_stream_noise (+ pd_stream_noise_args), pd_stream_advance, pd_multistep_step (+ pd_multistep_step_args), pd_guidance_rescale
 * (+ pd_guidance_rescale_args, pd_guidance_rescale_workspace), pd_class_contrast, pd_contrast_mask, pd_mask_blend (+ their args structs,
 * pd_contrast_mask_workspace), pd_mask_distance, pd_mask_morph, pd_mask_components, pd_mask_filter (+ their args structs,
 * pd_mask_morph_workspace, pd_mask_components_workspace), pd_object_index, pd_object_geometry, pd_object_intensity (+ their args structs,
 * pd_object_index_workspace). */
#define PD_ABI_VERSION 8

typedef enum { PD_OK = 0, PD_ERR_ARG = -1, PD_ERR_SHAPE = -2, PD_ERR_LAUNCH = -3, PD_ERR_UNSUPPORTED = -4 } pd_status;
/* PD_F32: exact-fp32 MFMA (parity mode).  PD_BF16 / PD_F16: 16-bit storage + MFMA, fp32 accumulate / statistics / softmax.
 * PD_F16 is the reference's `--mixed_precision fp16` (args_parser.py:381-390): every inference entry point, and -- since round 5 -- the
 * pixel UNet's backward set (pd_conv_wgrad, pd_gn_silu_bwd, pd_attn_d8_bwd + pd_attn_d8's lse, pd_pool2x2_sum, pd_channel_sum, pd_im2col3,
 * pd_token_wgrad) and the latent-diffusion backward set (pd_attn_d64_bwd + pd_attn_d64's lse, pd_attn_wide_bwd, pd_layernorm_bwd,
 * pd_geglu_bwd, pd_token_embedding_grad) under a loss scale (pd_loss_args.grad_scale; phendiff_amd.training.LossScaler = accelerate's
 * GradScaler): UNetTrainer and SDUNetTrainer both train in fp16. */
typedef enum { PD_F32 = 0, PD_BF16 = 1, PD_F16 = 2 } pd_dtype;
typedef enum { PD_PRED_EPSILON = 0, PD_PRED_SAMPLE = 1, PD_PRED_V = 2 } pd_pred_type;

int pd_abi_version(void);
const char* pd_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * pd_temb: timestep + class embedding and every ResnetBlock2D's time_emb_proj in one launch.
 * Replaces cond_unet_2d.py:289-309 (Timesteps -> TimestepEmbedding -> +class embedding) and the
 * `time_emb_proj(SiLU(temb))` Linear of all ResnetBlock2D instances (diffusers resnet.py; reached via
 * cond_unet_2d.py:171,187,217).  One output row per (timestep, class) pair, so a whole sampling
 * trajectory (S steps x B images) is one call.
 *   emb[r]  = W2 . silu(W1 . sincos(t[r]) + b1) + b2 + (class_emb[r] | E[label[r]] | 0)
 *   proj[r] = Wp . silu(emb[r]) + bp            (Wp = all time_emb_proj stacked: [proj_dim][T])
 */
typedef struct {
  int rows;                 /* number of (timestep, class) rows */
  int c0;                   /* block_out_channels[0] (sinusoid width) */
  int tdim;                 /* time_embed_dim = 4*c0 */
  int proj_dim;             /* sum of all resnet out_channels */
  int flip_sin_to_cos;      /* cond_unet_2d.py:139 */
  float freq_shift;         /* downscale_freq_shift */
  int num_classes;          /* rows of class table (0: no class embedding) */
  const float* timesteps;   /* [rows] fp32 (integer-valued) */
  const int64_t* labels;    /* [rows] or NULL */
  const float* class_emb;   /* [rows][tdim] or NULL (zeros => unconditional, cond_unet_2d.py:306-309) */
  /* all Linear weights are passed TRANSPOSED ([in][out], i.e. weight.t().contiguous()) so thread `out` streams coalesced */
  const float* w1; const float* b1;   /* time_embedding.linear_1^T [c0][tdim], [tdim] */
  const float* w2; const float* b2;   /* time_embedding.linear_2^T [tdim][tdim], [tdim] */
  const float* class_table;           /* class_embedding.weight [num_classes][tdim] or NULL */
  const float* wp; const float* bp;   /* stacked time_emb_proj^T [tdim][proj_dim], [proj_dim] */
  float* emb;               /* out [rows][tdim] (may be NULL) */
  float* proj;              /* out [rows][proj_dim] */
  float* feat;              /* optional out [rows][c0]: the sinusoid features (kept for the backward), or NULL */
  float* z1;                /* optional out [rows][tdim]: linear_1's pre-activation (kept for the backward), or NULL */
} pd_temb_args;
int pd_temb(const pd_temb_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_conv_in: first 3x3 conv (cond_unet_2d.py:127-129,313): NCHW fp32 sample -> NHWC activations.
 */
typedef struct {
  int dtype;                /* output activation dtype */
  int B, H, W, Cin, Cout;   /* Cin <= 4, Cout % 32 == 0 */
  const float* x;           /* [B][Cin][H][W] fp32 */
  const float* w;           /* [Cout][Cin][3][3] fp32 (OIHW, unpacked) */
  const float* bias;        /* [Cout] */
  void* y;                  /* [B][H][W][Cout] */
} pd_conv_in_args;
int pd_conv_in(const pd_conv_in_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_gn_stats: GroupNorm statistics folded with the affine parameters into per-(sample, channel)
 * scale/shift, so that the consumer conv applies y = x*scale + shift (+SiLU) while staging its tile.
 * Replaces the statistics half of torch.nn.GroupNorm(32, C) as used by ResnetBlock2D.norm1/norm2,
 * Attention.group_norm and conv_norm_out (cond_unet_2d.py:175,195,221,236).  The input may be the
 * channel concatenation [x0 | x1] of two NHWC tensors (skip connections, cond_unet_2d.py:333-343),
 * (statistics are invariant under the nearest x2 upsample, so Upsample2D needs no flag here).
 * Two launches: partial sums (fp64 combine) and finalize.  Standalone form (one extra read of the tensor); the UNet
 * plan uses the fused form instead: pd_conv(stats_out) in the producer + pd_gn_finalize.
 */
typedef struct {
  int dtype;
  int B, HW;                /* pixels per sample */
  int C0, C1;               /* channels of source 0 / source 1 (C1 = 0: single source) */
  int groups;               /* 32 */
  float eps;
  const void* x0; const void* x1;
  const float* gamma; const float* beta;   /* [C0+C1] */
  double* partial;          /* workspace [B][splits][C0+C1][2] */
  int splits;               /* partial blocks per (sample, group); >= 1 */
  float* scale; float* shift;   /* out [B][C0+C1] */
} pd_gn_stats_args;
int pd_gn_stats(const pd_gn_stats_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_conv: implicit-GEMM convolution on MFMA (NHWC, LDS-staged halo tiles).
 * Replaces torch.nn.Conv2d 3x3 (ResnetBlock2D.conv1/conv2, Downsample2D.conv, Upsample2D.conv,
 * conv_out) and 1x1 / Linear (ResnetBlock2D.conv_shortcut, Attention.to_q/k/v/to_out) together with the
 * elementwise ops around them in diffusers' ResnetBlock2D.forward / AttnProcessor2_0:
 *   prologue : x <- silu?(x*scale + shift)    (GroupNorm apply + SiLU), zero padding AFTER the transform
 *              optional nearest x2 upsample of the source (Upsample2D: F.interpolate never materialised)
 *              optional channel concat of two sources (torch.cat([h, skip], 1) never materialised)
 *   epilogue : + bias[co] + temb[n][co] + residual[n][y][x][co]
 * w_packed layout (T = dtype element): [Cout/32][Cin/32][taps][2][64 lanes][8] where for lane l
 * (r = l & 31, h = l >> 5) element j is W[co = 32*ct + r][ci = 32*chunk + 16*s + 8*h + j][tap].
 */
typedef enum { PD_OUT_NHWC = 0, PD_OUT_NCHW_F32 = 1, PD_OUT_QKV_HEADS = 2 } pd_out_mode;
typedef struct {
  int dtype;
  int B, Hin, Win;          /* source spatial size (before upsample) */
  int Hout, Wout;           /* output spatial size (checked against the conv arithmetic) */
  int C0, C1;               /* source channels; Cin = C0 + C1, each % 32 == 0 */
  int Cout;                 /* logical output channels */
  int Cout_pad;             /* packed output channels, % 32 == 0 (>= Cout) */
  int ksize;                /* 1 or 3 */
  int stride;               /* 1 or 2 (3x3 only) */
  int pad;                  /* 1 for 3x3 pad 1; 0 for 1x1 or the asymmetric (0,1,0,1) downsample */
  int upsample;             /* 1: nearest x2 before the conv (Upsample2D); 2: zero-stuffed x2, samples at the even positions (input
                               gradient of a stride-2 pad-1 conv); 3: zero-stuffed x2, samples at the odd positions (input gradient of
                               Downsample2D(padding=0): pad (0,1,0,1) then an unpadded stride-2 conv) */
  int silu;                 /* 1: SiLU after the affine */
  int out_mode;             /* pd_out_mode */
  int heads;                /* PD_OUT_QKV_HEADS: number of heads (Cout = 3*heads*8) */
  const void* x0; const void* x1;
  const float* scale; const float* shift;   /* [B][Cin] or NULL (no GroupNorm) */
  const void* w_packed;
  const float* bias;        /* [Cout_pad] */
  const float* temb; int temb_stride;       /* temb[n*temb_stride + co] or NULL */
  const void* residual;     /* NHWC [B][Hout][Wout][Cout] or NULL */
  void* y;
  float* stats_out;         /* NULL, or [B][pd_conv_stat_tiles()][Cout][2]: per-tile per-channel (sum, sum of squares) of the
                               stored output -- the GroupNorm statistics of the CONSUMER, produced for free here */
  /* Fused 1x1 "tail" (ResnetBlock2D.conv_shortcut folded into conv2): y += Wt . [tail_x0 | tail_x1] on the same pixels
     (no GroupNorm / SiLU on the tail).  3x3 stride-1 convs only; the tail's weight fragments follow the main ones in
     w_packed: per 32-co tile [main: (C0+C1)/32 * 9 * 2 fragments][tail: (tail_C0+tail_C1)/32 * 2 fragments]; `bias` is
     the sum of both biases.  tail_x0 = NULL: no tail. */
  const void* tail_x0; const void* tail_x1; int tail_C0, tail_C1;
  int im2col3;              /* 0, or n <= 3: x0 is an NCHW fp32 tensor with n channels (the UNet input sample) and the op is
                               the 3x3 pad-1 conv_in run as a 1x1 conv over 32 virtual channels k = ci*9 + ky*3 + kx
                               (ksize must be 1, C0 = 32, weights packed accordingly) */
  int phase;                /* (ABI 4) 0: ordinary convolution.  1 + 2 a + b (a, b = 0 or 1): one PHASE of the sub-pixel form of Upsample2D
                               (F.interpolate(x, 2.0, "nearest") then conv 3x3 pad 1, diffusers resnet.py; cond_unet_2d.py:200-228): output
                               pixel (2 oy + a, 2 ox + b) of the y tensor [B][2 Hout][2 Wout][Cout] = sum over dy, dx = 0, 1 of
                               W_ab[dy][dx] . x[oy - (1 - a) + dy][ox - (1 - b) + dx] (zero outside the image), W_ab = the 3x3 taps that
                               fall on the same source pixel summed (4 of the 9 tap positions per output pixel: 4 / 9 of the FLOPs).
                               Requires ksize = 2, stride 1, no upsample / GroupNorm / tail / residual, NHWC output, Hout = Hin,
                               Wout = Win; `pad` is ignored.  stats_out is then [B][4 T][Cout][2], T = pd_conv_stat_tiles(Hout, Wout, 2, 1):
                               phase p's tiles fill slots (p - 1) T .. p T - 1 */
  int phase_in;             /* (ABI 5) with phase = 1 + 2 a + b: the phase selects INPUT pixels instead of output pixels -- the input
                               gradient of a sub-pixel phase: x0 is [B][2 Hin][2 Win][C0] (the gradient of the upsampled output), the
                               launch reads its pixels (2 iy + a, 2 ix + b) and writes the dense y [B][Hout][Wout][Cout], Hout = Hin,
                               Wout = Win: y[oy][ox] (+= residual) = sum over dy, dx = 0, 1 of W[dy][dx] . x0[2 (oy - a + dy) + a][2 (ox - b + dx) + b]
                               (W = the phase's 2x2 weights packed as input-gradient weights: transposed, taps flipped).  residual is
                               allowed (the four phases accumulate into one gradient tensor); no stats_out */
} pd_conv_args;
int pd_conv(const pd_conv_args* a, void* stream);
/* number of statistic tiles per sample pd_conv writes for this shape (depends on the kernel's tile choice) */
int pd_conv_stat_tiles(int Hout, int Wout, int ksize, int stride);

/* pd_gn_finalize: per-tile channel sums (pd_conv stats_out) of one or two tensors (channel concat [x0 | x1]) ->
 * GroupNorm scale/shift per (sample, channel):  scale = rstd*gamma, shift = beta - mean*rstd*gamma  (fp64 combine). */
typedef struct {
  int B, HW, groups; float eps;
  int C0, T0; const float* stats0;     /* [B][T0][C0][2] */
  int C1, T1; const float* stats1;     /* [B][T1][C1][2] or NULL (C1 = 0) */
  const float* gamma; const float* beta;
  float* scale; float* shift;          /* out [B][C0+C1] */
  float* mean; float* rstd;            /* optional out [B][groups] (kept for the backward, pd_gn_silu_bwd), or NULL */
  const float* temb; int temb_stride;  /* optional: ResnetBlock2D time_embedding_norm = "scale_shift" (cond_unet_2d.py:103,180):
                                          row n = temb + n*temb_stride holds [scale | shift] (2*(C0+C1) floats, this resnet's
                                          time_emb_proj(SiLU(emb))); the written affine becomes GN(x)*(1 + scale) + shift */
} pd_gn_finalize_args;
int pd_gn_finalize(const pd_gn_finalize_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_attn_d8: softmax(q k^T / sqrt(8)) v for head_dim 8 (attention_head_dim=8, cond_unet_2d.py:176-178),
 * streaming (flash-style) softmax, scores never materialised.  Replaces F.scaled_dot_product_attention in
 * AttnProcessor2_0.  Inputs come head-major from pd_conv(out_mode = PD_OUT_QKV_HEADS):
 *   q, k : [B][heads][N][8]     v : [B][heads][N][8]     out: NHWC [B][N][heads*8]
 */
typedef struct {
  int dtype;
  int B, heads, N;
  const void* q; const void* k; const void* v;
  void* out;
  float* lse;   /* optional out [B][heads][N]: log2-domain log-sum-exp of the scaled scores (kept for pd_attn_d8_bwd), or NULL */
  const float* kmax2;   /* optional [B][heads]: an upper bound of max_n |k[b][head][n]|^2 over the keys as stored (pd_linear
                           kmax2_out produces it in the q/k/v projection's epilogue), or NULL.  With it (bf16 / fp16, large
                           launches) the kernel needs no per-tile key norms: K / V tiles go global -> LDS by DMA
                           (global_load_lds), V^T fragments come from transposed LDS reads.  Results are the same function
                           of the inputs either way (softmax is invariant to the running reference maximum) PROVIDED the
                           bound holds: kmax2[b][head] >= max_n |k|^2 of THIS launch's keys is a hard precondition (a slot
                           that is too small lets p = 2^(s - m) grow without the rescale: inf / NaN in fp16).  A first
                           32-key score above the implied bound makes the wave fall back to the exact running-maximum
                           path -- a safety net for zero / stale slots, not a substitute for the precondition. */
} pd_attn_args;
int pd_attn_d8(const pd_attn_args* a, void* stream);

/* pd_attn_d8_bwd: gradient of pd_attn_d8 (autograd of F.scaled_dot_product_attention), P recomputed from lse.
 *   q, k, v: as the forward;  o: the forward's output, dout: gradient w.r.t. it (both NHWC [B][N][heads*8]);
 *   delta: workspace [B][heads][N];  dqkv: out NHWC [B][N][3*heads*8] = [dq | dk | dv] (channel = which*C + head*8 + d),
 *   the output-gradient layout of the fused q/k/v projection. */
typedef struct {
  int dtype;
  int B, heads, N;
  const void* q; const void* k; const void* v;
  const void* o; const void* dout;
  const float* lse; float* delta;
  void* dqkv;
  float* slab;              /* (ABI 6) NULL, or a device workspace of >= pd_attn_d8_bwd_workspace(a) bytes (when that is > 0): the backward then runs
                               in ONE pass -- P and dS formed once per tile, dK / dV lane-local, dS transposed through LDS for dQ, whose
                               partial sums per 512-key block land here [key blocks][B][heads][N][8] fp32 and are added in order by a
                               small reduce launch (bit-identical run to run).  16-bit engines, N >= 512; otherwise the two-kernel path */
  size_t slab_bytes;
} pd_attn_bwd_args;
int pd_attn_d8_bwd(const pd_attn_bwd_args* a, void* stream);
/* bytes of pd_attn_bwd_args.slab the one-pass backward needs for this shape; 0: not applicable (fp32 engine, N < 512) */
size_t pd_attn_d8_bwd_workspace(const pd_attn_bwd_args* a);

/* ------------------------------------------------------------------------------------------------
 * pd_ddim_step: one fused DDIM / inverse-DDIM update on NCHW fp32 tensors.
 * Replaces DDIMScheduler.step (pipeline_conditionial_ddim.py:340-347) and DDIMInverseScheduler.step
 * (utils_Img2Img.py:794-798): both are  x' = sqrt_ap * clamp(x0) + dir_coef * eps  with
 *   epsilon: x0 = (x - sqrt_b*out)/sqrt_a, eps = out        sample: x0 = out, eps = (x - sqrt_a*x0)/sqrt_b
 *   v:       x0 = sqrt_a*x - sqrt_b*out,   eps = sqrt_a*out + sqrt_b*x
 * The host passes the four coefficients (computed in fp32 exactly as the reference's 0-dim tensors).
 * Optional classifier-free-guidance combine (pipeline_conditionial_ddim.py:324-328):
 *   out = uncond + w*(out - uncond)  [imagen]   or   out + w*(out - uncond)  [CFG]
 * Refused before any launch (PD_ERR_ARG): null args / sample / model_out / prev_sample, numel < 1, per_sample < 1 or not a divisor of
 * numel (the kernel divides by it), a prediction type outside the three, guidance without weights, tensors that are not 16-byte aligned.
 */
typedef struct {
  int64_t numel;            /* B*C*H*W */
  int64_t per_sample;       /* C*H*W (for per-sample guidance weights) */
  int pred_type;            /* pd_pred_type */
  int clip;                 /* clip_sample */
  float clip_range;
  int use_clipped_model_output;
  float sqrt_a, sqrt_b;     /* sqrt(alpha_prod_t), sqrt(1 - alpha_prod_t) */
  float sqrt_ap, dir_coef;  /* sqrt(alpha_prod_t_prev), sqrt(1 - alpha_prod_t_prev - sigma^2) */
  const float* sample;      /* x_t */
  const float* model_out;   /* conditional prediction */
  const float* uncond_out;  /* NULL: no guidance */
  const float* w;           /* guidance weights: [B] or 1 value */
  int w_per_sample;         /* 1: w has one value per sample */
  int guidance_cfg;         /* 0: imagen eqn, 1: CFG eqn */
  float* prev_sample;       /* out (may alias sample) */
  float* pred_x0;           /* out or NULL */
} pd_ddim_step_args;
int pd_ddim_step(const pd_ddim_step_args* a, void* stream);

/* pd_add_noise: sa[n]*x + sb[n]*noise (DDIMScheduler.add_noise) or velocity sa*noise - sb*x. */
typedef struct {
  int64_t numel, per_sample;
  int velocity;
  const float* x; const float* noise;
  const float* sa; const float* sb;   /* [B] per-sample coefficients (device) */
  float* out;
} pd_add_noise_args;
int pd_add_noise(const pd_add_noise_args* a, void* stream);

/* pd_zero: hipMemsetAsync(ptr, 0, bytes) on the stream -- a launch plan's way to reset what later launches max / add into
 * (pd_linear kmax2_out); captured into a hipGraph like every other entry point. */
typedef struct { void* ptr; size_t bytes; } pd_zero_args;
int pd_zero(const pd_zero_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_postproc: (x/2 + 0.5).clamp(0,1), NCHW -> NHWC (pipeline_conditionial_ddim.py:349-350), optionally
 * also the uint8 quantisation round(255*x) of DiffusionPipeline.numpy_to_pil.
 */
typedef struct {
  int B, C, H, W;
  const float* x;           /* NCHW */
  float* out_f32;           /* NHWC or NULL */
  uint8_t* out_u8;          /* NHWC or NULL */
} pd_postproc_args;
int pd_postproc(const pd_postproc_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * UNet backward building blocks (autograd of the forward above, utils_training.py:436).
 * Input gradients of convolutions reuse pd_conv with W'[ci][co][ky][kx] = W[co][ci][K-1-ky][K-1-kx] (stride-2 convs: upsample = 2,
 * zero-stuffed dY; the conv fused with Upsample2D: pd_conv at 2x resolution followed by pd_pool2x2_sum).
 *
 * pd_gn_silu_bwd: gradient through z = silu?(GroupNorm(x)) of [x0 | x1]:  dz -> dx (per source, = or +=), dgamma += , dbeta += .
 *   dy = dz * silu'(gamma*xhat + beta);  dx = rstd * (gamma*dy - mean_g(gamma*dy) - xhat * mean_g(gamma*dy*xhat))
 */
typedef struct {
  int dtype;
  int B, HW, C0, C1, groups, silu;
  const void* x0; const void* x1;        /* forward inputs of the norm (NHWC) */
  const void* dz0; const void* dz1;      /* gradient w.r.t. the normalised (+SiLU) tensor, same split */
  const float* mean; const float* rstd;  /* [B][groups] from pd_gn_finalize */
  const float* gamma; const float* beta; /* [C0+C1] */
  double* partial; int splits;           /* workspace [B][splits][C0+C1][2] */
  float* coef;                           /* workspace [B][groups][2] */
  void* dx0; void* dx1;                  /* outputs (either may be NULL) */
  int accumulate0, accumulate1;          /* 1: dx += */
  float* dgamma; float* dbeta;           /* [C0+C1], accumulated (+=), or NULL */
  int dz_combined;                       /* 1: dz0 holds all C0+C1 channels (stride C0+C1), dz1 must be NULL */
  const void* res;                       /* optional [B][HW][C0+C1]: added to dx (gradient of the skip / shortcut around the block) */
  float* sum0; float* sum1;              /* optional out [B][splits][C0] / [B][splits][C1]: per-channel sums of the dx0 / dx1 values
                                            this call stores (feeds pd_channel_sum with x = NULL: the producer's bias /
                                            time-embedding gradients without another pass over dx) */
  /* (ABI 7) resnet_time_scale_shift = "scale_shift" (cond_unet_2d.py:180,191,225; diffusers ResnetBlock2D: h = norm2(h) * (1 + scale)
   * + shift with [scale | shift] = time_emb_proj(silu(temb))): the norm's affine is modulated per sample,
   *   gamma_n = gamma (1 + scale_n),  beta_n = beta (1 + scale_n) + shift_n,
   * mod = the forward's projection rows, row n at mod + n * mod_stride holding [scale (C) | shift (C)] (C1 must be 0).  dgamma / dbeta
   * then accumulate sum_n (1 + scale_n) x the per-sample sums, and dmod (same row layout, written "=") receives
   *   d scale_n = gamma * sum(dy xhat) + beta * sum(dy),   d shift_n = sum(dy). */
  const float* mod; int mod_stride; float* dmod;
} pd_gn_bwd_args;
int pd_gn_silu_bwd(const pd_gn_bwd_args* a, void* stream);

/* pd_pool2x2_sum: dx[n][y][x][c] (+)= sum of du[n][2y..2y+1][2x..2x+1][c]  (gradient of F.interpolate(scale_factor=2, "nearest")) */
typedef struct { int dtype; int B, H, W, C; const void* du; void* dx; int accumulate; } pd_pool2x2_args;
int pd_pool2x2_sum(const pd_pool2x2_args* a, void* stream);

/* pd_channel_sum: out[n*out_stride + c] (+)= sum over pixels of x[n][p][c]  (bias gradients after a sum over n; d temb_proj) */
typedef struct {
  int dtype; int B, HW, C; const void* x; float* out; int out_stride; int accumulate;
  float* total; int total_valid;   /* optional [total_valid <= C]: total[c] += sum over samples of this call's per-sample sums */
  float* workspace; int splits;    /* optional [B][splits][C] scratch: the pixels of a sample are split over `splits` workgroups;
                                      with x = NULL it already holds the per-split sums (pd_gn_silu_bwd sum0 / sum1) */
} pd_channel_sum_args;
int pd_channel_sum(const pd_channel_sum_args* a, void* stream);

/* pd_nchw_to_nhwc: out[n][p][c] = c < C ? x[n][c][p] : 0 for c < Cpad (the loss gradient w.r.t. the UNet output, NCHW fp32,
 * as conv_out's NHWC output gradient). */
typedef struct { int dtype; int B, C, HW, Cpad; const float* x; void* out; } pd_nchw_to_nhwc_args;
int pd_nchw_to_nhwc(const pd_nchw_to_nhwc_args* a, void* stream);

/* Backward of the fp32 Linear layers of the time-embedding path (TimestepEmbedding, class embedding, time_emb_proj):
 *   pd_linear_wgrad:  dw[o][i] += sum_r dy[r][o] * act(x[r][i]);  db[o] += sum_r dy[r][o]      (act = SiLU when x_silu)
 *   pd_linear_dgrad:  dx[r][i]  = (sum_o dy[r][o] * w[o][i]) * (pre ? silu'(pre[r][i]) : 1)       (w: nn.Linear layout [out][in])
 *   pd_embedding_grad: dtable[k][i] += sum over rows with labels[r] == k of d[r][i]                (deterministic order)  */
typedef struct { int rows, in_dim, out_dim, x_silu; const float* dy; const float* x; float* dw; float* db; } pd_linear_wgrad_args;
int pd_linear_wgrad(const pd_linear_wgrad_args* a, void* stream);
typedef struct { int rows, in_dim, out_dim; const float* dy; const float* w; const float* pre; float* dx; } pd_linear_dgrad_args;
int pd_linear_dgrad(const pd_linear_dgrad_args* a, void* stream);
typedef struct { int rows, dim, num_classes; const int64_t* labels; const float* d; float* dtable; } pd_embedding_grad_args;
int pd_embedding_grad(const pd_embedding_grad_args* a, void* stream);

/* pd_conv_wgrad: weight gradient of a convolution pd_conv ran in the forward:
 *   dw[co][ci][ky][kx] (+)= sum_{n,oy,ox} dy[n][oy][ox][co] * Z[n][oy*stride+ky-pad][ox*stride+kx-pad][ci],
 * Z = silu?(scale*[x0|x1] + shift) (optionally nearest-x2 upsampled) rebuilt on the fly exactly as pd_conv's staging does.
 * B/Hin/.../pad/upsample/silu/x0/x1/scale/shift have pd_conv's meaning (upsample: 0 or 1).  dy is NHWC with channel stride
 * Cout (multiple of 8); dw is the fp32 OIHW gradient [Cout_valid][Cin_valid][k][k] (Cout_valid/Cin_valid = 0: all channels).
 * slab: workspace of slab_bytes >= pd_conv_wgrad_workspace(a) (smaller is accepted down to one split, at lower occupancy);
 * the partial sums are reduced in a fixed order: results are bitwise reproducible. */
typedef struct {
  int dtype;
  int B, Hin, Win, Hout, Wout;
  int C0, C1, Cout;
  int ksize, stride, pad, upsample, silu;
  const void* x0; const void* x1;
  const float* scale; const float* shift;
  const void* dy;
  float* slab; size_t slab_bytes;
  float* dw; int Cout_valid, Cin_valid; int accumulate;
  int phase;                /* (ABI 5) 0: ordinary.  1 + 2 a + b: the weight gradient THROUGH sub-pixel phase (a, b) of an upsampler's 3x3 convolution
                               (pd_conv_args.phase): ksize = 2, x0 = the LOW-resolution input [B][Hin][Win][C0], dy = the gradient of the upsampled
                               output [B][2 Hout][2 Wout][Cout] (Hout = Hin, Wout = Win) read at its pixels (2 oy + a, 2 ox + b), dw = the 3x3
                               gradient [Cout][C0][3][3]: the phase kernel's tap gradients are added to the 3x3 taps they are sums of (phase 1
                               honours `accumulate`, phases 2-4 always add: run the four in order).  4 / 9 of the FLOPs of upsample = 1. */
  int stage;                /* (ABI 8) 0: both launches; 1: the GEMM only; 2: the fold of the slab into dw only (as pd_token_wgrad_args.stage) */
} pd_wgrad_args;
size_t pd_conv_wgrad_workspace(const pd_wgrad_args* a);
int pd_conv_wgrad(const pd_wgrad_args* a, void* stream);

/* pd_pack_weight: fp32 master weights (nn.Conv2d OIHW / nn.Linear [out][in]) -> pd_conv's packed MFMA fragment order
 * (phendiff_amd/packing.py: pack_conv_weight), on the device, after each optimizer step of a training run.
 *   dgrad = 0: packed[co][ci][tap] = src[co][ci][tap]                   (src rows of src_in input channels)
 *   dgrad = 1: packed[co][ci][tap] = src[ci][co][taps-1-tap]            (input-gradient weights, packing.dgrad_weight)
 * cout/cin: valid packed rows / columns (zero beyond, up to cout_pad / cin_pad); dst_ct_stride: elements between consecutive
 * 32-row tiles of dst (> the tile size when another conv's fragments follow each tile: the fused conv_shortcut). */
typedef struct {
  int dtype;
  int cout, cin, cout_pad, cin_pad, ksize, src_in, dgrad;
  const float* src; void* dst; long long dst_ct_stride;
  /* (ABI 7) optional, dgrad = 0 only: the SAME source blocks also written as the input-gradient packing -- what a second call with
   * dgrad = 1, cout / cin (and their pads) swapped and dst = dst2 would write -- from one read of the fp32 master weights
   * (an optimizer step re-packs every weight both ways: half the re-pack's HBM reads).  dst2_ct_stride: elements between
   * consecutive 32-row (input-channel) tiles of dst2, >= (cout_pad/32) * ksize^2 * 1024. */
  void* dst2; long long dst2_ct_stride;
} pd_pack_weight_args;
int pd_pack_weight(const pd_pack_weight_args* a, void* stream);

/* pd_pack_weight_batch: n pd_pack_weight jobs of ONE dtype as a single launch (an optimizer step re-packs ~130 weights of the
 * pixel UNet, ~1400 of the SD UNet: 13 us of launch latency each).  jobs: DEVICE array of n descriptors (validated by the caller
 * as pd_pack_weight would); starts: DEVICE int[n + 1], starts[j] = sum over i < j of (cout_pad/32)*(cin_pad/32), starts[n] =
 * total_blocks; max_ksize: largest ksize among the jobs (sizes the LDS tile). */
typedef struct {
  int dtype; int n;
  const pd_pack_weight_args* jobs; const int* starts;
  int total_blocks; int max_ksize;
} pd_pack_weight_batch_args;
int pd_pack_weight_batch(const pd_pack_weight_batch_args* a, void* stream);

/* pd_upsample_phase_weights (ABI 8): the four 2x2 sub-pixel phase kernels of "nearest x2, then 3x3 pad-1 convolution" (diffusers Upsample2D,
 * cond_unet_2d.py via UpBlock2D; phendiff_amd.packing.upsample_phase_weights) from the OIHW fp32 master weight, stacked:
 * out[2 a + b][o][i][u][v] = sum_{y in Y_a(u), x in Y_b(v)} w[o][i][y][x],  Y_0 = ({0}, {1, 2}),  Y_1 = ({0, 1}, {2})  -- rows first, then columns,
 * in fp32.  The fine-tuning step refreshes them after every optimizer step (before pd_pack_weight_batch packs them). */
typedef struct { int cout, cin; const float* w; float* out; } pd_upsample_phase_weights_args;
int pd_upsample_phase_weights(const pd_upsample_phase_weights_args* a, void* stream);

/* pd_im2col3: out[n][y][x][ci*9+ky*3+kx] = x[n][ci][y+ky-1][x+kx-1] (zero padded; 27 of 32 channels used): the input of
 * conv_in seen as a 1x1 convolution, for its weight gradient (cond_unet_2d.py:127-129). x: NCHW fp32, C <= 3; out: NHWC dtype. */
typedef struct { int dtype; int B, H, W, C; const float* x; void* out; } pd_im2col3_args;
int pd_im2col3(const pd_im2col3_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training-step building blocks: the fused bandwidth-bound passes around the UNet
 * forward/backward, on flat fp32 buffers.
 *
 * pd_diffusion_loss (utils_training.py:415-433): loss = mean(w_n (out - target)^2) and d loss / d out, with
 *   epsilon: target = noise, w = 1      sample: target = clean, w_n = alpha_t/(1-alpha_t) (SNR weights, `weight`)
 *   v_prediction: target = sa_n*noise - sb_n*clean  (DDIMScheduler.get_velocity)
 * Deterministic two-stage reduction (fp64 partials).
 */
typedef struct {
  int64_t numel, per_sample;
  int pred_type;
  const float* model_out; const float* noise; const float* clean;
  const float* weight;            /* [B] SNR weights (sample prediction) or NULL */
  const float* sa; const float* sb;   /* [B] sqrt(alpha_bar_t), sqrt(1-alpha_bar_t) (v_prediction) or NULL */
  float grad_scale;               /* multiplies d loss / d out (1.0; loss scaling for fp16) */
  float* grad_out;                /* [numel] or NULL */
  double* partial;                /* workspace [1024] */
  float* loss_out;                /* [1] */
} pd_loss_args;
int pd_diffusion_loss(const pd_loss_args* a, void* stream);

/* pd_grad_norm (utils_training.py:438-440, torch.nn.utils.clip_grad_norm_): global L2 norm of a flat gradient buffer and the
 * clip coefficient min(1, max_norm / (norm + 1e-6)), both left on the device (no host sync). partial: workspace [1024]. */
int pd_grad_norm(const float* grad, int64_t numel, double* partial, float max_norm, float* norm_out, float* clip_coef_out, void* stream);

/* pd_adamw_ema (utils_training.py:452-454 optimizer.step/zero_grad, :553-556 EMAModel.step): one pass over flat fp32 buffers:
 *   g *= clip_coef;  torch.optim.AdamW single-tensor update;  ema -= one_minus_decay * (ema - param);  optional grad zeroing.
 * Host passes step_size = lr / (1 - beta1^t), bias_correction2_sqrt = sqrt(1 - beta2^t), one_minus_decay = 1 - EMA decay_t. */
typedef struct {
  int64_t numel;
  float lr, beta1, beta2, eps, weight_decay, step_size, bias_correction2_sqrt, one_minus_decay;
  int zero_grad;
  const float* clip_coef;         /* device scalar from pd_grad_norm, or NULL */
  float* param; float* grad; float* exp_avg; float* exp_avg_sq;
  float* ema;                     /* EMA shadow parameters or NULL */
  int ema_only;                   /* 1: no AdamW update (torch skips parameters whose .grad is None, e.g. the CustomEmbedding on an
                                     unconditional step, utils_training.py:465-471); EMA and grad zeroing still run */
} pd_adamw_ema_args;
int pd_adamw_ema(const pd_adamw_ema_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stable-Diffusion tier (diffusers UNet2DConditionModel as driven by custom_pipeline_stable_diffusion_img2img.py:680-686 and
 * _SD_prediction_wrapper, utils_training.py:459-496).  ResnetBlock2D / GroupNorm / every nn.Linear (as a 1x1 conv over NHWC
 * tokens) / sampling convs reuse pd_conv; the blocks below are what Transformer2DModel adds.
 *
 * pd_attn_d64: softmax(q k^T / sqrt(64)) v, head_dim 64 (BasicTransformerBlock.attn1: self attention; .attn2: cross
 *   attention over the 77 encoder_hidden_states tokens).  Token-major operands with explicit strides, so q/k/v may be
 *   slices of one fused projection output:  q[(b*Nq+i)*q_stride + head*64 + d],  k|v[(b*Nkv+j)*kv_stride + head*64 + d],
 *   out[(b*Nq+i)*out_stride + head*64 + d].
 */
typedef struct {
  int dtype;
  int B, heads, Nq, Nkv;
  const void* q; int q_stride;
  const void* k; const void* v; int kv_stride;
  void* out; int out_stride;
  float* lse;   /* optional out [B][heads][Nq]: log2-domain log-sum-exp of the scaled scores (kept for pd_attn_d64_bwd), or NULL */
} pd_attn_d64_args;
int pd_attn_d64(const pd_attn_d64_args* a, void* stream);

/* pd_token_wgrad: dw[n][k] (+)= sum_m dy[m][n] * x[m][k] -- weight gradient of nn.Linear over M tokens (the Linear layers of
 * BasicTransformerBlock trained through utils_training.py:436), MFMA GEMM with the reduction over tokens; dw is the fp32
 * [N][K] gradient of the nn.Linear weight.  slab: workspace of slab_bytes >= pd_token_wgrad_workspace(a) (smaller is accepted
 * down to one split); partial sums are reduced in a fixed order (bitwise reproducible). */
typedef struct {
  int dtype;
  long long M; int K, N;
  const void* x; int x_stride;
  const void* dy; int dy_stride;
  float* dw; int accumulate;
  float* slab; size_t slab_bytes;
  int stage;                /* (ABI 8) 0: both launches.  1: the GEMM only (partial tiles -> slab).  2: the ordered fold of the slab into dw only -- a caller
                               with one slab per call may run the folds (bandwidth-bound, a few CUs) on a second stream under the next layers' GEMMs */
} pd_token_wgrad_args;
int pd_token_wgrad(const pd_token_wgrad_args* a, void* stream);
size_t pd_token_wgrad_workspace(const pd_token_wgrad_args* a);

/* pd_gn_apply: y = silu?(GroupNorm([x0 | x1])) materialised once (scale / shift from pd_gn_finalize): the GroupNorm-apply +
 * SiLU of ResnetBlock2D.norm1/norm2 (diffusers resnet.py; cond_unet_2d.py:171,187,217 and the SD UNet / VAE blocks) for layers
 * whose convolution has many 64-channel output tiles, where pd_conv's in-flight transform would be repeated per tile. */
typedef struct {
  int dtype; int B, HW, C0, C1; int silu;
  const void* x0; const void* x1;
  const float* scale; const float* shift;   /* [B][C0+C1] */
  void* y;                                  /* NHWC [B][HW][C0+C1] */
} pd_gn_apply_args;
int pd_gn_apply(const pd_gn_apply_args* a, void* stream);

/* pd_linear: y[m][n] = sum_k x[m][k] * W[n][k] + bias[n] (+ residual[m][n]) -- nn.Linear over M tokens as a dedicated MFMA GEMM
 * (128 x 128 workgroup tiles, 64-channel K chunks).  Replaces the Linear layers of BasicTransformerBlock (attn1/attn2 to_q/k/v,
 * to_out.0, FeedForward; reached from custom_pipeline_stable_diffusion_img2img.py:680-686 and utils_training.py:486-494) and,
 * with the transposed weights (pd_pack_weight dgrad = 1), their input gradients.  w_packed: pd_conv's layout for a 1x1 kernel,
 * [N_pad/32][K/32][1][2][64 lanes][8].  x rows may be strided (x_stride elements, >= K); y / residual are dense [M][N]. */
typedef struct {
  int dtype;
  long long M;              /* rows (tokens) */
  int K;                    /* input features, % 32 == 0 */
  int N;                    /* output features, % 8 == 0 */
  int N_pad;                /* packed output features, % 32 == 0 */
  const void* x; int x_stride;
  const void* w_packed;
  const float* bias;        /* [N_pad] */
  const void* residual;     /* [M][N] or NULL */
  void* y;                  /* [M][N] */
  /* optional fusions for the q/k/v projection of diffusers' Attention (cond_unet_2d.py:176-178; AttnProcessor2_0):
     GroupNorm apply on x while staging, and the head-major layout pd_attn_d8 reads */
  const float* scale; const float* shift;   /* [M / rows_per_sample][K] or NULL: x <- x*scale + shift (pd_gn_finalize's output) */
  int rows_per_sample;      /* tokens per sample (multiple of 128 with scale; required with qkv_heads) */
  int qkv_heads;            /* 0: dense y; > 0: y = [3][B][heads][rows_per_sample][8] (N = 3*heads*8, as pd_conv PD_OUT_QKV_HEADS) */
  float* stats_out;         /* NULL, or [M / rows_per_sample][rows_per_sample / 128][N][2]: per-128-token-tile channel (sum, sum of
                               squares) of the stored y -- the consumer's GroupNorm statistics, folded by pd_gn_finalize (T = rows_per_sample/128) */
  int glu;                  /* 1: fused GEGLU (diffusers FeedForward.net[0] = GEGLU: proj -> chunk(2) -> value * gelu(gate)):
                               y = [M][N/2]; w_packed holds the projection's value rows (0 .. N/2) in the even and its gate rows
                               (N/2 .. N) in the odd 32-channel tiles (two pd_pack_weight calls with dst_ct_stride = two tiles);
                               bias stays in module order [N].  N % 64 == 0, no residual / statistics / head-major output */
  float* kmax2_out;         /* NULL, or (qkv_heads > 0, bf16 / fp16) [B][heads] fp32, ZEROED by the caller before the launch:
                               atomically maxed with |k[b][head][n]|^2 of every stored key row -- pd_attn_d8's kmax2 */
  void* fold_ws;            /* (ABI 4) NULL, or a device workspace of >= pd_linear_fold_workspace(a) bytes: the q/k/v projection behind a
                               GroupNorm (scale / shift + qkv_heads) then runs as the DMA-staged GEMM over per-sample weights
                               W diag(scale_n) and biases b + W shift_n written there by a small fold launch (same stream) */
  size_t fold_ws_bytes;
} pd_linear_args;
int pd_linear(const pd_linear_args* a, void* stream);
/* bytes of `fold_ws` that make pd_linear take the folded route for these arguments, 0 when the route does not apply */
size_t pd_linear_fold_workspace(const pd_linear_args* a);

/* pd_attn_wide: softmax(q k^T * scale) v with ONE wide head per D channels, D in {128, 256, 512} -- the mid-block attention of
 * the SD VAE (diffusers AutoencoderKL: Encoder/Decoder.mid_block.attentions[0], a single head over all 512 channels;
 * vae.encode / vae.decode at custom_pipeline_stable_diffusion_img2img.py:431,709-711).  Operand addressing as pd_attn_d64
 * (token-major with strides; channel = head*D + d).  scale = D^-1/2 for diffusers' Attention. */
typedef struct {
  int dtype;
  int B, heads, D, Nq, Nkv;
  float scale;
  const void* q; int q_stride;
  const void* k; const void* v; int kv_stride;
  void* out; int out_stride;
  float* lse;   /* optional out [B][heads][Nq]: log2-domain log-sum-exp of the scaled scores (kept for pd_attn_wide_bwd), or NULL */
} pd_attn_wide_args;
int pd_attn_wide(const pd_attn_wide_args* a, void* stream);

/* pd_attn_hd: softmax(q k^T * scale) v per (batch, head) for the head dimensions between the dedicated kernels:
 * D in {16, 32} (attention_head_dim 16 / 32 of CustomCondUNet2DModel, cond_unet_2d.py:60,100) and D in {40, 80, 160} (the
 * Stable-Diffusion 1.x denoisers, attention_head_dim = 8: eight heads on 320 / 640 / 1280 channels; BasicTransformerBlock.attn1 / .attn2 of
 * the CompVis/stable-diffusion-v1-* and runwayml/stable-diffusion-v1-5 UNets that custom_pipeline_stable_diffusion_img2img.py:108-130
 * names).  Operand addressing as pd_attn_d64 (token-major with element strides, multiples of 8; channel = head*D + d), so q/k/v may
 * be slices of one fused projection output.  scale = D^-1/2 for diffusers' Attention.  Any other D: PD_ERR_SHAPE.  D is padded to
 * the MFMA step in LDS / registers only, with zeros; nothing beyond a head's D channels or a sample's Nkv rows is used.
 * lse is what pd_attn_hd_bwd (D in {16, 32}) recomputes P from; D in {40, 80, 160} has no backward yet. */
typedef struct {
  int dtype;
  int B, heads, D, Nq, Nkv;
  float scale;
  const void* q; int q_stride;
  const void* k; const void* v; int kv_stride;
  void* out; int out_stride;
  float* lse;   /* optional out [B][heads][Nq]: log2-domain log-sum-exp of the scaled scores (as pd_attn_d64_args.lse), or NULL */
} pd_attn_hd_args;
int pd_attn_hd(const pd_attn_hd_args* a, void* stream);

/* pd_attn_hd_bwd: gradient of pd_attn_hd (autograd of F.scaled_dot_product_attention over heads of D channels), D in {16, 32}; any
 * other D: PD_ERR_SHAPE.  P is recomputed from the forward's lse; a delta pre-pass, a dQ kernel and a dK / dV kernel, no atomics: the
 * result is bitwise reproducible.  Fields and addressing as pd_attn_wide_bwd_args (token-major, element strides that are multiples of
 * 8, channel = head*D + d), so dq | dk | dv may be slices of one fused projection's output gradient.
 *   o / dout: the forward's output and the gradient w.r.t. it, [B][Nq][o_stride];  delta: workspace [B][heads][Nq];
 *   dq: [B][Nq][dq_stride];  dk, dv: [B][Nkv][dkv_stride].  fp32 / bf16 / fp16 (fp16 under the trainer's loss scale).
 * Nothing beyond a head's D channels or a sample's Nq / Nkv rows is read, and nothing else is written. */
typedef struct {
  int dtype, B, heads, D, Nq, Nkv; float scale;
  const void* q; int q_stride;
  const void* k; const void* v; int kv_stride;
  const void* o; const void* dout; int o_stride;
  const float* lse; float* delta;
  void* dq; int dq_stride;
  void* dk; void* dv; int dkv_stride;
} pd_attn_hd_bwd_args;
int pd_attn_hd_bwd(const pd_attn_hd_bwd_args* a, void* stream);

/* pd_attn_wide_bwd: gradient of pd_attn_wide (autograd of F.scaled_dot_product_attention, one wide head per D channels): what
 * accelerator.backward(loss) (utils_training.py:436) runs for the attention blocks of orig_google_ddpm_model_denoiser.json
 * (attention_head_dim null -> one 512-channel head, cond_unet_2d.py:176-197).  P is recomputed from the forward's lse.
 *   o / dout: the forward's output and the gradient w.r.t. it, [B][Nq][o_stride];  delta: workspace [B][heads][Nq] (written by the
 *   dQ pass, read by the dK / dV pass);  dq: [B][Nq][dq_stride];  dk, dv: [B][Nkv][dkv_stride].  bf16 / fp32 (fp16: inference only). */
typedef struct {
  int dtype, B, heads, D, Nq, Nkv; float scale;
  const void* q; int q_stride;
  const void* k; const void* v; int kv_stride;
  const void* o; const void* dout; int o_stride;
  const float* lse; float* delta;
  void* dq; int dq_stride;
  void* dk; void* dv; int dkv_stride;
} pd_attn_wide_bwd_args;
int pd_attn_wide_bwd(const pd_attn_wide_bwd_args* a, void* stream);

/* pd_latent_sample: AutoencoderKL.encode(x).latent_dist.sample(generator) (or .mode() when noise = NULL) times the
 * pipeline's scaling_factor (custom_pipeline_stable_diffusion_img2img.py:431-433, utils_Img2Img.py:833-836):
 *   out = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise),  moments = [B][2C][HW] fp32 = [mean | logvar]. */
typedef struct { int B, C, HW; float scale; const float* moments; const float* noise; float* out; } pd_latent_sample_args;
int pd_latent_sample(const pd_latent_sample_args* a, void* stream);

/* pd_latent_chain_bwd: the step between the UNet's input gradient and the encoder's output gradient when the autoencoder trains
 * (`--components_to_train autoencoder`, train.py:189-199; utils_training.py:237-256 encodes inside the step).  Backward of
 *   z = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps)  ->  noisy = sa z + sb noise  ->  loss(model_out, target(z)):
 *   g_clean  = sa[n] * g_noisy + { epsilon: 0;  sample: -g_out;  v_prediction: sb[n] * g_out }
 *              (the reference does not detach clean_images in the target, utils_training.py:415-433)
 *   d mean   = scale * g_clean
 *   d logvar = (-30 <= logvar <= 20) ? scale * g_clean * eps * 0.5 * exp(0.5 * logvar) : 0       (torch's clamp backward)
 * g_noisy, g_out, eps: [B][C][HW] fp32 (g_out may be NULL for epsilon; eps NULL = .mode(): d logvar = 0); moments [B][2C][HW] fp32.
 * out: [B][HW][Cpad] in `dtype`, channels [d mean | d logvar | zeros up to Cpad] -- quant_conv's NHWC output gradient.
 * fp32 arithmetic, one cast at the store.  Any loss scale is already inside g_noisy / g_out. */
typedef struct {
  int dtype; int B, C, HW, Cpad; int pred_type; float scale;
  const float* g_noisy; const float* g_out; const float* moments; const float* eps;
  const float* sa; const float* sb;
  void* out;
} pd_latent_chain_bwd_args;
int pd_latent_chain_bwd(const pd_latent_chain_bwd_args* a, void* stream);

/* pd_layernorm: y[r][c] = (x[r][c] - mean_r) * rstd_r * gamma[c] + beta[c]  (nn.LayerNorm(C), biased variance) */
typedef struct { int dtype; long long rows; int C; float eps; const void* x; const float* gamma; const float* beta; void* y; } pd_layernorm_args;
int pd_layernorm(const pd_layernorm_args* a, void* stream);

/* pd_geglu: y[r][i] = x[r][i] * gelu(x[r][inner + i])   (diffusers GEGLU after its Linear(C, 2*inner); exact erf GELU) */
typedef struct { int dtype; long long rows; int inner; const void* x; void* y; } pd_geglu_args;
int pd_geglu(const pd_geglu_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the Transformer2DModel blocks: what autograd runs under accelerator.backward(loss) (utils_training.py:436)
 * when _SD_prediction_wrapper (utils_training.py:459-496) trains the SD UNet.  Linear layers reuse pd_conv (input gradient,
 * transposed weights) and pd_conv_wgrad (ksize 1).
 *
 * pd_attn_d64_bwd: gradient of pd_attn_d64; P is recomputed from the forward's lse.  o / dout: the forward's output and the
 * gradient w.r.t. it, [B][Nq][o_stride]; delta: workspace [B][heads][Nq]; dq: [B][Nq][dq_stride], dk / dv: [B][Nkv][dkv_stride]
 * (channel = head*64 + d, so they may be slices of one fused projection's output gradient). */
typedef struct {
  int dtype;
  int B, heads, Nq, Nkv;
  const void* q; int q_stride;
  const void* k; const void* v; int kv_stride;
  const void* o; const void* dout; int o_stride;
  const float* lse; float* delta;
  void* dq; int dq_stride;
  void* dk; void* dv; int dkv_stride;
} pd_attn_d64_bwd_args;
int pd_attn_d64_bwd(const pd_attn_d64_bwd_args* a, void* stream);

/* pd_layernorm_bwd: dx = LayerNorm'(x; gamma)(dy) [+ res: the gradient arriving over the skip connection around the
 * normalised branch]; dgamma += sum_rows dy*xhat, dbeta += sum_rows dy (both or neither; `partial` is a workspace of
 * pd_layernorm_bwd_blocks(rows) * 2 * C floats, summed in a fixed order). */
typedef struct {
  int dtype; long long rows; int C; float eps;
  const void* x; const void* dy; const float* gamma; const void* res;
  void* dx; float* dgamma; float* dbeta; float* partial;
  /* ABI 8 (optional, needs `partial` sized for 3 * C floats per block): dxsum[c] += sum_rows dx[row][c] of the STORED dx -- the bias gradient of the
   * Linear layer whose output gradient dx is (the residual stream), without another pass over it */
  float* dxsum;
} pd_layernorm_bwd_args;
int pd_layernorm_bwd(const pd_layernorm_bwd_args* a, void* stream);
int pd_layernorm_bwd_blocks(long long rows);

/* pd_token_embedding_grad: gradient of CustomEmbedding (custom_embedding.py:36-47) from the encoder_hidden_states gradient:
 * dtable[labels[n]][c] += d[n*row_stride + c] (row n = token 0 of sample n; the 76 padding tokens are constants).
 * labels = NULL (unconditional step, utils_training.py:465-471): no-op. */
typedef struct { int dtype; int rows, dim, num_classes; long long row_stride; const int64_t* labels; const void* d; float* dtable; } pd_token_embedding_grad_args;
int pd_token_embedding_grad(const pd_token_embedding_grad_args* a, void* stream);

/* pd_geglu_bwd: x = [h | g] (the forward's input, [rows][2*inner]), dy [rows][inner] -> dx = [dy*gelu(g) | dy*h*gelu'(g)] */
typedef struct {
  int dtype; long long rows; int inner; const void* x; const void* dy; void* dx;
  /* ABI 8 (optional): per-split column sums of dx AS STORED -- the bias gradient of the projection that feeds the gate without another pass over
   * dx: sums[(n * sum_splits + sp) * 2 * inner + c] for the B samples of rows / B rows each (the workspace layout of pd_channel_sum with x = NULL,
   * which folds them).  Needs inner % 256 == 0 and rows % B == 0; sums = NULL: not computed. */
  float* sums; int sum_splits; int B;
} pd_geglu_bwd_args;
int pd_geglu_bwd(const pd_geglu_bwd_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient-guided transfer (_custom_guided_generation, utils_Img2Img.py:699-760).
 * pd_lp_guidance: losses[n] = || x0_n - target_n ||_p (Lp_loss, :245-270) with x0 = DDIMScheduler.step(...).pred_original_sample
 * (prediction type, clipping as pd_ddim_step), and its gradient split the way the chain rule needs it:
 *   d_model_out = dL/dx0 * dx0/d(model_out)   (fed to the UNet backward)      d_sample_direct = dL/dx0 * dx0/d(sample)
 * pd_guidance_apply: out = x - scale * (g_direct + g_unet)   (:747-751)
 */
typedef struct {
  int64_t numel, per_sample;
  int pred_type, clip; float clip_range, sqrt_a, sqrt_b;
  float p;                                  /* finite, >= 1 */
  const float* sample; const float* model_out; const float* target;
  double* partial; int splits;              /* workspace [B][splits] */
  float* d_model_out; float* d_sample_direct;
  float* losses;                            /* out [B] or NULL */
} pd_lp_guidance_args;
int pd_lp_guidance(const pd_lp_guidance_args* a, void* stream);
typedef struct { int64_t numel; float scale; const float* x; const float* g_direct; const float* g_unet; float* out; } pd_guidance_apply_args;
int pd_guidance_apply(const pd_guidance_apply_args* a, void* stream);
/* pd_lp_guidance_scaled: pd_lp_guidance with every d_model_out element multiplied by *grad_scale -- a DEVICE scalar the kernel reads (the
 * host never does), so a captured launch follows the scale between replays.  losses and d_sample_direct are unscaled.  With a power-of-two
 * scale the result is pd_lp_guidance followed by d_model_out * scale, bit for bit.  grad_scale = NULL is refused (PD_ERR_ARG). */
int pd_lp_guidance_scaled(const pd_lp_guidance_args* a, const float* grad_scale, void* stream);
/* pd_guided_step: the elementwise tail of a guided step in ONE launch -- per element
 *   u = g_unet * (1 / *grad_scale)      pushed = sample - guidance_scale * (g_direct + u)      prev_sample = ddim_step(model_out, pushed)
 * bit for bit what `g_unet *= 1 / scale`, pd_guidance_apply and pd_ddim_step(sample = pushed) give as three launches (no guidance combine).
 * A g_unet element that is not finite makes its thread store 1 to *overflow (left untouched otherwise: the caller zeroes it).  Every
 * tensor must be 16-byte aligned (f32x4 loads / stores); a tensor beyond 1024 x 1024 elements is walked in a grid-stride loop. */
typedef struct {
  int64_t numel, per_sample;
  int pred_type, clip; float clip_range;      /* as pd_ddim_step */
  int use_clipped_model_output;
  float sqrt_a, sqrt_b, sqrt_ap, dir_coef;    /* as pd_ddim_step */
  float guidance_scale;                       /* guidance_loss_scale */
  const float* grad_scale;                    /* device scalar, or NULL = 1 */
  const float* sample;                        /* x_t */
  const float* g_direct; const float* g_unet; /* d_sample_direct, the UNet input gradient (scaled) */
  const float* model_out;                     /* computed BEFORE the push */
  float* prev_sample;                         /* out, may alias sample */
  float* pushed;                              /* out or NULL: x_t - s * grad */
  int* overflow;                              /* device, or NULL: set to 1 if any g_unet element is not finite */
} pd_guided_step_args;
int pd_guided_step(const pd_guided_step_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dynamic thresholding (added under ABI 8): DDIMScheduler(thresholding=True), diffusers' _threshold_sample on the fp32 x0 of a step
 *     s = clamp(quantile(|x0|, ratio, per sample), min = 1, max = sample_max_value);   x0 = clamp(x0, -s, s) / s
 * as three entry points (csrc/threshold_kernels.hip; host side phendiff_amd.schedulers.DDIMScheduler.threshold_step):
 *     pd_ddim_raw_x0 -> pd_abs_quantile -> pd_ddim_step_threshold
 *
 * pd_abs_quantile: out[b] = lerp(a_(rank_lo), a_(rank_hi), weight), a_(k) the k-th smallest (0-based) of |x[b][0..n)| -- torch.quantile's
 * 'linear' interpolation once the host has turned (n, q) into (rank_lo, rank_hi, weight) in fp32 (phendiff_amd.schedulers.quantile_rank);
 * lerp(a, b, w) = a + w * (b - a) for w < 0.5, else b - (b - a) * (1 - w), each operation rounded on its own.
 *   x: fp32 [B][n], dense rows; 16-byte aligned when n % 4 == 0 (16-byte loads), 4-byte aligned otherwise (element loads).
 *   Exact selection: the bit pattern of |v| orders like the value for everything that is not a NaN, so a most-significant-digit radix select
 *   over its 31 bits (11 + 10 + 10) finds the order statistic itself.  Per digit one histogram launch over (chunk, row) -- a workgroup
 *   counts PD_ABS_QUANTILE_CHUNK elements of one row into LDS (integer atomics; a wave whose lanes hold one bin adds once) and adds its
 *   non-zero bins to the row's histogram in the workspace with global integer atomics -- and one launch that finds, per row, the bin
 *   holding each of the two ranks.  The two ranks are followed separately (two prefixes, two histograms once they part), so both order
 *   statistics are exact wherever they fall.  Integer counting only: the result does not depend on B, on scheduling or on the replay.
 *   -0 counts as +0; an infinity is the largest value and goes through the lerp as it is; a row that holds a NaN gives NaN and touches
 *   no other row.
 *   workspace: pd_abs_quantile_workspace(B, n) bytes (0 for sizes the call refuses), 4-byte aligned, contents irrelevant before and after:
 *   the entry zeroes it on the stream, with a kernel of its own.  Launches: seven kernels for every (B, n); no host read, no allocation,
 *   capturable.
 *   Refused before any launch: null args / x / out / workspace, ranks outside 0 <= rank_lo <= rank_hi <= n - 1 or more than 1 apart, a
 *   weight outside [0, 1), a misaligned x / out / workspace (PD_ERR_ARG); B, n < 1, n >= 2^31 (32-bit counters), B > 65535 (the grid's
 *   second dimension) (PD_ERR_SHAPE). */
#define PD_ABS_QUANTILE_CHUNK 8192
typedef struct {
  int64_t B, n;
  int64_t rank_lo, rank_hi;
  float weight;
  const float* x;
  float* out;
  void* workspace;
} pd_abs_quantile_args;
size_t pd_abs_quantile_workspace(int64_t B, int64_t n);
int pd_abs_quantile(const pd_abs_quantile_args* a, void* stream);

/* pd_ddim_step_threshold: pd_ddim_step with the static clamp replaced by the dynamic one,
 *     s = min(max(quantile[b], 1), sample_max_value);   x0 = min(max(x0, -s), s) / s     (IEEE division; a NaN quantile makes the row NaN)
 * the guidance combine (both equations), the three prediction types, use_clipped_model_output (eps from the thresholded x0), in-place
 * prev_sample == sample and the optional pred_x0 (the thresholded one) as there.  The struct is pd_ddim_step_args less clip / clip_range,
 * in that struct's order, plus the two trailing fields.
 * pd_ddim_raw_x0(a, x0): the unclamped x0 of the same arguments into x0 [numel] (what pd_abs_quantile reads); a->prev_sample, a->pred_x0
 * and a->quantile are not looked at.  pd_ddim_step_threshold RECOMPUTES x0 from sample / model_out through the same inline function under
 * the same contraction setting (csrc/pd_guided.h: ddim_x0_eps), so the x0 it thresholds is bit for bit the one whose quantile was taken --
 * which is why the raw pass must run before an in-place update overwrites sample.
 * Refused before any launch: null args / sample / model_out / prev_sample (x0) / quantile, guidance without weights, a prediction type
 * outside the three, tensors that are not 16-byte aligned, a quantile that is not 4-byte aligned, sample_max_value that is not positive
 * (PD_ERR_ARG); numel < 1, per_sample < 1 or not a divisor of numel, numel >= 2^41 (the grid) (PD_ERR_SHAPE). */
typedef struct {
  int64_t numel;            /* B*C*H*W */
  int64_t per_sample;       /* C*H*W: element i belongs to row i / per_sample of quantile (and of per-sample guidance weights) */
  int pred_type;            /* pd_pred_type */
  int use_clipped_model_output;
  float sqrt_a, sqrt_b;     /* as pd_ddim_step */
  float sqrt_ap, dir_coef;
  const float* sample;
  const float* model_out;
  const float* uncond_out;  /* NULL: no guidance */
  const float* w;
  int w_per_sample;
  int guidance_cfg;
  float* prev_sample;       /* out (may alias sample) */
  float* pred_x0;           /* out or NULL: the thresholded x0 */
  const float* quantile;    /* [numel / per_sample]: pd_abs_quantile's out, before the clamp to [1, sample_max_value] */
  float sample_max_value;
} pd_ddim_step_threshold_args;
int pd_ddim_raw_x0(const pd_ddim_step_threshold_args* a, float* x0, void* stream);
int pd_ddim_step_threshold(const pd_ddim_step_threshold_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_multistep_step (added under ABI 8; csrc/multistep_kernels.hip, host side phendiff_amd.schedulers.DPMSolverMultistepScheduler /
 * DPMSolverMultistepInverseScheduler): one update of a second-order linear multistep solver of the diffusion ODE (DPM-Solver++ 2M,
 * arXiv 2211.01095, and its noise-prediction twin), one fused elementwise launch on dense fp32 NCHW tensors.  Per element:
 *     o    = model_out, or the guidance combine of pd_ddim_step (same equations, same order of operations)
 *     m0   = form 0 (data prediction):  x0 of pd_ddim_step's three prediction types from (sample, o, sqrt_a, sqrt_b), then the static
 *                                       clamp (clip, clip_range) or, with quantile != NULL, the dynamic one of pd_ddim_step_threshold:
 *                                       s = min(max(quantile[b], 1), sample_max_value), x0 = min(max(x0, -s), s) / s
 *            form 1 (noise prediction): eps of pd_ddim_step's three prediction types; no clamp
 *     prev_sample = a * sample + b * m0                        (c == 0)
 *                   (a * sample + b * m0) + c * (m0 - m1)      (c != 0; m1 = hist_in)
 *     hist_out = m0;   pred_x0 = m0 where given (form 0 only)
 * every operation rounded to fp32 on its own (no contraction).  a, b, c come from the host (fp64, rounded once): the solver's exponential-
 * integrator coefficients of the step from the level (sqrt_a, sqrt_b) to the next one; c = 0 makes the step first-order (DDIM).
 * With c == 0 hist_in is not read at all: it may be NULL, or hold NaN.  prev_sample may alias sample; hist_out must not be hist_in.
 * x0 goes through the inline function pd_ddim_raw_x0 goes through (csrc/pd_guided.h: ddim_x0_eps) under the same contraction setting, so
 * pd_ddim_raw_x0 -> pd_abs_quantile -> pd_multistep_step thresholds bit for bit the x0 whose quantile was taken.
 * A tensor of more than 1024 x 1024 elements is walked in a grid-stride loop; no host read, no allocation, capturable.
 * Refused before any launch: null args / sample / model_out / prev_sample / hist_out, hist_in == NULL with c != 0, hist_out == hist_in,
 * guidance without weights, a prediction type outside the three, a form outside {0, 1}, form 1 with clip != 0, a quantile or pred_x0,
 * tensors that are not 16-byte aligned, w or a quantile that is not 4-byte aligned, a quantile with sample_max_value that is not positive
 * (PD_ERR_ARG); numel < 1, per_sample < 1 or not a divisor of numel (PD_ERR_SHAPE). */
typedef struct {
  int64_t numel;            /* B*C*H*W */
  int64_t per_sample;       /* C*H*W: element i belongs to row i / per_sample of w (per sample) and of quantile */
  int pred_type;            /* pd_pred_type */
  int form;                 /* 0: m0 = x0 (data prediction, "dpmsolver++"), 1: m0 = eps (noise prediction, "dpmsolver") */
  int clip;                 /* form 0: clamp x0 to [-clip_range, clip_range] (not looked at when quantile is given) */
  float clip_range;
  float sqrt_a, sqrt_b;     /* sqrt(alpha_bar), sqrt(1 - alpha_bar) of the level `sample` is at */
  float a, b, c;            /* prev_sample = a * sample + b * m0 + c * (m0 - m1) */
  const float* sample;
  const float* model_out;
  const float* uncond_out;  /* NULL: no guidance */
  const float* w;           /* guidance weights: [B] or 1 value */
  int w_per_sample;
  int guidance_cfg;         /* 0: imagen eqn, 1: CFG eqn */
  const float* hist_in;     /* m1, the previous step's m0; not read when c == 0 (may be NULL then) */
  float* prev_sample;       /* out (may alias sample) */
  float* hist_out;          /* out: m0 (required; not hist_in) */
  float* pred_x0;           /* out or NULL: m0 (form 0 only) */
  const float* quantile;    /* NULL, or [numel / per_sample]: pd_abs_quantile's out (form 0 only) */
  float sample_max_value;
} pd_multistep_step_args;
int pd_multistep_step(const pd_multistep_step_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_guidance_rescale (added under ABI 8; csrc/guidance_rescale.hip, host side phendiff_amd.schedulers.GuidanceRescale): the guided
 * prediction of classifier-free guidance brought back towards the conditional prediction's per-sample standard deviation -- the third
 * fix of arXiv 2305.08891 (section 3.4), diffusers' rescale_noise_cfg -- on dense fp32 [B][per_sample] tensors.  Per sample b:
 *     cfg_i  = the guidance combine of pd_ddim_step: uncond + w (cond - uncond) (imagen) or cond + w (cond - uncond) (CFG), cond =
 *              model_out; the same operations in the same order, each rounded to fp32 on its own (csrc/pd_guided.h: guidance_combine)
 *     s_cond, s_cfg = the unbiased (n - 1) standard deviations of cond and of cfg over the sample, from sum x and sum x^2 accumulated in
 *              fp64 (the square of an fp32 value is exact in fp64): var = max((sum x^2 - (sum x)^2 / n) / (n - 1), 0)
 *     g_b    = rescale * (s_cond / s_cfg) + (1 - rescale)       in fp64, rounded to fp32 once
 *     out_i  = cfg_i * g_b                                       one fp32 multiply
 * which is rescale_noise_cfg factored: rescale * cfg * r + (1 - rescale) * cfg = cfg * (rescale * r + 1 - rescale).
 * Two launches: per-chunk partial sums -- one workgroup of 256 threads per (sample, chunk of PD_GUIDANCE_RESCALE_CHUNK elements) -- then
 * the apply pass on the same tiling, in which every workgroup folds its own sample's partials.  Every sum runs in one fixed order: lane (a
 * thread's elements by ascending index), wave (xor butterfly 32 ... 1), workgroup (waves 0..3), chunk (256 runs of consecutive chunks in
 * index order, then the runs in index order).  Which element a lane takes depends on the element's index within its sample only: a
 * sample's result is a function of that sample alone -- not of B, of its row in the batch, of its alignment, of the grid or of the replay.
 * No atomics, no host read, no allocation, capturable; each input is read twice and out written once.
 *   Rows need not be 16-byte aligned (per_sample % 4 != 0): 16-byte accesses are used where four elements lie whole inside the row at an
 *   aligned address, element accesses everywhere else; nothing outside a row enters its sums.
 *   out may alias model_out (or uncond_out): the apply pass reads an element's inputs before it writes that element, and nothing else.
 *   More than 65536 (sample, chunk) pairs are walked in a grid-stride loop.
 *   A sample with s_cfg = 0 or with a NaN / infinity gives IEEE inf / NaN in its own row and touches no other row.
 *   workspace: pd_guidance_rescale_workspace(B, per_sample) bytes (0 for sizes the call refuses), 8-byte aligned, contents irrelevant
 *   before and after (every partial the apply pass reads was written by the first launch).
 * Refused before any launch: null args / model_out / uncond_out / w / out / workspace, rescale that is not finite or outside [0, 1],
 * tensors that are not 16-byte aligned, w that is not 4-byte aligned, a workspace that is not 8-byte aligned (PD_ERR_ARG); numel < 1,
 * per_sample < 2 or not a divisor of numel, more than 2^31 - 1 (sample, chunk) pairs (PD_ERR_SHAPE). */
#define PD_GUIDANCE_RESCALE_CHUNK 8192
typedef struct {
  int64_t numel;            /* B*C*H*W */
  int64_t per_sample;       /* C*H*W: the elements of one sample (one standard deviation, one guidance weight) */
  const float* model_out;   /* the conditional prediction */
  const float* uncond_out;  /* the unconditional prediction */
  const float* w;           /* guidance weights: [B] or 1 value */
  int w_per_sample;
  int guidance_cfg;         /* 0: imagen eqn, 1: CFG eqn */
  float rescale;            /* phi in [0, 1]: 0 leaves the guided prediction as it is, 1 gives it the conditional one's std */
  float* out;               /* the rescaled guided prediction (may alias model_out) */
  void* workspace;          /* pd_guidance_rescale_workspace(numel / per_sample, per_sample) bytes */
} pd_guidance_rescale_args;
size_t pd_guidance_rescale_workspace(int64_t B, int64_t n);
int pd_guidance_rescale(const pd_guidance_rescale_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Class-contrast masks and the masked blend (added under ABI 8; csrc/mask_kernels.hip, host side phendiff_amd.masked): the DiffEdit recipe
 * (arXiv 2210.11427; diffusers' StableDiffusionDiffEditPipeline.generate_mask) on the pixel tier.  All tensors dense, NCHW, fp32 unless
 * said otherwise; per_pixel = H * W.  No atomics, no host read, no allocation, capturable; every sample's result is a function of that
 * sample alone -- not of B, of its row in the batch, of the grid or of the replay.
 *
 * pd_class_contrast: one noise draw's contribution to the contrast map, from the two noise predictions a [B][C][per_pixel] (target class)
 * and b (source class):
 *     acc[s][p] = (first ? 0 : acc[s][p]) + (sum over c ascending of |a[s][c][p] - b[s][c][p]|) / C
 * every operation rounded to fp32 on its own, the division once at the end.  first != 0: acc is not read (it may hold anything, NaN
 * included).  One launch per draw; one thread per four consecutive elements of acc, the partial last quad and sample boundaries inside a
 * quad included (16-byte loads where four pixels lie whole inside a channel plane at an aligned address, element loads elsewhere).
 * Refused before the launch: null args / a / b / acc, pointers that are not 16-byte aligned (PD_ERR_ARG); B < 1, C outside 1..32,
 * per_pixel < 1, B * C * per_pixel >= 2^62 (PD_ERR_SHAPE).
 *
 * pd_contrast_mask: the accumulated map -> the binary mask.  Per sample s:
 *     mean  = (sum over p of acc[s][p]) / per_pixel       summed and divided in fp64, rounded to fp32 once
 *     limit = ratio * mean                                  fp32
 *     map[s][p]  = fminf(acc[s][p], limit) / limit          (diffusers: clamp(0, mean * ratio) / (mean * ratio))
 *     mask[s][p] = map[s][p] > 0.5f ? 1 : 0
 *     stats[s]   = {mean, limit, (number of pixels with mask 1) / per_pixel}     the count in integers, divided in fp64, rounded to fp32 once
 * A sample whose limit is not a finite positive number -- the classes differ nowhere (limit = 0), or the sample holds a NaN or an
 * infinity -- gets map = 0 and mask = 0 everywhere and the fraction 0; no other sample changes.
 * THE MEAN IS PER SAMPLE.  diffusers takes .mean() over the whole batch of maps, which makes an image's mask depend on its neighbours in
 * the batch; that contradicts the rule above, and at B = 1 both definitions are the same number.  (The sum over draws is not divided by
 * their number: map is invariant to a scaling of acc.)
 * Two launches on one tiling, as pd_guidance_rescale: per-chunk partial sums -- one workgroup of 256 threads per (sample, chunk of
 * PD_CONTRAST_MASK_CHUNK pixels), in the fixed order lane (ascending index), wave (xor butterfly 32 ... 1), workgroup (waves 0..3) -- then
 * the apply pass, in which every workgroup folds its own sample's partials (256 runs of consecutive chunks in index order, then the runs in
 * index order) and writes its chunk; the workgroup of a sample's first chunk also counts the sample's mask for stats.  Which element a lane
 * takes depends on the element's index within its sample only.  More than 65536 (sample, chunk) pairs are walked in a grid-stride loop.
 *   map, stats: optional (NULL: not written).  workspace: pd_contrast_mask_workspace(B, per_pixel) bytes (0 for sizes the call refuses),
 *   8-byte aligned, contents irrelevant before and after.
 * Refused before any launch: null args / acc / mask / workspace, ratio that is not a finite positive number, acc or map not 16-byte
 * aligned, stats not 4-byte aligned, a workspace that is not 8-byte aligned (PD_ERR_ARG); B < 1, per_pixel < 1, more than 2^31 - 1
 * (sample, chunk) pairs (PD_ERR_SHAPE).
 *
 * pd_mask_blend: out[s][c][p] = mask[s][p] ? x[s][c][p] : keep[s][c][p], mask [B][per_pixel] bytes broadcast over the channels.  A
 * SELECTION, not m * x + (1 - m) * keep: the element not taken never enters the result (a NaN or an infinity there does not reach out) and
 * a kept element is keep's, bit for bit.  Any non-zero mask byte takes x.  out may alias x (or keep): a thread reads its four elements
 * before it writes them.  One launch, one thread per four consecutive elements.
 * Refused before the launch: null args / x / keep / mask / out, x / keep / out not 16-byte aligned (PD_ERR_ARG); B < 1, C outside 1..32,
 * per_pixel < 1, B * C * per_pixel >= 2^62 (PD_ERR_SHAPE). */
#define PD_CONTRAST_MASK_CHUNK 2048
typedef struct {
  int64_t B;
  int C;                    /* 1..32 */
  int64_t per_pixel;        /* H*W */
  const float* a;           /* [B][C][per_pixel]: the prediction under the target class */
  const float* b;           /* [B][C][per_pixel]: the prediction under the source class */
  float* acc;               /* [B][per_pixel]: in (unless first) and out */
  int first;                /* != 0: the first draw, acc is written without being read */
} pd_class_contrast_args;
int pd_class_contrast(const pd_class_contrast_args* a, void* stream);

typedef struct {
  int64_t B;
  int64_t per_pixel;        /* H*W */
  const float* acc;         /* [B][per_pixel]: the accumulated contrast of all draws */
  float ratio;              /* threshold_ratio > 0: the map saturates at ratio * mean (diffusers' mask_thresholding_ratio, 3) */
  uint8_t* mask;            /* [B][per_pixel]: 0 / 1 */
  float* map;               /* [B][per_pixel] in [0, 1], or NULL */
  float* stats;             /* [B][3]: mean, limit, masked fraction; or NULL */
  void* workspace;          /* pd_contrast_mask_workspace(B, per_pixel) bytes */
} pd_contrast_mask_args;
size_t pd_contrast_mask_workspace(int64_t B, int64_t per_pixel);
int pd_contrast_mask(const pd_contrast_mask_args* a, void* stream);

typedef struct {
  int64_t B;
  int C;                    /* 1..32 */
  int64_t per_pixel;        /* H*W */
  const float* x;           /* [B][C][per_pixel]: taken where mask != 0 */
  const float* keep;        /* [B][C][per_pixel]: taken where mask == 0 */
  const uint8_t* mask;      /* [B][per_pixel] */
  float* out;               /* [B][C][per_pixel] (may alias x or keep) */
} pd_mask_blend_args;
int pd_mask_blend(const pd_mask_blend_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mask refinement (added under ABI 8; csrc/mask_morph.hip, host side phendiff_amd.mask_ops): disc morphology through an exact
 * Euclidean distance transform, connected components, hole filling and small-component removal -- the clean-up of a per-pixel contrast
 * mask.  Every mask is a dense uint8 [B][H][W] tensor, nonzero = set; 1 <= H, W <= PD_MASK_MAX_SIDE, so H^2 + W^2 < 2^30 and every
 * sum below fits an int32.  A sample's result is a function of that sample alone; nothing is read back by the host; every entry
 * point is a fixed number of launches for given (B, H, W, parameters): capturable.  All arithmetic is in integers, so the results
 * are exact whatever the schedule.  INTEGER atomics (min, add, or) are used: their result does not depend on the order (the house
 * rule "no atomics" is about floating-point sums); floating-point atomics are not.
 *
 * pd_mask_distance: d2[s][y][x] = min over the pixels (y', x') of sample s with (mask != 0) == (to_set != 0) of (y - y')^2 + (x - x')^2;
 * PD_MASK_FAR where the sample holds no such pixel.  Pixels outside the image are neither set nor clear: nothing is padded in.
 * limit > 0: every value above limit -- the PD_MASK_FAR of a sample without such a pixel included -- is written as limit + 1, and
 * the row pass looks at most floor(sqrt(limit)) pixels to either side.  limit = 0: no saturation.  Two launches: the column pass (one
 * thread per (sample, column) scans down, then up, and writes the squared vertical distance into d2) and the row pass (one workgroup
 * per (sample, row) stages the row of d2 in LDS -- 4 W bytes -- and takes min over dx of dx^2 + g2[x + dx], walking outwards from
 * dx = 0 until dx^2 reaches the best so far; neighbouring lanes read neighbouring LDS words), which rewrites the row in place.
 * Refused before any launch: null args / mask / d2, d2 not 4-byte aligned (PD_ERR_ARG); B < 1, H or W outside 1..PD_MASK_MAX_SIDE,
 * limit outside [0, PD_MASK_FAR) (PD_ERR_SHAPE).
 *
 * pd_mask_morph: dilation or erosion by the disc {dy^2 + dx^2 <= r2}, r2 = floor(radius^2) (the host computes it in float64: radius
 * 1 is the 4-neighbour cross, 1.5 the 3 x 3 square, 2 the 13-pixel disc), by thresholding the distance (limit = r2, so O(radius) per
 * pixel):   PD_MORPH_DILATE  out = d2 to the nearest set pixel <= r2      PD_MORPH_ERODE  out = mask && d2 to the nearest clear pixel > r2
 * As the outside of the image is neither set nor clear, an object the image edge cuts is not eroded from the edge and a closing does
 * not pull the border in: scipy.ndimage.binary_dilation(border_value=0) / binary_erosion(border_value=1) under that element.  out is
 * 0 / 1 and may NOT alias mask.  Two launches (the column pass into the workspace, the row pass into out).  workspace:
 * pd_mask_morph_workspace(B, H, W) bytes (int32 [B][H][W]; 0 for sizes the call refuses).  stats (optional): the stats rows of
 * pd_mask_filter (PD_MASK_STATS_FIELDS words per sample, stats_stride words apart), so that an opening or a closing -- two calls --
 * fills one row: with PD_MORPH_STATS_IN in stats_mode the first launch zeroes the whole row and the second adds the set pixels of
 * mask to PD_MS_PIXELS_IN; with PD_MORPH_STATS_OUT the second launch adds the set pixels of out to PD_MS_PIXELS_OUT (integer
 * atomics).  The other three words stay 0.
 * Refused before any launch: null args / mask / out / workspace, out aliasing mask (the two byte ranges overlap), workspace or
 * stats not 4-byte aligned, an op that is not one of the two, a stats_mode outside 0..3 (PD_ERR_ARG); the sizes pd_mask_distance
 * refuses, r2 outside [0, PD_MASK_FAR), stats with stats_stride < PD_MASK_STATS_FIELDS (PD_ERR_SHAPE).
 *
 * pd_mask_components: connected components of one phase (phase = 1: the set pixels, 0: the clear pixels) under connectivity 4 or 8.
 * Outputs (each optional, at least one of the first four required):
 *     label  int32 [B][H][W]   1 + the smallest within-sample linear index y * W + x among the component's pixels; 0 on the other phase
 *     area   int32 [B][H][W]   the pixel count of the pixel's component; 0 on the other phase
 *     border uint8 [B][H][W]   1 where the pixel's component touches row 0, row H - 1, column 0 or column W - 1; 0 on the other phase
 *     count  int32 [B]         the number of components
 *     status int32 [B]         0; nonzero where a device loop met its hard cap (see below) -- the sample's outputs are then unusable
 * Label-equivalence union-find in global memory (Komura 2015; Playne & Hawick 2018; the pointer jumping of Jaiganesh & Burtscher's
 * ECL-CC, 2018), four launches: init (parent[i] = i), merge (a pixel unions with its W and N neighbours, under 8-connectivity also NW
 * and NE, where they share its phase; a pixel at a row's end is no neighbour of the next row's first pixel, a sample's last row none
 * of the next sample's first), flatten (parent[i] = find(i), and at the root an integer atomicAdd for the area and atomicOr for the
 * border flag), broadcast.  parent[i] <= i always and only ever decreases, so the smallest index of a component ends as its root.
 * TERMINATION: find follows parents strictly smaller than the node and ends at a fixed point; union retries only after another
 * thread's atomicMin lowered the root it was about to link, and the larger of its two roots strictly decreases with every retry.
 * Both loops also carry a hard cap of H * W iterations; a loop that meets it stops and sets the sample's status word.  Reads of parent
 * that race with atomicMin are relaxed atomic loads.
 * workspace: pd_mask_components_workspace(B, H, W) bytes (two int32 [B][H * W]: parent, and area + border flag at the roots).
 * Refused before any launch: null args / mask / workspace, no output at all, pointers not aligned to their element (PD_ERR_ARG);
 * the sizes pd_mask_distance refuses, connectivity not 4 or 8, phase not 0 or 1 (PD_ERR_SHAPE).
 *
 * pd_mask_filter: elementwise over mask and the label / area / border of one labelled phase:
 *     PD_FILTER_DROP_SMALL (phase 1)  out = mask && area >= area_limit                          (clears components below min_area)
 *     PD_FILTER_FILL_HOLES (phase 0)  out = mask || (clear && !border && (area_limit < 0 || area <= area_limit))
 * A hole is a component of clear pixels that does not touch the image border; holes are labelled with the connectivity dual to the
 * foreground's (foreground 8: holes 4, foreground 4: holes 8 -- what scipy.ndimage.binary_fill_holes implies).  out is 0 / 1 and may
 * alias mask.  stats (optional) int32, PD_MASK_STATS_FIELDS words per sample, stats_stride words apart: pixels in, pixels out,
 * components seen (pixels with label = index + 1), components kept (DROP_SMALL) or filled (FILL_HOLES), status (copied from
 * `status`, the word pd_mask_components wrote; 0 where status is NULL).  Two launches: the stats rows are initialised, then one
 * workgroup per (sample, 1024 pixels) writes out and adds its four counts with integer atomics.
 * Refused before any launch: null args / mask / label / area / border / out, pointers not aligned to their element, a rule that is
 * not one of the two (PD_ERR_ARG); the sizes pd_mask_distance refuses, DROP_SMALL with area_limit < 0, stats with stats_stride <
 * PD_MASK_STATS_FIELDS (PD_ERR_SHAPE). */
#define PD_MASK_FAR 1073741824
#define PD_MASK_MAX_SIDE 16384
#define PD_MASK_STATS_FIELDS 5
enum { PD_MORPH_DILATE = 0, PD_MORPH_ERODE = 1 };
enum { PD_MORPH_STATS_IN = 1, PD_MORPH_STATS_OUT = 2 };
enum { PD_FILTER_DROP_SMALL = 0, PD_FILTER_FILL_HOLES = 1 };
enum { PD_MS_PIXELS_IN = 0, PD_MS_PIXELS_OUT = 1, PD_MS_COMPONENTS = 2, PD_MS_SELECTED = 3, PD_MS_STATUS = 4 };
typedef struct {
  int64_t B;
  int H, W;                 /* 1..PD_MASK_MAX_SIDE */
  const uint8_t* mask;      /* [B][H][W] */
  int to_set;               /* nonzero: distance to the nearest set pixel; 0: to the nearest clear pixel */
  int limit;                /* 0: exact everywhere; > 0: values above limit are written as limit + 1 */
  int32_t* d2;              /* [B][H][W] */
} pd_mask_distance_args;
int pd_mask_distance(const pd_mask_distance_args* a, void* stream);

typedef struct {
  int64_t B;
  int H, W;
  const uint8_t* mask;      /* [B][H][W] */
  int op;                   /* PD_MORPH_DILATE / PD_MORPH_ERODE */
  int r2;                   /* floor(radius^2) */
  uint8_t* out;             /* [B][H][W]: 0 / 1; may not alias mask */
  void* workspace;          /* pd_mask_morph_workspace(B, H, W) bytes */
  int32_t* stats;           /* [B] rows of PD_MASK_STATS_FIELDS words, stats_stride words apart; or NULL */
  int64_t stats_stride;
  int stats_mode;           /* PD_MORPH_STATS_IN | PD_MORPH_STATS_OUT */
} pd_mask_morph_args;
size_t pd_mask_morph_workspace(int64_t B, int H, int W);
int pd_mask_morph(const pd_mask_morph_args* a, void* stream);

typedef struct {
  int64_t B;
  int H, W;
  const uint8_t* mask;      /* [B][H][W] */
  int phase;                /* 1: label the set pixels; 0: the clear pixels */
  int connectivity;         /* 4 or 8 */
  int32_t* label;           /* [B][H][W] or NULL */
  int32_t* area;            /* [B][H][W] or NULL */
  uint8_t* border;          /* [B][H][W] or NULL */
  int32_t* count;           /* [B] or NULL */
  int32_t* status;          /* [B] or NULL */
  void* workspace;          /* pd_mask_components_workspace(B, H, W) bytes */
} pd_mask_components_args;
size_t pd_mask_components_workspace(int64_t B, int H, int W);
int pd_mask_components(const pd_mask_components_args* a, void* stream);

typedef struct {
  int64_t B;
  int H, W;
  const uint8_t* mask;      /* [B][H][W] */
  const int32_t* label;     /* [B][H][W]: of the phase the rule reads (DROP_SMALL: 1, FILL_HOLES: 0) */
  const int32_t* area;      /* [B][H][W] */
  const uint8_t* border;    /* [B][H][W] */
  const int32_t* status;    /* [B] or NULL */
  int rule;                 /* PD_FILTER_DROP_SMALL / PD_FILTER_FILL_HOLES */
  int area_limit;           /* DROP_SMALL: min_area >= 0; FILL_HOLES: max_area, < 0 = any size */
  uint8_t* out;             /* [B][H][W]: 0 / 1; may alias mask */
  int32_t* stats;           /* [B] rows of PD_MASK_STATS_FIELDS words, stats_stride words apart; or NULL */
  int64_t stats_stride;
} pd_mask_filter_args;
int pd_mask_filter(const pd_mask_filter_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-object measurements (added under ABI 8: three entry points, no existing struct changes; csrc/object_stats.hip, host side
 * phendiff_amd.objects): from the sparse labels of pd_mask_components to one table row per object -- dense labels, integer geometry,
 * intensity sums of an image stack under the labels.  Sizes as for the masks: 1 <= H, W <= PD_MASK_MAX_SIDE, so a sample has at most
 * 2^28 pixels.  K = max_objects (1..2^28) is the number of table rows per sample.  The house rules of the mask section hold: integers
 * are exact (INTEGER atomics only: 64-bit add / min / max / or, whose result has no order), floating-point sums are fp64 in a fixed
 * order with no floating-point atomic anywhere, a sample's result is a function of that sample alone, nothing is read back by the
 * host, and every entry point is a fixed number of launches for given (B, H, W, K, C): capturable.  No device loop is unbounded: every
 * trip count is fixed by the sizes (or, in pd_object_intensity, by a bounding box clamped to the image).
 *
 * pd_object_index: label (int32 [B][H][W] as pd_mask_components writes it: 1 + the smallest within-sample linear index of the pixel's
 * component, 0 on the other phase) -> dense labels.  A ROOT is a pixel with label == y * W + x + 1.
 *     index  int32 [B][H][W]   0 on the other phase; else k in 1..count, the rank of the component's root in raster order among the
 *                              sample's roots -- the numbering scipy.ndimage.label gives.  Components of rank > K get index 0
 *     count  int32 [B]         the TRUE number of components (roots), also where it exceeds K
 *     status int32 [B]         PD_OBJ_OVERFLOW where count > K (components 1..K stay correct); PD_OBJ_BAD_LABEL where a nonzero label lies
 *                              outside 1..H * W or names a pixel that is no root (such a pixel gets index 0; nothing is read out of
 *                              bounds); PD_OBJ_LABEL_STATUS where label_status[s] != 0 (optional input: the status word of
 *                              pd_mask_components, so that one word tells whether the sample's table can be used)
 * A per-sample exclusive prefix sum of the root flags in four launches: per tile of 1024 pixels the number of roots; per sample the
 * exclusive scan of its tile counts (256 at a time with a carry: ceil(tiles / 256) steps) and count / status; per tile again the rank
 * 1 + offset + (roots before the pixel in the tile) written at every pixel of the workspace (0 where the pixel is no root); the gather
 * index = rank[label - 1].  Integer adds in a fixed order.  workspace: pd_object_index_workspace(B, H, W) bytes (int32 [B][H * W]
 * ranks, then int32 [B][ceil(H * W / 1024)] tile offsets; 0 for sizes the call refuses).  index may alias label.
 * Refused before any launch: null args / label / index / count / status / workspace, pointers not 4-byte aligned (PD_ERR_ARG); B < 1,
 * H or W outside 1..PD_MASK_MAX_SIDE, max_objects outside 1..2^28 (PD_ERR_SHAPE).
 *
 * pd_object_geometry: index -> geometry, int64 [B][K][PD_OBJ_GEOM_FIELDS], row k - 1 for index k (an index outside 0..K is read as 0):
 *     PD_OG_AREA  PD_OG_Y0 PD_OG_Y1 PD_OG_X0 PD_OG_X1 (the bounding box, inclusive)  PD_OG_SUM_Y PD_OG_SUM_X PD_OG_SUM_YY PD_OG_SUM_XX
 *     PD_OG_SUM_YX (raw moments of the pixel coordinates)  PD_OG_EDGES  PD_OG_BORDER
 * edges: the number of unit pixel edges between the object and anything that is not that object -- per pixel, the 4-neighbours whose
 * index differs, the outside of the image included (an a x b rectangle: 2 (a + b)).  border: 1 if the object has a pixel in row 0,
 * row H - 1, column 0 or column W - 1.  Rows without an object (k > min(count, K)) are all zero.  Every sum fits: area <= 2^28,
 * y, x < 2^14, so sum_yy, sum_xx, sum_yx < 2^28 * 2^28 = 2^56.
 * Three launches: every word initialised (0; the two minima to INT64_MAX); one wave per (sample, row, 64 columns): the lanes of a RUN
 * of equal index are combined before any atomic -- a run is contiguous in one row, so its length comes from one ballot, its x sums
 * from closed forms, its edges from a segmented wave sum -- and the run's first lane issues the row's 64-bit integer atomics (7 adds,
 * 2 min, 2 max, at most one or); then the minima of empty rows are set to 0.
 * Refused before any launch: null args / index / geometry, index not 4-byte or geometry not 8-byte aligned (PD_ERR_ARG); the sizes
 * pd_object_index refuses (PD_ERR_SHAPE).
 *
 * pd_object_intensity: images (dense NCHW [B][C][H][W]; PD_OBJ_F32, PD_OBJ_U8 or PD_OBJ_U16 -- every value converts to double exactly)
 * under index -> out, double [B][K][C][PD_OBJ_INTENSITY_FIELDS]: PD_OI_SUM, PD_OI_SUMSQ (squares formed in fp64: exact for all three
 * types), PD_OI_MIN, PD_OI_MAX over the object's pixels, per channel.  One launch, one workgroup per (sample, table row, channel): it
 * reads the row's area and bounding box from `geometry` (area <= 0: writes four zeros and exits; the box is clamped to the image, so a
 * table that is not pd_object_geometry's cannot send a read out of bounds), walks the box in raster order -- thread t takes positions
 * t, t + 256, ... -- SELECTS the pixels whose index equals k (nothing is multiplied by zero: a NaN outside the object cannot reach it),
 * adds them in that order and reduces the 256 partial results in a fixed tree (wave butterfly, then the four waves in order).  The
 * result is a function of the object's box, its pixels and their values alone: bitwise reproducible, independent of the batch, the
 * schedule and the other objects.  A NaN inside an object reaches that object's row only (sum and sumsq by arithmetic; min and max
 * are both NaN then).  COST: C * (sum over the objects of their box area) pixel reads -- about the objects' area for compact cells, at
 * most K * H * W * C (objects whose boxes are the whole image).
 * Refused before any launch: null args / index / geometry / images / out, pointers not aligned to their element (PD_ERR_ARG); the
 * sizes pd_object_index refuses, C < 1, B * K * C above 2^31 - 1 workgroups, a dtype that is not one of the three (PD_ERR_SHAPE). */
#define PD_OBJ_GEOM_FIELDS 12
#define PD_OBJ_INTENSITY_FIELDS 4
#define PD_OBJ_MAX_OBJECTS 268435456
enum { PD_OBJ_OVERFLOW = 1, PD_OBJ_BAD_LABEL = 2, PD_OBJ_LABEL_STATUS = 4 };
enum { PD_OBJ_F32 = 0, PD_OBJ_U8 = 1, PD_OBJ_U16 = 2 };
enum { PD_OG_AREA = 0, PD_OG_Y0 = 1, PD_OG_Y1 = 2, PD_OG_X0 = 3, PD_OG_X1 = 4, PD_OG_SUM_Y = 5, PD_OG_SUM_X = 6, PD_OG_SUM_YY = 7,
       PD_OG_SUM_XX = 8, PD_OG_SUM_YX = 9, PD_OG_EDGES = 10, PD_OG_BORDER = 11 };
enum { PD_OI_SUM = 0, PD_OI_SUMSQ = 1, PD_OI_MIN = 2, PD_OI_MAX = 3 };
typedef struct {
  int64_t B;
  int H, W;                     /* 1..PD_MASK_MAX_SIDE */
  int max_objects;              /* K: 1..PD_OBJ_MAX_OBJECTS */
  const int32_t* label;         /* [B][H][W] */
  const int32_t* label_status;  /* [B] or NULL */
  int32_t* index;               /* [B][H][W] (may alias label) */
  int32_t* count;               /* [B] */
  int32_t* status;              /* [B] */
  void* workspace;              /* pd_object_index_workspace(B, H, W) bytes */
} pd_object_index_args;
size_t pd_object_index_workspace(int64_t B, int H, int W);
int pd_object_index(const pd_object_index_args* a, void* stream);

typedef struct {
  int64_t B;
  int H, W;
  int max_objects;              /* K */
  const int32_t* index;         /* [B][H][W] */
  int64_t* geometry;            /* [B][K][PD_OBJ_GEOM_FIELDS] */
} pd_object_geometry_args;
int pd_object_geometry(const pd_object_geometry_args* a, void* stream);

typedef struct {
  int64_t B;
  int H, W;
  int max_objects;              /* K */
  int C;                        /* channels, >= 1 */
  int dtype;                    /* PD_OBJ_F32 / PD_OBJ_U8 / PD_OBJ_U16 */
  const int32_t* index;         /* [B][H][W] */
  const int64_t* geometry;      /* [B][K][PD_OBJ_GEOM_FIELDS]: area and bounding box are read */
  const void* images;           /* [B][C][H][W] */
  double* out;                  /* [B][K][C][PD_OBJ_INTENSITY_FIELDS] */
} pd_object_intensity_args;
int pd_object_intensity(const pd_object_intensity_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Tiled trajectories (added under ABI 8; csrc/tile_kernels.hip, host side phendiff_amd.tiling): the working sample is a canvas
 * (B, C, Hc, Wc), the UNet evaluates overlapping th x tw tiles, their outputs are blended into one canvas-sized model output.  fp32 NCHW.
 * The grid is a tensor product of two axes; per axis with canvas extent L, tile extent t and stride s = t - overlap (1 <= s <= t):
 *     n = ceil((L - t) / s) + 1 tiles,   tile k starts at min(k * s, L - t)   (the last one flush with the edge)
 * so any number of tiles may cover a position.  Tile order everywhere: image b, then ky, then kx; T = B * nty * ntx.
 *
 * pd_tile_gather: tiles [first, first + count) of the canvas -> tiles [count][C][th][tw], a copy (bit for bit).
 * pd_tile_blend: writes EVERY element of out [B][C][Hc][Wc] from the T tile outputs and the per-axis weight tables wy [nty][th],
 * wx [ntx][tw] (phendiff_amd.tiling.TileGrid: normalised so that the weights of a position sum to one on each axis):
 *     out(b, c, y, x) = sum over the covering tiles, ky ascending then kx ascending, of (wy[ky][y - y0] * wx[kx][x - x0]) * tile(...)
 * with the weight product, each term and each addition rounded to fp32 on their own, the first term taken as it is.  Gather form: one
 * thread per output position (or 4 of a row) reads the tiles that cover it -- no atomics, no cleared memory, a function of the inputs alone.
 * Both take 16 bytes per lane where every origin along x, Wc and tw are multiples of 4 and the pointers are 16-byte aligned, 4 bytes
 * otherwise.  One launch each; no host read, no allocation, capturable.
 * Refused before any launch: null args / pointers, pointers that are not 4-byte aligned (PD_ERR_ARG); a size < 1, a tile larger than the
 * canvas, a stride outside [1, tile], tile counts that are not the grid's, first < 0, count < 1, first + count > T, a canvas or a tile batch
 * of 2^31 elements or more (32-bit offsets) (PD_ERR_SHAPE). */
typedef struct {
  int B, C, Hc, Wc;         /* canvas */
  int th, tw;               /* tile extent */
  int nty, ntx;             /* tiles per axis */
  int sy, sx;               /* stride per axis: tile - overlap */
  int first, count;         /* tiles [first, first + count) of T */
  const float* canvas;      /* [B][C][Hc][Wc] */
  float* tiles;             /* out [count][C][th][tw] */
} pd_tile_gather_args;
int pd_tile_gather(const pd_tile_gather_args* a, void* stream);

typedef struct {
  int B, C, Hc, Wc;
  int th, tw;
  int nty, ntx;
  int sy, sx;
  const float* tiles;       /* [T][C][th][tw] */
  const float* wy;          /* [nty][th] */
  const float* wx;          /* [ntx][tw] */
  float* out;               /* [B][C][Hc][Wc] */
} pd_tile_blend_args;
int pd_tile_blend(const pd_tile_blend_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stream capture helpers (hipGraph): the S-step sampling loop is captured once and replayed.
 */
int pd_graph_begin(void* stream);
int pd_graph_end(void* stream, void** graph_exec_out);
int pd_graph_launch(void* graph_exec, void* stream);
int pd_graph_destroy(void* graph_exec);

/* Timing helpers: HIP events on the launch stream (bench.py roofline leg). */
int pd_event_create(void** ev);
int pd_event_record(void* ev, void* stream);
int pd_event_elapsed_ms(void* start, void* stop, float* ms);   /* synchronises on `stop` */
int pd_event_destroy(void* ev);

/* ------------------------------------------------------------------------------------------------
 * (ABI 7) The evaluation metrics' feature extractor: FID / IS / KID as torch_fidelity.calculate_metrics computes them for
 * utils_training.py:948-1001 (per class at evaluation time) and utils_Img2Img.py:462-563 (after a class-transfer experiment) run the
 * "inception-v3-compat" network (TF-Slim InceptionV3 of the original FID code) over uint8 images.  csrc/metric_kernels.hip; host side
 * phendiff_amd/metrics.py (BatchNorm folded into weights / bias at pack time; statistics in fp64 on the host).
 *   pd_resize_tf1: x uint8 NHWC [N][H][W][3] -> y NHWC [N][OH][OW][32] in `dtype` (channels 3..31 zero):
 *       v = bilinear(x) with source coordinate = destination index * scale (scale_y = H / OH, scale_x = W / OW as fp32; no half-pixel
 *       centres, neighbours floor / min(floor + 1, size - 1): interpolate_bilinear_2d_like_tensorflow1x), y = (v - sub) / div.
 *   pd_conv_rect: y[b][oy][ox][y_co + co] = relu?(bias[co] + sum W[co][ci][ky][kx] x[b][oy stride + ky - pad_h][ox stride + kx - pad_w][ci])
 *       for co < Cout_pad; x NHWC with channel stride x_cs (>= Cin, Cin % 32 == 0), y NHWC with channel stride y_cs (the output is a
 *       channel SLICE of a wider tensor: the concatenation of the Inception branches); w_packed = pd_conv's fragment order with
 *       taps = KH * KW (tap = ky * KW + kx), [Cout_pad/32][Cin/32][taps][2][64][8]; bias fp32 [Cout_pad].
 *   pd_pool2d: mode 0 max / 1 average with count_include_pad = False over k x k windows (stride, pad; padding never wins a max),
 *       NHWC -> a channel slice of y; mode 2: global average over Hin x Win -> y fp32 [B][C].
 *   pd_fc_f32: y[r][o] = sum_k x[r][k] wt[k][o] (+ bias[o]), fp32 (wt = the Linear weight transposed, [in][out]). */
typedef struct { int dtype; int N, H, W, OH, OW; float scale_y, scale_x, sub, div; const unsigned char* x; void* y; } pd_resize_tf1_args;
int pd_resize_tf1(const pd_resize_tf1_args* a, void* stream);
typedef struct {
  int dtype; int B, Hin, Win, Cin, Hout, Wout, Cout_pad, KH, KW, stride, pad_h, pad_w, relu;
  const void* x; int x_cs; const void* w_packed; const float* bias; void* y; int y_cs, y_co;
} pd_conv_rect_args;
int pd_conv_rect(const pd_conv_rect_args* a, void* stream);
typedef struct { int dtype; int B, Hin, Win, C, Hout, Wout, k, stride, pad, mode; const void* x; int x_cs; void* y; int y_cs, y_co; } pd_pool2d_args;
int pd_pool2d(const pd_pool2d_args* a, void* stream);
typedef struct { int rows, in_dim, out_dim; const float* x; const float* wt; const float* bias; float* y; } pd_fc_f32_args;
int pd_fc_f32(const pd_fc_f32_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_image_preprocess (added under ABI 8): decoded uint8 images -> the float32 NCHW tensor in [-1, 1] every entry point of the engine starts from.
 * Replaces the per-image host transforms of src/utils_dataset.py:104-127 (Resize(BILINEAR) -> ToTensor -> Normalize [-> RandomHorizontalFlip
 * -> RandomVerticalFlip], and the uint8 "raw" twin Resize -> PILToTensor) and of src/utils_Img2Img.py:197-206.  csrc/data_kernels.hip; host
 * side phendiff_amd/data.py (resample_tables builds the tables).  The resize is Pillow's 8-bit bilinear resample bit for bit: separable,
 * 22-bit fixed-point coefficients, horizontal pass first into uint8, then the vertical pass; an axis whose size does not change is skipped.
 *   x: N images of H x W pixels, uint8, channels interleaved; byte strides image_stride / row_stride / pixel_stride (row_stride >=
 *      W * pixel_stride, image_stride >= the extent of one image).  Cin = 1 | 3 channels are read from every pixel (pixel_stride >= Cin, so
 *      pixel_stride 4 with Cin 3 reads RGBA and drops alpha); one channel is replicated to three (PIL convert("RGB") of mode L).
 *   coef_x int32 [OW][ksize_x], bounds_x int32 [OW][2] = (first source column, count <= ksize_x): the horizontal tables; coef_y [OH][ksize_y],
 *      bounds_y [OH][2] the vertical ones.  ksize = 2 * ceil(max(in / out, 1)) + 1 (checked).  The tables of an axis with in == out are not
 *      read (may be null).  per output: acc = 1 << 21; acc += src[first + k] * coef[k]; out = clamp(acc >> 22, 0, 255).
 *   out_index int32 [N] (null: image n -> slot n): the output slot of each image, 0 <= slot < out_slots (an image whose slot is out of range is
 *      not written) -- a list of mixed source sizes fills one batch in several launches.
 *   y_u8 (may be null): uint8 NHWC [out_slots][OH][OW][3], the resized bytes (never flipped).
 *   y_f32 (may be null): float32 NCHW [out_slots][3][OH][OW] = ((float)u8 / 255.f - mean_c) / std_c (IEEE division, no contraction), written
 *      mirrored per flips[n] (uint8 [N], null = none): bit 0 horizontal, bit 1 vertical.
 * Refused (PD_ERR_SHAPE): a down-scale factor above 32 on an axis; source or output arrays of 4 GiB or more per launch. */
typedef struct {
  int N, H, W, Cin, OH, OW, out_slots;
  long long image_stride, row_stride; int pixel_stride;
  int ksize_x, ksize_y;
  const unsigned char* x;
  const int* coef_x; const int* bounds_x; const int* coef_y; const int* bounds_y;
  const int* out_index; const unsigned char* flips;
  float mean0, mean1, mean2, std0, std1, std2;
  float* y_f32; unsigned char* y_u8;
} pd_image_preprocess_args;
int pd_image_preprocess(const pd_image_preprocess_args* a, void* stream);

/* pd_image_preprocess_bands (added under ABI 8): the same transform for image stacks that are not RGB (Cell Painting's five stains, multiplexed
 * immunofluorescence): C interleaved uint8 bands in, C bands out -- no replication, no dropped channel.  Every band is an independent mode-L
 * image: the tables, the 22-bit fixed point and the horizontal-then-vertical order are those of pd_image_preprocess (one tiled
 * resampler, csrc/pd_resample.h, serves this kernel, that one and the 16-bit entry below).  Fields as in pd_image_preprocess_args, except:
 *   C in 1..32 channels are read from every pixel (C <= pixel_stride <= 64: a wider stride reads a strided view and skips the rest);
 *   mean, std: device float32 [C] (read only when y_f32 is given);
 *   y_u8 uint8 NHWC [out_slots][OH][OW][C]; y_f32 float32 NCHW [out_slots][C][OH][OW] = ((float)u8 / 255.f - mean[c]) / std[c].
 * Refused as pd_image_preprocess refuses, plus C out of range (PD_ERR_ARG) and null mean / std with y_f32 (PD_ERR_ARG).  A workgroup stages
 * whole source rows at the pixel stride given (span_x * pixel_stride + 4 bytes a row, span_x up to ~1060 columns at a 32 x horizontal
 * down-scale), so a view into wide pixels (pixel_stride above ~45 at that scale) is refused with "tile does not fit the LDS budget"
 * (PD_ERR_SHAPE) where the same bands stored densely run: pass a dense copy then (ImagePreprocessor does). */
typedef struct {
  int N, H, W, C, OH, OW, out_slots;
  long long image_stride, row_stride; int pixel_stride;
  int ksize_x, ksize_y;
  const unsigned char* x;
  const int* coef_x; const int* bounds_x; const int* coef_y; const int* bounds_y;
  const int* out_index; const unsigned char* flips;
  const float* mean; const float* std;
  float* y_f32; unsigned char* y_u8;
} pd_image_preprocess_bands_args;
int pd_image_preprocess_bands(const pd_image_preprocess_bands_args* a, void* stream);

/* pd_image_preprocess_bands16 (added under ABI 8): pd_image_preprocess_bands for 16-bit sources (plate-reader / sCMOS TIFFs): C interleaved
 * uint16 bands in, C bands out, every band resampled as Pillow resamples a mode I;16 image (its 16bpc path), bit for bit.
 * csrc/data16_kernels.hip over the resampler, checks and band kernel of csrc/pd_resample.h; host side phendiff_amd/data.py (resample_tables_f64 builds the tables).  Fields as in
 * pd_image_preprocess_bands_args, except:
 *   x: uint16, 2-byte aligned; the strides stay BYTE strides and must be even; 2 * C <= pixel_stride <= 128.
 *   coef_x double [OW][ksize_x], coef_y double [OH][ksize_y]: the float64 triangle-filter weights, normalised by the row sum, NOT rounded to
 *      fixed point (zero past each row's count); bounds_* and ksize_* as in the 8-bit entries.
 *      per output: ss = 0.0; ss = ss + (double)src[first + k] * coef[k] for k in order (product and sum rounded separately: no FMA);
 *      out = clamp((int)(ss + 0.5), 0, 65535).  Horizontal pass first INTO uint16, then the vertical pass; an unchanged axis is skipped.
 *   y_u16 (may be null): uint16 NHWC [out_slots][OH][OW][C], the resized samples (never flipped).
 *   y_f32 (may be null): float32 NCHW [out_slots][C][OH][OW]: f = ((float)v - lo[c]) / (hi[c] - lo[c]); f = min(max(f, 0), 1) (a NaN stays
 *      one); y = (f - mean[c]) / std[c] -- five IEEE fp32 operations, no reciprocal, no contraction; mirrored per flips[n].
 *   lo, hi, mean, std: device float32 [C], read only when y_f32 is given (lo = 0, hi = 65535: the v / 65535 analogue of ToTensor).
 * Refused as pd_image_preprocess_bands refuses, plus odd strides or an odd x (PD_ERR_SHAPE / PD_ERR_ARG) and null lo / hi with y_f32
 * (PD_ERR_ARG).  A workgroup stages whole source rows at the pixel stride given: a view into wide pixels under a steep horizontal down-scale
 * is refused with "tile does not fit the LDS budget" (PD_ERR_SHAPE) where the same bands stored densely run. */
typedef struct {
  int N, H, W, C, OH, OW, out_slots;
  long long image_stride, row_stride; int pixel_stride;
  int ksize_x, ksize_y;
  const unsigned short* x;
  const double* coef_x; const int* bounds_x; const double* coef_y; const int* bounds_y;
  const int* out_index; const unsigned char* flips;
  const float* lo; const float* hi; const float* mean; const float* std;
  float* y_f32; unsigned short* y_u16;
} pd_image_preprocess_bands16_args;
int pd_image_preprocess_bands16(const pd_image_preprocess_bands16_args* a, void* stream);

/* pd_band_histogram16 (added under ABI 8): exact per-band value counts of uint16 stacks, counts[c][v] += number of samples of band c equal to
 * v -- what an intensity window (percentiles) is read from.  The source is addressed as in pd_image_preprocess_bands16 (N images of H x W
 * pixels, C in 1..32 bands read from each, even byte strides, 2 * C <= pixel_stride; no upper limit on pixel_stride here).
 *   counts: device unsigned int [C][65536].  The caller zeroes it; launches ACCUMULATE (a list of mixed sizes sums over its groups).
 * Integer counting only: the result does not depend on scheduling and is bitwise reproducible.  A workgroup counts one band of a chunk of
 * at most 65535 pixels into a whole 65536-bin histogram of 16-bit counters in LDS (128 KiB) and adds its non-zero bins to `counts`.
 * Refused: N * H * W >= 2^32, odd or too small strides (PD_ERR_SHAPE); null pointers, an odd x, C out of range (PD_ERR_ARG). */
typedef struct {
  int N, H, W, C;
  long long image_stride, row_stride; int pixel_stride;
  const unsigned short* x;
  unsigned int* counts;
} pd_band_histogram16_args;
int pd_band_histogram16(const pd_band_histogram16_args* a, void* stream);

/* pd_postproc_bands16 (added under ABI 8): the way back from the engine's float32 NCHW tensors to uint16 stacks in the source's range (the
 * inverse of pd_image_preprocess_bands16's float tail), element-wise:
 *   f = x * std[c] + mean[c] (two roundings); f = clamp(f, 0, 1), NaN -> 0; r = f * (hi[c] - lo[c]) + lo[c] (two roundings);
 *   y = clamp(rintf(r), 0, 65535) (round half to even; NaN -> 0).
 *   x float32 NCHW [N][C][H][W]; y uint16 NHWC [N][H][W][C]; lo, hi, mean, std device float32 [C]. */
typedef struct {
  int N, C, H, W;
  const float* x;
  const float* lo; const float* hi; const float* mean; const float* std;
  unsigned short* y;
} pd_postproc_bands16_args;
int pd_postproc_bands16(const pd_postproc_bands16_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_train_sample (added under ABI 8): the per-step sampling of perform_training_epoch (utils_training.py:244-256) on the device, one launch:
 * Gaussian noise, timesteps and noisy = sqrt_acp[t] * clean + sqrt_1m_acp[t] * noise in a single pass over `clean`.  csrc/sample_kernels.hip;
 * host side phendiff_amd.training.DeviceTrainingSampler.  The values depend only on (seed, step, rank, purpose, element index) -- not on the
 * launch geometry, the batch split or the pointers -- so a run resumes from (seed, rank, step) alone.  It is NOT torch's CPU stream and NOT
 * torch's device Philox layout.
 *
 * The stream (the contract): Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85; ten rounds) with
 *     key     = (seed low 32 bits, seed high 32 bits)
 *     counter = (q low 32 bits, q high 32 bits, step low 32 bits, (step bits 32..47 << 16) | (rank << 4) | purpose)
 *   rank < 4096, step < 2^48; purpose 0 = training noise, 1 = timesteps (never a noise purpose), 2 = posterior noise / a plain randn.
 *   noise: flat element e = elem_base + i (i = index into this launch's buffers) takes word e & 3 of counter q = e >> 2.  Words (0, 1) are
 *     one Box-Muller pair, words (2, 3) the other: with u = (x >> 8) * 2^-24 + 2^-25 in (0, 1) (evaluated exactly: 25 significant bits, more
 *     than one fp32 holds, so the kernel takes ln u as log1p(u - 1) and the angle as 2 u - 2 in the upper half of the interval),
 *     r = sqrt(-2 ln u_a), z_even = r * cospi(2 u_b), z_odd = r * sinpi(2 u_b); precise logf / log1pf / sqrtf / sincospif, fp32.
 *   timesteps: t_b = ((uint64)x * N) >> 32 with x = word 0 of counter q = b (b = i / per_sample, the sample index within this launch)
 *     under purpose 1; written as int64 by the thread that holds sample b's first element.
 *   noisy: sqrt_acp[t_b] * clean + sqrt_1m_acp[t_b] * noise, two products and one sum without contraction: bit-identical to pd_add_noise on
 *     the same noise and t.  The tables are fp32 [N] on the device (the host-computed ones DiffusionLoss / add_noise gather from).
 * One thread per Philox counter = four consecutive elements: 16-byte loads / stores where the quad lies whole inside one sample and the
 * buffers are aligned there, element by element where it straddles two samples (per_sample % 4 != 0), is cut by the end of the tensor or
 * by an elem_base that is no multiple of 4.  B, per_sample and their product are arbitrary positive sizes.
 *   clean == NULL: a pure randn fill of noise[B * per_sample] (noisy must be NULL); timesteps are drawn only when timesteps_out is given.
 *   timesteps_in (optional, int64 [B], values in [0, N); the table index is clamped to that range): used instead of drawing, never written.
 * Refused before any launch: null args / noise, N <= 0 where timesteps are needed, rank / step / purpose out of range, clean without tables or
 * noisy or a source of timesteps, noisy without clean (PD_ERR_ARG); B, per_sample <= 0, a product or elem_base + product beyond 2^62, more
 * than 2^31 - 1 blocks (PD_ERR_SHAPE). */
typedef struct {
  uint64_t seed, step;
  int rank, purpose;
  int64_t B, per_sample;
  uint64_t elem_base;
  int N;
  const float* clean;
  const float* sqrt_acp; const float* sqrt_1m_acp;
  const int64_t* timesteps_in;
  int64_t* timesteps_out;
  float* noise; float* noisy;
} pd_train_sample_args;
int pd_train_sample(const pd_train_sample_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_stream_noise / pd_stream_advance (added under ABI 8): out = a * x + b * z over fp32 [B][per_sample], z drawn from pd_train_sample's
 * stream above -- the same key and counter layout, the same Box-Muller, the same rounding (csrc/pd_philox.h is compiled into both) -- at a
 * position that lives in DEVICE memory, so that a captured launch draws new numbers on every replay.  csrc/stream_noise.hip; host side
 * phendiff_amd.DeviceNoise; the from-noise generation of trajectories.GenerationGraph.
 *
 *   state: 16 bytes on the device, {uint64 seed, uint64 index}; read by every launch, written only by pd_stream_advance.
 *   One stream per IMAGE: row b of a launch draws with step = index + index_offset + b, so image k of a run is a function of (seed, k)
 *     alone, whatever the batch size, the rank layout or the number of batches drawn before it.  Element e of the row is flat element
 *     elem_base + e of that stream: word (elem_base + e) & 3 of counter q = (elem_base + e) >> 2 under
 *     counter = (q low, q high, step low 32 bits, ((step bits 32..47) << 16) | (rank << 4) | purpose), key = (seed low, seed high).
 *     Row b equals pd_train_sample's `noise` for (seed, step, rank, purpose, B = 1, per_sample, elem_base), bit for bit.
 *   Purposes, beside pd_train_sample's 0 (training noise), 1 (timesteps: never a noise purpose) and 2 (randn):
 *     PD_PURPOSE_INITIAL_SAMPLE  3  x_T of a generation, elem_base = 0;
 *     PD_PURPOSE_FORWARD_NOISE   4  the noise of add_forward_noise_to_image / DDIMScheduler.add_noise, elem_base = 0;
 *     PD_PURPOSE_VARIANCE_NOISE  5  the variance noise of stochastic DDIM (eta > 0): trajectory step i (its position in the scheduler's
 *                                   timesteps) takes elements i * per_sample .. (i + 1) * per_sample - 1 of the image's stream.
 *   Coefficients: the scalars a, b by value, or -- sa and sb both given -- per-row device tables sa[B], sb[B] (DDIMScheduler.add_noise's
 *     form).  x == NULL: out = b * z.  out may be x.  Each product and the sum are rounded separately (no contraction), as pd_add_noise
 *     rounds them: with the tables the result is pd_add_noise's on the same z, bit for bit.
 *   per_sample is a multiple of 4 (every model's C * H * W here), so no counter straddles two images; elem_base is arbitrary: a head or
 *     tail counter cut by the row's ends is written element by element, everything else by 16-byte loads and stores where x and out are
 *     aligned there.  One thread per counter; no atomics; nothing read outside x, the tables and the state, nothing written outside out.
 *   The step field holds 48 bits.  index_offset + B beyond 2^48 is refused; the launch cannot refuse a device-side index that has grown
 *     past it: the field then WRAPS (step mod 2^48), i.e. the streams of the first images come again.  DeviceNoise checks its host
 *     shadow of the index before every launch.
 * pd_stream_advance: index += n by one thread; capturable -- the last node of a captured generation, so the next replay draws the next
 *   images.
 * Refused before any launch: null args / state / out, a misaligned pointer, rank outside [0, 4096), purpose outside 0 .. 15 or 1, only one
 * of sa / sb, index_offset + B > 2^48 (PD_ERR_ARG); B < 1, per_sample < 1 or no multiple of 4, a grid of 2^31 blocks or more
 * (PD_ERR_SHAPE). */
#define PD_PURPOSE_INITIAL_SAMPLE 3
#define PD_PURPOSE_FORWARD_NOISE 4
#define PD_PURPOSE_VARIANCE_NOISE 5
typedef struct {
  const uint64_t* state;    /* device: {seed, index} */
  uint64_t index_offset;
  int rank, purpose;
  int64_t B, per_sample;
  uint64_t elem_base;
  float a, b;               /* used when sa == NULL */
  const float* sa; const float* sb;   /* [B] (device) or both NULL */
  const float* x;           /* [B][per_sample] or NULL */
  float* out;               /* [B][per_sample]; may be x */
} pd_stream_noise_args;
int pd_stream_noise(const pd_stream_noise_args* a, void* stream);
int pd_stream_advance(void* state, uint64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_sample_stats (added under ABI 8): per-sample diagnostics of a batch that stays on the device -- what check_Gaussianity
 * (utils_Img2Img.py:79-93: mean, std, a 100-bin histogram on (-3, 3), scipy's normaltest) and Lp_loss (:245-270) need from an inverted batch
 * or a regenerated one, reduced to B x (PD_SAMPLE_STATS_FIELDS + bins) numbers.  csrc/sample_stats.hip; host side phendiff_amd.diagnostics
 * (check_gaussianity, sample_distances; normaltest_from_moments turns n, m2, m3, m4 into K^2 and its p-value).
 *   x: contiguous [B][n] of `dtype` (PD_F32 / PD_BF16 / PD_F16); sample b starts at element b * n, whatever its alignment.  Every element is
 *      widened to fp64 (exactly) before any arithmetic.
 *   y (may be null): same dtype; y_sample_stride = n for one y per sample, 0 for one y[n] shared by all samples (Lp_loss's (N,C,H,W) / (C,H,W)).
 *   bins > 0: edges = bins + 1 ascending fp64 values on the device (np.linspace(lo, hi, bins + 1) for np.histogram's uniform bins) and hist
 *      [B][bins] uint32.  Element v falls in bin k when edges[k] <= v < edges[k + 1]; the last bin also takes v == edges[bins]; anything else
 *      (a NaN, an infinity, a value outside) falls in no bin.  The bin is guessed as (int)((v - edges[0]) * bins / (edges[bins] - edges[0])) in
 *      fp64 and then moved until the comparisons with edges[k] / edges[k + 1] hold (the guess alone is one off at some edges), so with linspace
 *      edges the counts equal np.histogram(x64, bins, (lo, hi)) count for count.  bins <= PD_SAMPLE_STATS_MAX_BINS = 4096 (edges and counts of
 *      one workgroup live in LDS: 12 * bins + 8 bytes); n < 2^32 (the counts are uint32).  hist is zeroed by a launch of the call's own.
 *   stats [B][PD_SAMPLE_STATS_FIELDS] fp64, every field written by every call:
 *      PD_SS_SUM, PD_SS_MIN, PD_SS_MAX, PD_SS_NONFINITE: sum of the elements (mean = sum / n), smallest and largest element (a NaN is passed
 *        over; +inf / -inf when every element is a NaN), number of NaN / infinite elements.
 *      PD_SS_M2, PD_SS_M3, PD_SS_M4: central moments sum(d^k) / n with d = x - sum / n in fp64 (two passes: no cancellation for a shifted
 *        sample).  They, and the sum, are NaN / infinite when PD_SS_NONFINITE > 0 -- the IEEE result, as numpy's would be.
 *      PD_SS_ERR_L1, PD_SS_ERR_SQ, PD_SS_ERR_MAX: sum |e|, sum e^2, max |e| with e = x - y in fp64; 0 when y is null.
 *   workspace: pd_sample_stats_workspace(B, n, bins) bytes (the per-chunk partials: 80 bytes per PD_SAMPLE_STATS_CHUNK elements of a sample;
 *      0 for sizes the call refuses), 8-byte aligned, contents irrelevant before and after; workspace_bytes states what the caller allocated.
 * Launches: [zero hist], pass A (per-chunk sum / min / max / non-finite), a fold per sample, pass B (per-chunk sums of d^2 d^3 d^4, the error
 * sums, the histogram in LDS integer atomics flushed with global integer atomic adds), a fold per sample; no host synchronisation, capturable.
 * Every floating-point reduction runs in a fixed order (lane, wave, workgroup, chunk index) and the element -> lane map depends on the index
 * within the sample only (16-byte loads where a slot is aligned and whole, element loads elsewhere, same values to the same lane): a
 * sample's stats and hist are bitwise reproducible and do not depend on B, on its row in the batch or on the pointers' alignment.
 * Refused before any launch: null args / x / stats / workspace, a dtype outside the three, bins < 0, bins > 0 without edges or hist, a
 * workspace_bytes below the query's (PD_ERR_ARG); B, n <= 0, bins > PD_SAMPLE_STATS_MAX_BINS, y_sample_stride outside {0, n}, B * n >= 2^62,
 * n >= 2^32 with bins > 0, more than 2^31 - 1 blocks (PD_ERR_SHAPE). */
#define PD_SAMPLE_STATS_FIELDS 10
#define PD_SAMPLE_STATS_CHUNK 8192
#define PD_SAMPLE_STATS_MAX_BINS 4096
enum { PD_SS_SUM = 0, PD_SS_MIN = 1, PD_SS_MAX = 2, PD_SS_NONFINITE = 3, PD_SS_M2 = 4, PD_SS_M3 = 5, PD_SS_M4 = 6,
       PD_SS_ERR_L1 = 7, PD_SS_ERR_SQ = 8, PD_SS_ERR_MAX = 9 };
typedef struct {
  int dtype, bins;
  int64_t B, n;
  int64_t y_sample_stride;
  const void* x; const void* y;
  const double* edges;
  double* stats;
  uint32_t* hist;
  void* workspace; size_t workspace_bytes;
} pd_sample_stats_args;
size_t pd_sample_stats_workspace(int64_t B, int64_t n, int bins);
int pd_sample_stats(const pd_sample_stats_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_ssim (added under ABI 8): structural similarity (Wang et al. 2004) and the ingredients of multi-scale SSIM (Wang et al. 2003) between
 * two batches that stay on the device, reduced to B x C x levels x 2 fp64 numbers: per (sample, channel, scale) the mean of the SSIM map and
 * the mean of its contrast-structure factor.  csrc/ssim.hip; host side phendiff_amd.diagnostics (ssim_maps_means, sample_ssim: the channel
 * means, the clamp, the powers and the product of MS-SSIM are taken there in float64).
 *   x: contiguous [B][C][H][W] of `dtype` (PD_F32 / PD_BF16 / PD_F16); sample b starts at element b * C * H * W, whatever its alignment.
 *      Every element is widened to fp64 (exactly) before any arithmetic, and everything after it is fp64.
 *   y: same dtype; y_sample_stride = C * H * W for one y per sample, 0 for one y [C][H][W] shared by all samples.
 *   w0 .. w(win - 1): the window's taps, BY VALUE (nothing to keep alive for a captured graph); win odd, 3 .. PD_SSIM_MAX_WIN.  The host
 *      passes g[i] = exp(-(i - (win - 1) / 2)^2 / (2 sigma^2)) / sum (diagnostics.gaussian_window); taps past win are ignored.  The 2-D
 *      window is the outer product of the taps, applied as a row filter and then a column filter.  Filtering is VALID: no padding, the maps
 *      have (H - win + 1) x (W - win + 1) positions (Wang et al.'s original; pytorch_msssim).
 *   Per position, with mx, my, exx, eyy, exy the five filtered maps of x, y, x^2, y^2, xy:
 *        vx = exx - mx^2, vy = eyy - my^2, vxy = exy - mx my
 *        cs = (2 vxy + c2) / (vx + vy + c2),   ssim = cs (2 mx my + c1) / (mx^2 + my^2 + c1)
 *      c1 = (0.01 R)^2, c2 = (0.03 R)^2 for a data range R are the caller's to compute; both finite and positive.
 *   levels 1 .. PD_SSIM_MAX_LEVELS: scale s >= 1 is scale s - 1 of both images reduced by a 2x2 mean of stride 2, an odd trailing row or
 *      column dropped, computed as ((a00 + a01) + (a10 + a11)) * 0.25 in fp64 and KEPT in fp64.  min(H, W) >> (levels - 1) >= win.
 *   out [B][C][levels][2] fp64, every element written by every call: [..][s][0] the mean of ssim, [..][s][1] the mean of cs over the valid
 *      positions of scale s.  A NaN / infinity in a plane of x or y makes that plane's numbers NaN (the IEEE result) and no other's.
 *   workspace: pd_ssim_workspace(B, C, H, W, levels) bytes (16 bytes per tile of 16 x 32 positions, counted for the smallest window, plus
 *      the fp64 pyramid of both images, y's counted per sample; 0 for sizes the call refuses), 8-byte aligned, contents irrelevant before and
 *      after; workspace_bytes states what the caller allocated.
 * Launches: per scale s >= 1 one reduce launch for x and one for y, per scale one tiled pass (a workgroup of 256 threads owns 16 x 32 valid
 * positions of one plane: it stages those plus the win - 1 halo of x and y in LDS as fp64, filters rows into five LDS maps, then columns,
 * and reduces ssim / cs to one pair; LDS 8 (2 (15 + win)(31 + win) + 160 (15 + win)) bytes: 50,752 at win 11, 110,592 at win 33), one fold
 * launch at the end; 2 * levels .. 3 * levels - 1 launches, no host synchronisation, capturable.
 * Every sum runs in a fixed order (lane, wave, workgroup, tile index), no floating-point atomics; only element loads are used and the
 * position -> lane map depends on the position within the plane only: a sample's numbers are bitwise reproducible and do not depend on B, on
 * its row in the batch or on the pointers' alignment.  Nothing outside x's B * C * H * W and y's elements is read: a position outside a
 * plane is never loaded, and what would need it is left out by selection, never multiplied by zero.
 * Refused before any launch: null args / x / y / out / workspace, a dtype outside the three, non-finite or non-positive c1 / c2, a
 * non-finite tap, a workspace_bytes below the query's (PD_ERR_ARG); B, C, H, W <= 0, an even win or one outside 3 .. 33, levels outside
 * 1 .. 5, min(H, W) >> (levels - 1) < win, y_sample_stride outside {0, C * H * W}, more than 2^40 elements or 2^31 - 1 workgroups
 * (PD_ERR_SHAPE). */
#define PD_SSIM_MAX_WIN 33
#define PD_SSIM_MAX_LEVELS 5
typedef struct {
  int dtype, C, H, W, win, levels;
  int64_t B, y_sample_stride;
  double w0, w1, w2, w3, w4, w5, w6, w7, w8, w9, w10, w11, w12, w13, w14, w15, w16, w17, w18, w19, w20, w21, w22,
         w23, w24, w25, w26, w27, w28, w29, w30, w31, w32;
  double c1, c2;
  const void* x; const void* y;
  double* out;
  void* workspace; size_t workspace_bytes;
} pd_ssim_args;
size_t pd_ssim_workspace(int64_t B, int C, int H, int W, int levels);
int pd_ssim(const pd_ssim_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_kid_mmd, pd_feature_moments (added under ABI 8): the statistics of KID and FID over features that stay on the device -- torch-fidelity's
 * metric_kid.py (polynomial-kernel MMD^2 over random subsets) and metric_fid.py (mean and np.cov) -- in fp64 on v_mfma_f64_16x16x4_f64 from
 * fp32 features (every element widened exactly before any arithmetic).  csrc/metric_stats.hip; host side phendiff_amd.metrics
 * (kernel_inception_distance_device, fid_statistics_device).  The matrix square root of FID and the Inception score stay on the host.
 *
 * pd_kid_mmd: for subset s, a_i = f1[idx1[s][i]] and b_i = f2[idx2[s][i]] (i < m), k(x, y) = (x . y * gamma + coef0)^degree (the power by
 * repeated multiplication):
 *     sums[s] = ( sum_{i != j} k(a_i, a_j),  sum_{i != j} k(b_i, b_j),  sum_{i, j} k(a_i, b_j) )
 *     mmd[s]  = (sums[s][0] + sums[s][1]) / (m (m - 1)) - 2 sums[s][2] / m^2
 *   f1 [N1][f1_stride], f2 [N2][f2_stride]: fp32, 16-byte aligned, strides in elements (>= D, multiples of 4); D a multiple of 64 in 64 .. 4096.
 *   idx1, idx2: int32, row s at element s * idx_stride (idx_stride >= m); only the first m entries of a row are read.  CONTRACT:
 *     0 <= idx1 < N1 and 0 <= idx2 < N2 -- the contents cannot be checked without a launch; the caller draws them and answers for them.
 *   One workgroup per PD_METRIC_STATS_TILE^2 tile of a kernel matrix (XX and YY: upper-triangle tiles, an off-diagonal one counted twice; XY:
 *   all); the matrices are never stored.  Rows at or past m of a ragged tile are not read and their kernel values are selected away (not
 *   multiplied by zero), as are the diagonals of XX / YY.  One fp64 partial per tile goes to the workspace, a second launch folds a subset's
 *   partials in tile order: no atomics, every sum in a fixed order -- results are bitwise reproducible and subset s does not depend on S or
 *   on the other subsets.
 *   workspace: pd_kid_mmd_workspace(S, m) bytes (8 per tile; 0 for sizes the call refuses), 8-byte aligned, contents irrelevant.
 *   Refused before any launch: null args / pointers, misaligned f1 / f2, degree outside 1 .. 8, non-finite gamma / coef0, a workspace_bytes
 *   below the query's (PD_ERR_ARG); D, the strides, S < 1, m < 2, m > min(N1, N2), idx_stride < m, more than 2^31 - 1 workgroups (PD_ERR_SHAPE).
 *
 * pd_feature_moments: mean [D] = sum_n f[n] / N and cov [D][cov_stride] = (F - mean)^T (F - mean) / (N - 1) (np.cov(rowvar=False)), fp64.
 *   Column sums per chunk of PD_FEATURE_MOMENTS_CHUNK rows, folded in chunk order; the covariance contracts the centred rows (centred in fp64,
 *   rows at or past N selected to zero) per upper-triangle tile and writes the tile and its mirror image from the same registers: cov is
 *   bitwise symmetric, every element of its D columns is written, columns D .. cov_stride - 1 are left alone.
 *   workspace: pd_feature_moments_workspace(N, D) bytes (the chunk sums; 0 for sizes the call refuses).
 *   Refused before any launch: null args / pointers, misaligned f, a workspace_bytes below the query's (PD_ERR_ARG); D not a multiple of 64
 *   in 64 .. 4096, f_stride < D or not a multiple of 4, cov_stride < D, N < 2, N >= 2^31 (PD_ERR_SHAPE). */
#define PD_METRIC_STATS_TILE 64
#define PD_FEATURE_MOMENTS_CHUNK 64
typedef struct {
  int D, S, m, degree;
  int64_t N1, N2;
  int64_t f1_stride, f2_stride;
  int64_t idx_stride;
  double gamma, coef0;
  const float* f1; const float* f2;
  const int32_t* idx1; const int32_t* idx2;
  double* sums; double* mmd;
  void* workspace; size_t workspace_bytes;
} pd_kid_mmd_args;
size_t pd_kid_mmd_workspace(int64_t S, int64_t m);
int pd_kid_mmd(const pd_kid_mmd_args* a, void* stream);

typedef struct {
  int D;
  int64_t N;
  int64_t f_stride, cov_stride;
  const float* f;
  double* mean; double* cov;
  void* workspace; size_t workspace_bytes;
} pd_feature_moments_args;
size_t pd_feature_moments_workspace(int64_t N, int D);
int pd_feature_moments(const pd_feature_moments_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_knn_radii, pd_manifold_query (added under ABI 8): the k-nearest-neighbour manifold estimates under improved precision / recall
 * (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) over features that stay on the device, fp64 on
 * v_mfma_f64_16x16x4_f64 from fp32 features (every element widened exactly before any arithmetic).  csrc/manifold_stats.hip; host side
 * phendiff_amd.metrics (knn_radii_device, manifold_query_device, precision_recall_device, density_coverage_device).
 *
 * Everything is in SQUARED distances; no square root is taken anywhere:
 *     d2(a, b) = max(0, |a|^2 + |b|^2 - 2 a.b)
 *   The dot product and both norms come out of the same contraction order (a norm is the Gram entry of a row with itself), so two
 *   bitwise-equal rows give d2 == 0.0 exactly.  A NaN d2 counts as +inf: it is never selected as a neighbour and never counted, whatever
 *   the radius.  A pair's d2 depends on its two rows alone -- not on their position, on `splits`, on the other rows.
 *
 * pd_knn_radii: rad2[i] = the (k + 1)-th smallest value of row i of the d2 matrix of f [N][f_stride] with itself, the diagonal SELECTED to
 *   exactly 0 (the row's own entry takes one place, as in kthvalue(k + 1) over a cdist that includes self).  1 <= k <= PD_MANIFOLD_MAX_K,
 *   k + 1 <= N.  A row with fewer than k + 1 finite distances (a NaN row) gets +inf.
 * pd_manifold_query: for query row j of q [Nq][q_stride] against the references r [Nr][r_stride]:
 *     count[j] = #{ i : d2(q_j, r_i) <= rad2[i] }   (rad2 [Nr], one radius per REFERENCE row; count NULL: not computed, rad2 not read)
 *     dmin2[j] = min_i d2(q_j, r_i)                 (NULL: not written; +inf for a NaN query row)
 *   A NaN in one query row touches only that row's outputs; a NaN reference row is never near anything.
 *
 *   Features: fp32, 16-byte aligned, strides in elements (>= D, multiples of 4); D a multiple of 64 in 64 .. 4096; N, Nq, Nr < 2^31.
 *   splits: a workgroup owns a block of 64 rows and walks one of `splits` ranges of the 64-column tiles, so that a few thousand rows still
 *   fill the device; 0 = the library's default, some S in 1 .. min(column tiles, PD_MANIFOLD_MAX_SPLITS) that is a function of the shapes
 *   only, never of the device (the workspace queries answer for it: what they return for splits = 0 is what they return for that S).
 *   The N x N matrix is never stored: each split leaves its k + 1 candidates (resp. a count and a minimum) per row in the workspace and a
 *   second launch merges them.  No atomics; the reductions are order statistics, integer sums and minima: the outputs are bitwise
 *   reproducible and independent of `splits` and of the order of the reference rows.  Rows at or past N of a ragged tile are not read and
 *   their distances are selected to +inf, never multiplied by zero; nothing outside [N][D] of a strided row is read.
 *   workspace (8-byte aligned, contents irrelevant; S = the splits in effect; 0 for sizes the call refuses):
 *     pd_knn_radii_workspace(N, k, splits)        = 8 (N + N S (k + 1)) bytes           (the norms, the candidates)
 *     pd_manifold_query_workspace(Nq, Nr, splits) = 8 (Nq + Nr + Nq S) + 4 Nq S bytes, rounded up to 8 (norms, minima, counts)
 *   Refused before any launch: null args / pointers, count without rad2, count and dmin2 both NULL, misaligned pointers, a workspace_bytes
 *   below the query's (PD_ERR_ARG); D, the strides, k outside 1 .. 16, k + 1 > N, a size below 1 or at or above 2^31, splits outside
 *   0 .. PD_MANIFOLD_MAX_SPLITS, more than 2^31 - 1 workgroups (PD_ERR_SHAPE). */
#define PD_MANIFOLD_MAX_K 16
#define PD_MANIFOLD_MAX_SPLITS 64
typedef struct {
  int D, k, splits;
  int64_t N, f_stride;
  const float* f;
  double* rad2;
  void* workspace; size_t workspace_bytes;
} pd_knn_radii_args;
size_t pd_knn_radii_workspace(int64_t N, int k, int splits);
int pd_knn_radii(const pd_knn_radii_args* a, void* stream);

typedef struct {
  int D, splits;
  int64_t Nq, Nr, q_stride, r_stride;
  const float* q; const float* r;
  const double* rad2;
  int32_t* count;
  double* dmin2;
  void* workspace; size_t workspace_bytes;
} pd_manifold_query_args;
size_t pd_manifold_query_workspace(int64_t Nq, int64_t Nr, int splits);
int pd_manifold_query(const pd_manifold_query_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pd_comm_*: the data-parallel gradient exchange -- DistributedDataParallel's bucketed all-reduce under accelerator.backward(loss)
 * (train.py:311-326, utils_training.py:436) -- directly on RCCL (loaded at run time; PD_ERR_UNSUPPORTED when librccl.so is absent).
 * One communicator per process / GPU, created on the current device.  Rank 0 draws the id (pd_comm_unique_id); the host program ships
 * the 128 bytes to the other ranks; every rank calls pd_comm_init(id, rank, world, &comm).
 * pd_allreduce_bucket: in-place fp32 sum (mean != 0: then divided by world) of one contiguous bucket on `stream`;
 *   algo 0 = ncclAllReduce, algo 1 = reduce-scatter + all-gather over count / world shards (count % world == 0, else algo 0 is used). */
typedef struct { char bytes[128]; } pd_comm_id;
int pd_comm_unique_id(pd_comm_id* out);
int pd_comm_init(const pd_comm_id* id, int rank, int world, void** comm_out);
int pd_allreduce_bucket(void* comm, float* buf, size_t count, int mean, int algo, void* stream);
/* rank and size as the communicator itself reports them (ncclCommUserRank / ncclCommCount) -- what bench.py prints as `rccl_world_size` */
int pd_comm_query(void* comm, int* rank_out, int* world_out);
int pd_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* PHENDIFF_HIP_H_ */
