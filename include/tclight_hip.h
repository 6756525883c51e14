/* tclight_hip.h -- C ABI of libtclight_hip.so, the MI355X (gfx950) kernels behind TC-Light's hot paths.
 *
 * The reference (Linketic/TC-Light) is pure Python/PyTorch and has no FFI; its drop-in seams are the
 * Python call signatures listed in SURVEY.md 8(b).  Each entry point below names the reference
 * function (file:line under /root/reference) whose arithmetic it replaces; the tc_light_amd Python modules bind
 * them with ctypes and re-exposes the reference's own signatures (INTEGRATION.md shows the stub).
 *
 * Conventions: all pointers are DEVICE pointers unless the name says host (`sched`, `h_*`);
 * plain C types only; every call takes the HIP stream it enqueues on and returns
 * 0 = TCL_OK, 1 = TCL_EINVAL (bad argument / unsupported shape), 2 = TCL_ELAUNCH (HIP error).
 * Calls are asynchronous w.r.t. the host and never allocate; scratch comes from the caller
 * (`ws`, sized by the matching *_workspace_bytes function).  Re-entrant per stream.
 */
#ifndef TCLIGHT_HIP_H
#define TCLIGHT_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif
#ifdef __cplusplus
extern "C" {
#endif

/* ===================================================================== path 2: two-stage optimiser (f32) */
/* warp_flow(frames, past_flows)  utils/flow_utils.py:5-16 -- bicubic(A=-0.75) backward warp, zeros padding,
 * align_corners.  img/out [n,c,h,w]; flow [n,flow_c>=2,h,w] (first two channels used). */
int tcl_warp_flow_fwd(const float* img, const float* flow, float* out, int n, int c, int h, int w, int flow_c, hipStream_t st);
/* autograd of the above w.r.t. img (grid_sample backward): gimg is zeroed then scatter-added. */
int tcl_warp_flow_bwd(const float* gout, const float* flow, float* gimg, int n, int c, int h, int w, int flow_c, hipStream_t st);
/* clamp(bmm(pixels, M[:3,:3]) + M[:3,3], 0, 1)  generate.py:405-407, utils/dataloader.py:38-42.
 * src [N,3,h,w]; idx int32[nb] frame of each output (NULL = identity); expo [N,3,4]; out [nb,3,h,w]. */
int tcl_apply_exposure(const float* src, const int* idx, const float* expo, float* out, int nb, int h, int w, hipStream_t st);
/* clamp(SH2RGB(features_dc)[unq_inv[frame]], 0, 1)  generate.py:499-501,530-531.  The codebook is stored CHANNEL-PLANAR,
 * feat [3,K] (= features_dc.t()), so gathers / scatter-adds of neighbouring pixels are contiguous per channel; inv int32 [N*h*w]. */
int tcl_gather_codebook(const float* feat, const int* inv, const int* fidx, float* out, int nb, int h, int w, size_t K, hipStream_t st);
/* value[0] = 1 - relaxed_ms_ssim(X, Y, data_range=1, start_level=1)  utils/loss_utils.py:125-211; gradX = d value / dX
 * (NULL to skip).  X, Y: `planes` contiguous h*w planes (= batch*channels). */
size_t tcl_msssim_workspace_bytes(int planes, int h, int w);
int tcl_ms_ssim_loss(const float* X, const float* Y, int planes, int h, int w, float* value, float* gradX, void* ws, hipStream_t st);
/* TVLoss(weight)(x) and its gradient  utils/loss_utils.py:324-340.  ws16: 2 KiB of scratch (fixed-point loss accumulators). */
int tcl_tv_loss(const float* x, int b, int c, int h, int w, float weight, float* value, float* grad, void* ws16, hipStream_t st);
/* torch.optim.Adam single-tensor step (generate.py:381,483-487); g is consumed and zeroed. step counts from 1. */
int tcl_adam_step(float* p, float* g, float* m, float* v, size_t n, float lr, float b1, float b2, float eps, int step, hipStream_t st);
/* How the flow term scatters d(loss)/d(warped previous frame) (generate.py:420-427 / :507-514 backward): 1 (default) = through an LDS window per
 * 64x16 pixel tile, flushed once; 0 = every addend straight to global memory.  Integer (fixed-point) sums either way: same bits when W % 64 == 0,
 * the same value up to the f32 rounding of differently grouped partial sums otherwise.  Test / A-B hook (env TCL_FLOW_TILED sets the initial mode). */
int tcl_flow_scatter_mode(int tiled);
/* Per-frame fixed-point scale of that scatter (the reference's float grid_sample backward, utils/flow_utils.py:5-16, has no range limit; the
 * engine's bit-reproducible integer cells do).  flow_shift[f] = min(22, 30 - ceil(log2 L_f)) with L_f = the largest number of masked-in pixels
 * of frame f whose bicubic 4x4 window covers one pixel of frame f-1: with |mask * weight| <= 1 no 32-bit cell can overflow, however strongly the
 * flow converges.  Call once per clip (flows / masks are constants of both stages) and pass flow_shift to the four stage entry points below.
 * flows [N,2,h,w], masks [N,1,h,w]; scratch: (h*w + 1) int32; flow_shift: N int32 (device). */
int tcl_flow_cell_shift(const float* flows, const float* masks, int N, int H, int W, int* scratch, int* flow_shift, hipStream_t st);
/* Are the track ids of every frame pairwise distinct (true of get_flowid's output, utils/flow_utils.py:56-93: a pixel of frame i takes the id
 * of ONE pixel of frame i-1 or a fresh id)?  *result (device int) <- 1 / 0; scratch: K ints.  Stage 2 then accumulates codebook rows one frame
 * at a time without atomics -- bit-reproducible -- by passing ids_unique = 1 below; with 0 it falls back to float atomics (any id layout). */
int tcl_track_ids_unique(const int* unq_inv, int N, int H, int W, size_t K, int* scratch, int* result, hipStream_t st);
/* RGB2SH(torch_scatter.scatter(pixels, unq_inv, reduce='mean'))  generate.py:477-479 -> feat [3,K] planar.  cnt: K floats scratch. */
int tcl_scatter_mean_rgb2sh(const float* img, const int* inv, float* feat, float* cnt, int n, int h, int w, size_t K, int ids_unique, hipStream_t st);

/* Whole-stage drivers: every iteration is enqueued on `st`; no host synchronisation inside.
 * sched (HOST) int32 [iters][batch]: frame ids of each mini-batch, -1 pads a short batch (stands in for
 * DataLoader(shuffle=True), generate.py:363-367).  d_cat (DEVICE) int32 [iters][2*batch]: per iteration
 * [cur(b) | max(cur-1,0)(b) | pad].  losses: device float [iters]. */
size_t tcl_stage_workspace_bytes(int batch, int h, int w);
/* Generator.exposure_align  generate.py:354-451.  exposure [N,3,4] (= eye on entry), g/m/v zero on entry;
 * aligned_out [N,3,h,w] receives OptDataset.exposure_align's result.  lr(it) = get_expon_lr_func(lr_init, lr_final,
 * max_steps = epochs*N/batch)((it / iters_per_epoch) * N / batch + it % iters_per_epoch + 1)  (generate.py:372,394). */
int tcl_exposure_align(const float* edited, const float* flows, const float* masks, const int* flow_shift, int N, int H, int W, const int* sched,
                       const int* d_cat, int iters, int iters_per_epoch, int batch, int epochs, float lr_init, float lr_final, float lambda_dssim,
                       float lambda_flow, float* exposure, float* g, float* m, float* v, float* losses, float* aligned_out,
                       void* ws, hipStream_t st);
/* Generator.unique_tensor_optimization  generate.py:453-533.  feat/g/m/v [3,K] planar, feat initialised by tcl_scatter_mean_rgb2sh;
 * images_out [N,3,h,w] (may be NULL) receives the final gather. */
int tcl_unique_tensor_opt(const float* target, const float* flows, const float* masks, const int* flow_shift, const int* unq_inv, int N, int H, int W,
                          size_t K, int ids_unique, const int* sched, const int* d_cat, int iters, int batch, float feature_lr, float lambda_dssim,
                          float lambda_flow, float lambda_tv, float* feat, float* g, float* m, float* v, float* losses,
                          float* images_out, void* ws, void* lazy_ws, hipStream_t st);
/* lazy_ws (may be NULL): tcl_stage2_lazy_workspace_bytes(K, iters) bytes.  With it (and ids_unique) the dense Adam of generate.py:483-487 is
 * applied LAZILY: a codebook row is only read / written in the iterations whose mini-batch holds it, the steps it skipped in between (pure
 * momentum decay, no gradient) are replayed with the same arithmetic right before it is needed, and one dense pass ends the stage -- the
 * result is bit-identical to stepping all K rows every iteration, at ~(rows of the mini-batch) / K of the optimiser's HBM traffic. */
size_t tcl_stage2_lazy_workspace_bytes(size_t K, int iters);

/* One mini-batch of stage 1 / stage 2, GRADIENT ONLY (forward + backward of generate.py:396-429 / :496-522, no optimiser step): what the
 * whole-stage drivers above run per iteration, exposed so that a multi-GPU host loop can put a collective between the gradient and the
 * Adam step (tc_light_amd/post_opt.py; SURVEY 8(e): the slots of a mini-batch are dealt to the ranks, codebook / exposure gradients meet
 * in reduce_scatter / all_reduce over xGMI, tcl_adam_step updates).  d_cidx (DEVICE) int32 [2*b_loc] = [cur(b_loc) | max(cur-1,0)(b_loc)]
 * for THIS caller's slots; b_glob = slots of the whole mini-batch, nvalid_glob = how many of them have frame id > 0: every mean of the
 * reference's loss runs over the global mini-batch, so the callers' partial gradients and *loss_part values simply add up.
 * g is accumulated into (+=) and must be zero (or hold other slots' partial sums) on entry; ws: tcl_stage_workspace_bytes(b_loc, h, w). */
int tcl_exposure_grad(const float* edited, const float* flows, const float* masks, const int* flow_shift, int N, int H, int W, const int* d_cidx, int b_loc,
                      int b_glob, int nvalid_glob, float lambda_dssim, float lambda_flow, const float* exposure, float* g,
                      float* loss_part, void* ws, hipStream_t st);
int tcl_unique_tensor_grad(const float* target, const float* flows, const float* masks, const int* flow_shift, const int* unq_inv, int N, int H, int W, size_t K,
                           int ids_unique, const int* d_cidx, int b_loc, int b_glob, int nvalid_glob, float lambda_dssim, float lambda_flow,
                           float lambda_tv, const float* feat, float* g, float* loss_part, void* ws, hipStream_t st);

/* ===================================================================== path 1: denoising loop (f16, f32 accumulate)
 * Activations are NHWC / token-major [B, H*W, C] f16 on the device.  These replace the library kernels the reference
 * reaches through diffusers' UNet2DConditionModel / AutoencoderKL (generate.py:342-347; generate_utils.py:144,161). */
/* C[M,N] = act(A[M,K] . W[N,K]^T + bias[N]) + resid[M,N];  act: 0 none, 1 SiLU.  K % 64 == 0; lda, ldw (row strides of A, W
 * in halves) % 8 == 0.  torch.nn.Linear / 1x1 Conv2d.  bias / resid may be NULL.
 * act: 0 none, 1 SiLU, 3 ReLU, 4 GELU (erf), applied to A.W^T + bias before the residual is added; 5 = GELU applied AFTER the residual
 * add (C = gelu(A.W^T + bias + resid), resid required).
 * act 2 = fused GEGLU (diffusers ff.net.0 + GEGLU): W/bias rows must be pre-arranged in 64-row groups [32 value rows | the 32
 * matching gate rows]; C is [M, N/2] = value * gelu(gate); N % 64 == 0, no resid. */
int tcl_gemm_f16(const void* A, const void* W, const void* bias, const void* resid, void* C, int M, int N, int K, int lda, int ldw,
                 int ldc, int ldr, int act, hipStream_t st);
/* Register caller-owned device scratch for split-K partial sums (used by tcl_gemm_f16 / tcl_conv3x3_f16 when the tile grid
 * would leave most CUs idle).  NULL disables split-K.  All calls that use it must be issued on one stream. */
int tcl_set_workspace(void* ws, size_t bytes);
/* Tuning / test hook: force the kernel configuration (cfg ids: the tile table g_tiles in csrc/gemm.hip; 0 = automatic choice) and the number of K
 * splits (0/1 = none) for every following tcl_gemm_f16 / tcl_conv3x3_f16 call; calls the forced configuration cannot serve
 * return TCL_EINVAL.  Process-global, not thread-safe. */
int tcl_gemm_tune(int cfg, int splits);
/* Automatic configuration choice (default on): the first call with a new problem shape times the candidate tile
 * configurations on the caller's stream (synchronising it once) and caches the winner for the life of the process; results are
 * bit-identical whichever candidate wins (the K-split count is a fixed function of the shape).  0 = static heuristic only and
 * drops the cache. */
int tcl_gemm_autotune(int enable);
/* Persistent tile table (text, one line per problem shape).  _load merges a file into the cache (entries are re-validated against each
 * call's leading dimensions before use); _save writes the cache; _size = entries.  tcl_gemm_autotune(2) = table-only mode: shapes missing
 * from the table take the static heuristic instead of being timed -- no host synchronisation in the hot loop and the same tile (hence the
 * same bits, run to run) for a given shape.  tc_light_amd/unet.py loads tc_light_amd/gemm_tune_gfx950.txt at start-up when it exists. */
int tcl_gemm_tune_save(const char* path);
int tcl_gemm_tune_load(const char* path);
size_t tcl_gemm_tune_size(void);
/* Host-only query: which tile configuration (*cfg, an id of the table in csrc/gemm.hip) and how many K splits (*splits) a tcl_gemm_f16 /
 * tcl_conv3x3_f16 call with these scalar arguments gets under the current workspace, forced configuration, table and autotune mode.  resid: 0 = none,
 * 1 = a separate tensor, 2 = in place (resid == C / Y).  *cfg = 0: the tuner would time the shape on first use.  It is the dispatcher's own choice
 * function, asked without operands: nothing is launched and no device memory is touched, so it runs on a machine without a GPU.  TCL_EINVAL where the
 * call itself would return it. */
int tcl_gemm_plan(int M, int N, int K, int lda, int ldw, int ldc, int ldr, int act, int resid, int* cfg, int* splits);
int tcl_conv3x3_plan(int B, int Hin, int Win, int Cin, int Cout, int stride, int pad, int Hup, int Wup, int act, int resid, int* cfg, int* splits);
/* 3x3 Conv2d as implicit GEMM on NHWC: X [B,Hin,Win,Cin], W [Cout, 9*Cin] (tap-major: (ky*3+kx)*Cin + c), Y [B,Hout,Wout,Cout].
 * pad=1: padding 1 (UNet ResnetBlock2D / Downsample2D stride 2); pad=0 with stride 2: the VAE encoder's (0,1,0,1) padding.
 * Hup/Wup > 0: the input is first nearest-upsampled to Hup x Wup (Upsample2D with explicit output size), fused in the gather. */
int tcl_conv3x3_f16(const void* X, const void* W, const void* bias, const void* resid, void* Y, int B, int Hin, int Win, int Cin,
                    int Cout, int stride, int pad, int Hup, int Wup, int act, hipStream_t st);

/* torch.nn.GroupNorm(groups, C1+C2, eps) [+ SiLU] over x = cat([x1, x2], channel) (x2 may be NULL with C2 = 0): the
 * ResnetBlock2D / Transformer2DModel / AutoencoderKL norms, with the up-block skip concat folded in.  y [B,HW,C1+C2].
 * ws: tcl_groupnorm_workspace_bytes(B, C) bytes of scratch (per-block partial sums).  Deterministic: no float atomics -- the same
 * input gives the same bits on every run. */
size_t tcl_groupnorm_workspace_bytes(int B, int C);
int tcl_groupnorm_f16(const void* x1, int C1, const void* x2, int C2, const void* gamma, const void* beta, void* y, int B, int HW,
                      int groups, float eps, int silu, void* ws, hipStream_t st);
/* The same with a second output: yraw [B,HW,C1+C2] (may be NULL) receives the un-normalised channel concat cat([x1, x2]) -- the operand of the
 * up-block ResnetBlock2D's conv_shortcut (diffusers ResnetBlock2D.forward: `input_tensor = conv_shortcut(input_tensor)` on the concatenated
 * input) -- from the pass that reads x1 / x2 anyway, instead of a concat pass of its own (tcl_concat_channels_f16).
 * Channel groupings (both entries): groups <= 64, C % groups == 0, cpg = C / groups >= 4, C1 and C2 multiples of 8, and NO 8-channel chunk [8k, 8k + 8)
 * may touch three groups -- the kernels split a chunk once, between the group of its first and the group of its last channel.  A chunk that starts
 * off = 8k mod cpg channels into a group touches three when 2*cpg - off < 8; of the admitted cpg only 5 has such an offset (off = 3 at channel 8 of
 * C = 160, groups = 32).  Such a grouping returns TCL_EINVAL before any launch, like every other unsupported shape; nothing is written. */
int tcl_groupnorm_concat_f16(const void* x1, int C1, const void* x2, int C2, const void* gamma, const void* beta, void* y, void* yraw, int B, int HW,
                             int groups, float eps, int silu, void* ws, hipStream_t st);
/* torch.nn.LayerNorm(C) (BasicTransformerBlock.norm1/2/3). */
int tcl_layernorm_f16(const void* x, const void* gamma, const void* beta, void* y, long rows, int C, float eps, hipStream_t st);
/* The same, plus metric = y / |y| per row with tcl_tome_normalize_f16's f16 arithmetic (norm1 of a VidToMe-patched block, patch.py:161-166 ->
 * merge.py:84: the matching metric of the block's tokens, produced while they are in registers). */
/* C = act(LayerNorm(x; gamma, beta, eps) . W^T + bias) (+ resid): norm2 -> attn2.to_q and norm3 -> ff.net.0 (GEGLU, act 2) of BasicTransformerBlock
 * (generate.py:342-347 -> diffusers) in one kernel, for K = 320 (the level-0 blocks; other widths: tcl_layernorm_f16 + tcl_gemm_f16).  The
 * normalised activations are rounded to f16 exactly as tcl_layernorm_f16 rounds them; the f32 statistics are summed in another order (not bit-identical
 * to the two-kernel route, 1e-3 rel-L2 like any two f16 LayerNorms).  N >= 128, N % 32 == 0 (GEGLU: % 64), 16-B aligned rows. */
int tcl_ln_gemm_f16(const void* x, const void* gamma, const void* beta, float eps, const void* W, const void* bias, const void* resid, void* C,
                    int M, int N, int K, int ldx, int ldw, int ldc, int ldr, int act, hipStream_t st);
/* The attn2 `to_q` projection of a C = 320 transformer block written straight into the attention kernel's query panel (diffusers Attention.to_q ->
 * AttnProcessor2_0, utils/model_utils.py:66-67): LayerNorm(x) @ W^T -> ws_q's Qp [B, H, ceil256(Tq), 48], pre-scaled by scale * log2 e, exactly as
 * tcl_attention_pack_f16 would have packed the Linear's output (same rounding points), without the [M, H d] round trip.  M = B * Tq rows, d = 40.
 * Rows Tq .. ceil256(Tq) of every (b, h) panel are NOT written: the caller keeps ws_q (tcl_attention_q_bytes) zero-initialised and reuses it.
 * Follow with tcl_attention_f16(..., TCL_ATTN_PREPACKED, ws_q, ws_kv). */
int tcl_ln_gemm_qpanel_f16(const void* x, const void* gamma, const void* beta, float eps, const void* W, int M, int H, int d, int Tq, int ldx, int ldw,
                           float scale, void* ws_q, hipStream_t st);
/* attn1's fused QKV projection of a VidToMe-merging block written straight into the attention panels (patch.py:170-176: `attn1(norm_hidden_states)` over the
 * merged tokens; diffusers Attention.to_q / to_k / to_v, no bias): x [ne*T, K] @ W[3 H d, K]^T -> Qp / Kp / V^T panels in ws_q / ws_kv with exactly the
 * (entry b's rows start x_bs elements after entry b-1's; row_index != NULL: token t is row row_index[t] of its entry's block -- the merge map of
 * merge.py's "replace" mode applied in the operand load instead of by a gather pass)
 * bytes tcl_attention_pack_f16 would have written from the [ne*T, 3 H d] product (d = 40 or 80).  ws_q / ws_kv: tcl_attention_q_bytes / _kv_bytes(ne, H, T, d),
 * ZERO-INITIALISED once per (ne, H, T, d) by the caller and reusable by stream-ordered calls of that shape (padding is never written).  Follow with
 * tcl_attention_f16(..., TCL_ATTN_PREPACKED [| TCL_ATTN_PAIR], ws_q, ws_kv). */
int tcl_gemm_qkv_panels_f16(const void* x, long x_bs, const int* row_index, const void* W, int ne, int T, int H, int d, int K, int ldx, int ldw, float scale,
                            void* ws_q, void* ws_kv, hipStream_t st);
int tcl_layernorm_metric_f16(const void* x, const void* gamma, const void* beta, void* y, void* metric, long rows, int C, float eps, hipStream_t st);
/* diffusers GEGLU: in [rows, 2D] -> out [rows, D] = in[:, :D] * gelu(in[:, D:]) (exact erf gelu). */
int tcl_geglu_f16(const void* in, void* out, long rows, int D, hipStream_t st);
/* in-place softmax(scale * x) over rows of length T (VAE mid-block single-head attention). */
int tcl_softmax_rows_f16(void* x, long rows, int T, int ld, float scale, hipStream_t st);
int tcl_concat_channels_f16(const void* x1, int C1, const void* x2, int C2, void* y, long rows, hipStream_t st);
/* im2col for 3x3/pad-1 convs with tiny Cin (IC-Light conv_in 8->320, utils/model_utils.py:21-26; VAE 3->128, 4->512). */
int tcl_im2col3x3_small_f16(const void* x, void* out, int B, int H, int W, int Cin, int Kpad, hipStream_t st);
/* y = f16(act_out(W . act_in(x) + bias)) + add : time_embedding MLP and ResnetBlock2D.time_emb_proj (M = 1). */
int tcl_gemv_f16(const void* W, const void* x, const void* bias, const void* add, void* y, int N, int K, int silu_in, int silu_out, hipStream_t st);
/* diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin]. */
int tcl_timestep_embed_f16(float t, int dim, void* out, hipStream_t st);
/* Generator.pred_noise input assembly (generate.py:295-298 + model_utils.py:35-40): latents x / concat_conds [N,4,h,w] f16 ->
 * UNet input [2F,H',W',8] NHWC.  mode 0: xy-plane, idx = frame ids; mode 1: yt-plane ('n c h w -> w c n h', generate.py:267),
 * idx = latent columns, frames sl..sl+nwin. */
int tcl_pack_latents_f16(const void* x, const void* cond, const int* idx, int F, int mode, int sl, int nwin, int h, int w, void* out, hipStream_t st);
/* The same assembly for the background-conditioned IC-Light model (utils/model_utils.py:97-179, init_iclight_bg: a 12-channel conv_in, and
 * `torch.cat([sample, c_concat], dim=1)` of its hooked forward with c_concat = foreground latent | background latent): x / cond_fg [N,4,h,w] f16,
 * cond_bg [bg_frames,4,h,w] f16 -> out [2F,H',W',12] NHWC, channels 0-3 x, 4-7 cond_fg, 8-11 cond_bg, both CFG halves written (cfg_pair holds).  Modes,
 * idx, sl, nwin as tcl_pack_latents_f16.  bg_frames == 1: the one background latent is read for every frame (never repeated in memory); any other
 * value is the frame count N of cond_bg, the same as x's.  Records are 24 B: one 16 B and one 8 B store per pixel; `out` 8 B aligned.
 * TCL_EINVAL: null pointers, F <= 0, h, w <= 0, another mode, a misaligned out, bg_frames < 1, and in yt mode nwin <= 0, sl < 0 or a per-frame
 * background shorter than the window (1 < bg_frames < sl + nwin).  N itself is not an argument (as in the 8-channel entry), so in xy mode a
 * bg_frames other than 1 or N is the caller's to refuse (Generator does). */
int tcl_pack_latents12_f16(const void* x, const void* cond_fg, const void* cond_bg, int bg_frames, const int* idx, int F, int mode, int sl, int nwin,
                           int h, int w, void* out, hipStream_t st);
/* CFG combine uncond + g*(cond - uncond) (generate.py:349-350) scattered back to noises[N,4,h,w]; in mode 1 frames
 * n < scale_upto are multiplied by `scale` (the sqrt(0.5) overlap rule, generate.py:276-278) and only the first nkeep
 * frames of the window are written (the rest is overwritten by the next window in the reference's sequential order). */
int tcl_unpack_cfg_f16(const void* eps, const int* idx, int F, int mode, int sl, int nwin, int h, int w, float guidance, int scale_upto,
                       float scale, int nkeep, void* noise, hipStream_t st);
/* noises_t <- AdaIN(noises_t, noises); noises <- sqrt(a)*noises_t + sqrt(1-a)*noises  (generate.py:281-282,
 * utils/general_utils.py:137-156).  planes = N*4, hw = h*w. */
int tcl_adain_fuse_f16(void* noises_t, void* noises, int planes, int hw, float alpha, hipStream_t st);
/* DPMSolverMultistepScheduler.step, sde-dpmsolver++ (generate.py:235): m0 <- x0 = (x - sigma_t*eps)/alpha_t;
 * x <- ca*x + cb0*m0 + cb1*m1 + cc*z (coefficients from tc_light_amd/scheduler.py; f32 math; m1/z may be NULL). */
int tcl_dpm_sde_step_f16(void* x, const void* eps, float* m0, const float* m1, const void* z, long n, float sigma_t, float alpha_t, float ca,
                         float cb0, float cb1, float cc, hipStream_t st);
/* DDIM inversion of the IC-Light UNet (invert.py:151-244; tc_light_amd/invert.py).  The master latents x [N,4,h,w] stay f32 on the device; slot j of a
 * group serves frame idx[j] (F physical slots: both halves of the pair batch, an odd group's duplicate included).  A slot whose idx is outside [0, N) is
 * skipped.  h, w <= 0, F <= 0, N <= 0 and null pointers return TCL_EINVAL.
 * tcl_invert_pack_f16 (replaces `torch.cat([x, concat_conds], dim=1)` of model_utils.py:35-40 and the NCHW -> NHWC cast): out [F,h,w,8] f16 NHWC,
 * channels 0-3 = f16(x[idx[j]]), channels 4-7 = cond[idx[j]] (cond [N,4,h,w] f16). */
int tcl_invert_pack_f16(const float* x, const void* cond, const int* idx, int N, int F, int h, int w, void* out, hipStream_t st);
/* tcl_ddim_step_f32 (replaces pred_next_x, invert.py:215-244): eps [F,h,w,4] f16 NHWC as the UNet returns it; the first F_valid slots are applied
 * (0 < F_valid <= F; their idx entries are distinct).  mu = sqrt(alpha_t), sigma = sqrt(1 - alpha_t), *_prev the same of alpha_t_prev (host, f64 -> f32;
 * mu, mu_prev > 0).  In f32, no fma contraction, IEEE division:  x0 = (x - s_a*eps) / m_a;  x = m_b*x0 + s_b*eps  with (a, b) = (prev, t) when
 * `inversion` and (t, prev) otherwise (invert.py:237-242).  x is updated in place and f16(x) goes into channels 0-3 of record j of xin [F,h,w,8] f16
 * (the UNet input tcl_invert_pack_f16 wrote; channels 4-7 are left alone), so the next step needs no repack. */
int tcl_ddim_step_f32(float* x, const void* eps, const int* idx, int N, int F, int F_valid, int h, int w, float mu, float sigma, float mu_prev,
                      float sigma_prev, int inversion, void* xin, hipStream_t st);
/* IC-Light's "Lighting Preference" start (gradio_demo_iclight.py:235-299: bg_source, lowres_denoise, the img2img call; csrc/light.hip).
 * tcl_light_gradient_f32: out [3,H,W] f32 (16 B aligned) = u/254, the same plane three times, u = uint8(np.linspace(255, 0, W)) along x for
 * TCL_LIGHT_LEFT, (0, 255, W) for RIGHT, the same over H along y for TOP / BOTTOM -- linspace in f64 as start + i*step with
 * step = (stop - start)/(n - 1), no fma contraction, the last sample = stop, n == 1 -> start; truncated to uint8.  u/254 is the [0,1]-convention
 * image whose 2x - 1 (VAEEngine.encode) is the demo's u/127 - 1 (numpy2pytorch).  H, W <= 0, 3*H*W >= 2^31 - 3 or another side return TCL_EINVAL. */
enum { TCL_LIGHT_LEFT = 0, TCL_LIGHT_RIGHT = 1, TCL_LIGHT_TOP = 2, TCL_LIGHT_BOTTOM = 3 };
int tcl_light_gradient_f32(float* out, int H, int W, int side, hipStream_t st);
/* tcl_light_start_f16 (the img2img pipeline's scheduler.add_noise at the first executed sigma): out [N,chw] f16, x0 f16, z f32;
 * out[n][i] = f16(fl32(fl32(alpha*x0[n*x0_stride + i]) + fl32(sigma_t*z[n*z_stride + i]))) -- no contraction, one rounding to f16.  Strides are in
 * elements per frame, 0 broadcasts one frame to all N (x0: the gradient's latent; z: noise_mode "same"), otherwise >= chw.  Any chw > 0; 16 B
 * accesses when chw and the strides are multiples of 8 and the pointers 16 B aligned.  alpha = 1/sqrt(sigma^2 + 1), sigma_t = sigma*alpha (host f64 -> f32). */
int tcl_light_start_f16(void* out, const void* x0, long x0_stride, const float* z, long z_stride, int N, long chw, float alpha, float sigma_t,
                        hipStream_t st);
/* Inputs of the background-conditioned model (generation.iclight_model: fbc; IC-Light's background demo, whose constants are restated in DESIGN
 * section 6; csrc/light.hip).
 * tcl_bg_ramp_f32 (replaces the demo's `np.linspace(start, stop, n)` tiled to an image for bg_source left / right / top / bottom / grey): out
 *   [3,H,W] f32 (16 B aligned) = u/254, the same plane three times, u = uint8(np.linspace(start, stop, n)) with start at index 0 of the axis `side`
 *   names (x, n = W for TCL_LIGHT_LEFT / RIGHT; y, n = H for TOP / BOTTOM) -- the linspace rule of tcl_light_gradient_f32.  start == stop is a
 *   constant image.  start, stop outside [0, 255] and whatever tcl_light_gradient_f32 refuses return TCL_EINVAL.
 * tcl_matte_grey_f32 (replaces the demo's run_rmbg composite `127 + (img - 127) * alpha` clipped to uint8, and numpy2pytorch): frames [n,3,H,W]
 *   f32 in [0,1], alpha [n,1,H,W] f32 (RMBGEngine.estimate_alpha) -> out [n,3,H,W] f32.  Per channel in f32, no fma contraction: u = 255 f;
 *   v = 127 + (u - 127) a; q = trunc(clamp(v, 0, 255)) (NaN -> 0); out = q/254, whose 2x - 1 (VAEEngine.encode) is the demo's q/127 - 1.  16 B
 *   accesses when H*W % 4 == 0 and the three pointers are 16 B aligned. */
int tcl_bg_ramp_f32(float* out, int H, int W, int side, int start, int stop, hipStream_t st);
int tcl_matte_grey_f32(const float* frames, const float* alpha, float* out, int n, int H, int W, hipStream_t st);
/* generation.normal: the background demo's "Compute Normal" (process_normal) on the fbc model -- four relights of one foreground under the left /
 * right / bottom / top ramps, one seed, turned into a surface normal (csrc/light.hip).
 * tcl_matte_grey_sigma_f32 (the demo's run_rmbg(img, sigma=16)): tcl_matte_grey_f32 with v = 127 + ((u - 127) + sigma) a -- the same f32 operation
 *   order, no fma contraction, q = trunc(clamp(v, 0, 255)) (NaN -> 0), out = q/254.  (u - 127) + 0 is exact, so sigma = 0 is tcl_matte_grey_f32 bit for
 *   bit.  A NaN sigma returns TCL_EINVAL.
 * tcl_fbc_normal: left / right / bottom / top [n,3,H,W] f32 (what VAEEngine.decode_latents_batch returns), alpha [n,1,H,W] f32 or NULL (= 1
 *   everywhere) -> normal_u8 [n,H,W,3] u8 (required; RGB = (u, v, h)), normal_f32 [n,3,H,W] f32 and ambient [n,3,H,W] f32 (each may be NULL).  Per
 *   pixel in f32, no fma contraction, IEEE division and square root; L, R, B, T = the inputs clamped to [0,1], NaN -> 0.  Per channel c:
 *   A = (((L+R)+B)+T) * 0.25;  q(X) = (X + e)/(A + e) - 1, e = 1e-5f;  u_c = (q(R) - q(L)) * 0.5;  v_c = (q(T) - q(B)) * 0.5.  Across channels:
 *   u = ((u_0+u_1)+u_2)/3, v likewise;  s = clamp((1 - u*u) - v*v, 0, 1e5);  h = s^5 as s2 = s*s, s4 = s2*s2, h = s4*s (the demo's exponent
 *   0.5 * sigma with sigma = 10; no powf);  len = sqrt((u*u + v*v) + h*h);  N = (u, v, h)/len;  m = trunc(clamp(alpha*255, 0, 255))/255 (the demo's
 *   u8 round trip of the matte; its Lanczos resize is the identity at the working size);  out = N*m + (0, 0, 1)*(1 - m);
 *   normal_u8 = trunc(clamp(out*127.5 + 127.5, 0, 255));  normal_f32 = out;  ambient = A per channel.
 *   Bounds the design rests on: every clamped relight is at most 4A, so q lies in [-1, 3]; u^2 + v^2 + h^2 >= 0.30 (the minimum of r + (1 - r)^10
 *   over r = u^2 + v^2), so no division can produce NaN or Inf for finite input.
 *   One thread handles four consecutive pixels of a frame and issues all its loads before the arithmetic; 16 B loads when H*W % 4 == 0, the f32
 *   pointers are 16 B and normal_u8 4 B aligned, a scalar path otherwise.  Null required pointers, n, H, W <= 0 and 3*n*H*W >= 2^31 return TCL_EINVAL. */
int tcl_matte_grey_sigma_f32(const float* frames, const float* alpha, float* out, int n, int H, int W, float sigma, hipStream_t st);
int tcl_fbc_normal(const float* left, const float* right, const float* bottom, const float* top, const float* alpha, void* normal_u8,
                   float* normal_f32, float* ambient, int n, int H, int W, hipStream_t st);
/* generation.light_path: a light whose direction moves over the clip -- one ramp per frame at an arbitrary angle (csrc/light.hip).
 * tcl_light_ramp_angle_f32: dir is a DEVICE array [N,2] f64 of (c, s) per frame, the unit vector of the frame's angle (hostlogic.light_dirs; the
 *   angle names the side the light comes FROM: 0 left, 90 top, 180 right, 270 bottom); out [N,3,H,W] f32 = u/254 (one f32 division), the same plane
 *   three times -- the [0,1] convention of tcl_light_gradient_f32.  Per pixel (x, y), every operation in f64 rounded on its own (no fma contraction),
 *   IEEE division:  px = x - (W-1)/2;  py = y - (H-1)/2;  d = px*c + py*s;  R = (|c|*(W-1) + |s|*(H-1))/2;  t = (R - d)/(2R);  when R == 0 (a
 *   single sample along the light's axis) t = ((|c| + |s|) + (c + s)) / (2(|c| + |s|)), the origin corner of a square image: np.linspace(start,
 *   stop, 1) keeps the FIRST sample, and this is exactly 1 at 0 / 90 and 0 at 180 / 270, the level the two entries above give at n == 1;
 *   v = lo + (hi - lo)*t;  u = trunc(clamp(v, 0, 255)).  hi is met at the corner nearest the light, lo at the opposite one.  fc passes the levels of
 *   tcl_light_gradient_f32 (255, 0), fbc those of the bg_source ramps (224, 32).
 *   In real arithmetic the formula at 0 / 90 / 180 / 270 is the linspace rule of the two entries above; the roundings differ (isolated pixels, at
 *   most one level) -- so the caller (Generator.light_ramps) takes the existing entries for frames whose reduced angle is an exact multiple of 90,
 *   and a constant path reproduces left / top / right / bottom bit for bit.
 *   One launch for all N frames; a pixel's value is computed once and stored to the three planes, as 16 B stores when H*W % 4 == 0 and out is 16 B
 *   aligned, element by element otherwise.  Null pointers, N, H, W <= 0, 3*N*H*W >= 2^31, a level outside [0, 255] or hi < lo return TCL_EINVAL;
 *   non-finite dir entries are the caller's to refuse (hostlogic.check_light_path). */
int tcl_light_ramp_angle_f32(float* out, const double* dir, int N, int H, int W, int hi, int lo, hipStream_t st);
/* The highres pass (gradio_demo_iclight.py:301-334: highres_scale, highres_denoise; csrc/resize.hip): decoded frames -> u8 -> PIL's LANCZOS resize
 * -> the [0,1]-convention image the VAE encoder takes.
 * tcl_frames_to_u8: frames [N,3,H,W] f32 (what VAEEngine.decode returns) -> out [N,H,W,3] u8, u = trunc(clamp(fl32(255*p), 0, 255)): one f32 product
 *   (no fma contraction), clamp, truncation; NaN -> 0.  16 B loads when H*W % 4 == 0 and frames is 16 B aligned.  3*N*H*W >= 2^31 returns TCL_EINVAL.
 * tcl_u8_to_frames_f32: u8 [N,H,W,3] -> out [N,3,H,W] f32 = u / denom (one IEEE division; denom 254: the demo's u/127 - 1 under VAEEngine.encode's 2x - 1).
 * tcl_resize_lanczos_table (HOST, no device work): the table of one axis resampled from `in` to `out` samples, PIL's precompute_coeffs +
 *   normalize_coeffs_8bpc operation for operation in f64 with the C library's sin: scale = in/out, filterscale = max(scale, 1), support = 3*filterscale,
 *   ksize = 2*ceil(support) + 1, window int(center -/+ support + 0.5) clamped to [0, in], Lanczos-3 weights normalised by their sum and rounded half
 *   away from zero to 22-bit fixed point.  h_table: out*2 ints (first input index, tap count) followed by out*ksize ints (taps, zero past the count);
 *   tcl_resize_lanczos_table_ints(in, out) = out*(2 + ksize) is its length, 0 for in == out (that axis is not resampled) or an unsupported ratio.
 * tcl_resize_lanczos_u8: src [N,H,W,3] u8 -> dst [N,Ho,Wo,3] u8, bit-identical to PIL.Image.resize((Wo, Ho), Image.LANCZOS) frame by frame:
 *   accumulators start at 1 << 21, are shifted right by 22 and clipped to u8, the horizontal pass is clipped to u8 before the vertical pass, an axis
 *   whose size does not change is not resampled (both: a copy).  tx / ty (DEVICE): the tables of the W -> Wo and H -> Ho axes (ignored, may be NULL, for an
 *   unchanged axis).  Per-axis in/out from 0.25 to 2; other ratios, null pointers, non-positive sizes, N > 65535 and 3*N*Ho*Wo >= 2^31 return TCL_EINVAL. */
int tcl_frames_to_u8(const float* frames, void* out, int N, int H, int W, hipStream_t st);
int tcl_u8_to_frames_f32(const void* u8, float* out, int N, int H, int W, float denom, hipStream_t st);
size_t tcl_resize_lanczos_table_ints(int in, int out);
int tcl_resize_lanczos_table(int in, int out, int* h_table);
int tcl_resize_lanczos_u8(const void* src, void* dst, int N, int H, int W, int Ho, int Wo, const int* tx, const int* ty, hipStream_t st);
/* layout conversions around the VAE (generate_utils.py:140-172): 2*img-1 -> NHWC8 f16; clamp(y/2+0.5) -> [B,3,H,W] f32.
 * ldc = row stride in halves, >= the channels read or written (tcl_nchw_to_nhwc_f16 zeroes columns C..ldc-1); empty batches and narrower strides
 * return TCL_EINVAL.  tcl_transpose_f16: in [batch,R,ldi] -> out [batch,Cc,ldo], ldi >= Cc, ldo >= R, padding columns of out are left untouched. */
int tcl_img_to_nhwc8_f16(const float* img, void* out, int B, int HW, hipStream_t st);
int tcl_nhwc_to_img_f32(const void* y, int ldc, float* img, int B, int HW, hipStream_t st);
int tcl_nhwc_to_nchw_f16(const void* y, int ldc, void* out, int B, int C, int HW, float scale, hipStream_t st);
int tcl_nchw_to_nhwc_f16(const void* x, void* out, int ldc, int B, int C, int HW, float scale, hipStream_t st);
int tcl_transpose_f16(const void* in, void* out, int batch, int R, int Cc, int ldi, int ldo, hipStream_t st);
/* 1x1 Conv2d with <= 8 channels (AutoencoderKL quant_conv 8->8 / post_quant_conv 4->4): y[m, :Co] = W[Co,Ci] x[m, :Ci] + b;
 * columns Co..ldo-1 of y are zeroed. */
int tcl_conv1x1_small_f16(const void* x, int ldi, const void* W, const void* b, void* y, int ldo, long M, int Ci, int Co, hipStream_t st);

/* softmax(Q K^T * scale) V per head, flash style (torch SDPA / xformers via AttnProcessor2_0: attn1 on the VidToMe-merged
 * tokens, patch.py:170-176, and attn2 text cross-attention).  q/k/v/o point at head 0 of batch 0 with heads interleaved
 * in channels (head hh = channels [hh*d, (hh+1)*d)); ld* row strides and *bs batch strides in halves; d in {40, 80, 160}.
 * K/V batch = b / kv_div.  pack_kv is a set of TCL_ATTN_* bits.  Without TCL_ATTN_PACK_KV the call reuses the K/V panels a previous call left in ws_kv
 * (text K/V are constant per run).  TCL_ATTN_PAIR: the B samples are one half of an identical pair (the CFG halves before the first text cross-attention):
 * the kernel variant is chosen as for 2 B samples, so the half alone gives the bits the full batch would have given.  TCL_ATTN_PREPACKED: the panels in
 * ws_q / ws_kv were already written by tcl_attention_pack_f16 (same arguments; e.g. on another stream, with the caller's event between the two) or by a
 * panel-writing GEMM: only the attention kernels run.
 * ws_q (tcl_attention_q_bytes): packed Q panel + one int per 128-query block (head_dim 40, large launches: blocks whose speculative
 * softmax left the f16 range are flagged there and redone by the exact-maximum kernel of the same call); no initialisation needed. */
enum { TCL_ATTN_PACK_KV = 1, TCL_ATTN_PAIR = 2, TCL_ATTN_PREPACKED = 4 };
size_t tcl_attention_q_bytes(int B, int H, int Tq, int d);
size_t tcl_attention_kv_bytes(int Bkv, int H, int Tk, int d);
int tcl_attention_f16(const void* q, int ldq, long qbs, const void* k, int ldk, long kbs, const void* v, int ldv, long vbs, void* o, int ldo,
                      long obs, int B, int H, int Tq, int Tk, int d, float scale, int kv_div, int pack_kv, void* ws_q, void* ws_kv,
                      hipStream_t st);
/* Which flash kernel tcl_attention_f16 takes for this call (flags: the TCL_ATTN_* bits), asked on the host alone: out4 = (variant id, blocks of its launch,
 * blocks of the flag-gated exact launch behind the speculative head_dim-40 kernel or 0, dynamic LDS bytes).  Variant ids: 0 d40 two query blocks speculative,
 * 1 d40 two query blocks exact, 2 d40 one query block, 3 d80, 4 d128, 5 d160.  Refuses what tcl_attention_f16 refuses. */
int tcl_attention_plan(int B, int H, int Tq, int Tk, int d, int kv_div, int flags, int* out4);
/* The packing half of tcl_attention_f16 alone: Q panel (scaled) into ws_q and, with TCL_ATTN_PACK_KV, the K / V^T panels into ws_kv. */
int tcl_attention_pack_f16(const void* q, int ldq, long qbs, const void* k, int ldk, long kbs, const void* v, int ldv, long vbs, int B, int H, int Tq,
                           int Tk, int d, float scale, int kv_div, int pack_kv, void* ws_q, void* ws_kv, hipStream_t st);
/* tcl_attention_f16 with a K / V entry PER SAMPLE (generation.prompt_path: the text cross-attention where every frame has its own text, and the chunks
 * of a pass draw frames in no order a `b / kv_div` could express).  kv_index: DEVICE int32 [B], sample b attends to entry kv_index[b] of the kv_rows
 * entries in ws_kv (tcl_attention_kv_bytes(kv_rows, H, Tk, d); with TCL_ATTN_PACK_KV they are packed from k / v [kv_rows, Tk, ...] by this call);
 * h_kv_index: a HOST copy of the same table, checked here -- an entry outside [0, kv_rows) returns TCL_EINVAL and nothing is launched (the device
 * never checks).  kv_div is not consulted then; d in {40, 80, 160}.  The kernels are those of tcl_attention_f16, chosen by the same rule, with the
 * entry read by a per-block scalar load: a sample's arithmetic is what it is when its entry is handed over through kv_div, bit for bit.
 * kv_index == NULL: the call IS tcl_attention_f16 (same kernels, `b / kv_div`), h_kv_index and kv_rows are not looked at. */
int tcl_attention_kvindex_f16(const void* q, int ldq, long qbs, const void* k, int ldk, long kbs, const void* v, int ldv, long vbs, void* o, int ldo,
                              long obs, int B, int H, int Tq, int Tk, int d, float scale, int kv_div, int pack_kv, void* ws_q, void* ws_kv,
                              const int* kv_index, const int* h_kv_index, int kv_rows, hipStream_t st);
/* generation.prompt_path: the text conditioning of F frames between keyframe prompts, one launch (csrc/text_lerp.hip).  keys [n_keys, LD] f16: the
 * keyframes' CLIP last_hidden_state (LD = L * D elements each); out [F, LD] f16.  tab: DEVICE int32 [F, 3] = (k0, k1, the bits of t as f32) per frame,
 * h_tab a HOST copy of it, checked here: k0, k1 outside [0, n_keys) or t outside [0, 1] (NaN included) return TCL_EINVAL and nothing is launched.
 * Per element, with a = keys[k0][i], b = keys[k1][i], every operation rounded to f32 on its own (no fma contraction), one rounding to f16:
 *   a32 = f32(a);  b32 = f32(b);  e = b32 - a32;  m = t * e;  s = a32 + m;  out[f][i] = f16(s).
 * t == 0 copies the f16 bits of keys[k0], t == 1 those of keys[k1] (the formula would turn -0 into +0, and a + 1 (b - a) need not be b).
 * t is computed by the caller in f64 and rounded to f32 once.  16 B accesses when LD % 8 == 0 and out / keys are 16 B aligned.  F <= 65535. */
int tcl_text_lerp_f16(void* out, const void* keys, int n_keys, const int* tab, const int* h_tab, int F, long LD, hipStream_t st);
/* generation.ip_adapter: IP-Adapter's decoupled image cross-attention (Ye et al. 2023, eq. 5), added in place into the output of the text
 * cross-attention (csrc/ip_attn.hip):  a += ip_scale * softmax(q K_ip^T * qk_scale) V_ip  per (sample, head).
 * q [B, Tq, H*d] f16 (row stride ldq, sample stride qbs, in halves): the UN-scaled query the text attention consumed.  kv_ip [B / kv_div, Tip, 2*H*d]
 * f16, K | V per token; sample b reads entry b / kv_div.  a [B, Tq, H*d] f16 (lda, abs_): read and written.  1 <= Tip <= 16, d in {40, 80, 160},
 * H <= 8 a power of two, B % kv_div == 0, strides multiples of 8 halves and the three bases 16 B aligned: anything else returns TCL_EINVAL before a
 * launch.  ip_scale == 0 returns 0 without a launch.
 * Per (row, head), every operation rounded to f32 on its own (no fma contraction), with q_i, k_ti, v_ti, a_i the f16 operands widened to f32:
 *   s_t = 0;  for i = 0 .. d-1 in index order:  s_t = s_t + q_i * k_ti;      s_t = s_t * qk_scale          (t = 0 .. Tip-1)
 *   m = max_t s_t;   e_t = expf(s_t - m);   l = e_0 + e_1 + ... in index order;   w_t = e_t / l   (one division per weight)
 *   o_i = 0;  for t = 0 .. Tip-1 in token order:  o_i = o_i + w_t * v_ti
 *   term = ip_scale * o_i;   a_i = f16(a_i + term)   -- one rounding to f16; a term of +-0 leaves the bits of a_i as they are (V_ip = 0 changes nothing).
 * Deterministic: a thread per (row, head), no atomics.  6 B of device memory traffic per element of [B*Tq, H*d]. */
int tcl_attention_ip_add_f16(const void* q, int ldq, long qbs, const void* kv_ip, void* a, int lda, long abs_, int B, int H, int Tq, int Tip, int d,
                             float qk_scale, float ip_scale, int kv_div, hipStream_t st);

/* ---- VidToMe token merging (utils/VidToMe/vidtome/merge.py, patch.py:14-91); int32 maps live on the device ---- */
/* metric / metric.norm(dim=-1) with f16 rounding of the norm and the quotient (merge.py:84, :386). */
int tcl_tome_normalize_f16(const void* x, void* y, long rows, int C, hipStream_t st);
/* bipartite soft matching with align_batch (merge.py:84-117 randframe, :389-421 2s): cosine scores of src rows a_pos[na]
 * vs dst rows b_pos[nb] of metric [Bt,T,C] (normalised), batch entries concatenated along dst, greedy row max; the r src rows with
 * the highest f16 score are merged (ties: highest score, lowest concatenated dst index for the match, lowest src index for the cut).
 * The score matrix is never materialised and nothing is sorted: unmerged src rows keep their index order in the merged sequence (the
 * reference orders them by score, which only permutes the tokens of a permutation-invariant attention).
 * Outputs: mrg[na-r+nb] = input position feeding each merged slot ([unmerged src | dst], mode "replace");
 *          unm[position] = merged slot each input position is restored from (merge.py:135-155).
 * Exactly the entries named above are written: mrg[0 .. na-r+nb) and unm[p] for every p in a_pos or b_pos; unm at a position that neither list names is
 * left as the caller had it.  a_pos and b_pos are read while the maps are written: mrg / unm must not overlap them (nor each other).
 * ws: tcl_tome_match_workspace_bytes(na) bytes, ZEROED ONCE by the caller before the first call and then only passed to this function
 * (one stream; may be re-used for any smaller na): every call leaves it all-zero again except two result words at a fixed offset (layout:
 * 4 KiB control | 256 KiB unused, formerly score-histogram bins | keys).  Per call: the score kernel + two small launches (threshold select, maps). */
size_t tcl_tome_match_workspace_bytes(int na);
/* 1: C = 640 affine matches take the strip-resident kernel too (same maps; faster alone, slower beside the flash kernel: off by default; TCL_TOME640). */
int tcl_tome_strip640(int enable);
int tcl_tome_match_f16(const void* metric, long bstride, int Bt, int C, const int* a_pos, int na, const int* b_pos, int nb, int r,
                       int* mrg, int* unm, void* ws, hipStream_t st);
/* The same with a hint: the positions are affine -- a_pos[i] = i < a_split ? i : i + a_gap and b_pos[j] = b0 + j -- which is what every VidToMe
 * match is (the dst frame of a random-frame merge, the two halves of a two-set merge).  For C = 320 this takes a kernel that keeps a src
 * strip in registers and sweeps the dst tiles with a running maximum (csrc/merge.hip, k_tome_match320); same outputs, bit for bit. */
int tcl_tome_match_affine_f16(const void* metric, long bstride, int Bt, int C, const int* a_pos, int na, const int* b_pos, int nb, int r,
                              int a_split, int a_gap, int b0, int* mrg, int* unm, void* ws, hipStream_t st);
/* out[i] = outer[off + inner[i]] (inner NULL = identity): composition of unmerge maps (func_warper, vidtome/utils.py:42-48). */
int tcl_index_compose(const int* outer, const int* inner, int off, int n, int* out, hipStream_t st);
/* out[b][p] = map[p] >= 0 ? s1[b][map[p]] : s2[b][~map[p]]  (merge in "replace" mode; map NULL = copy). */
int tcl_gather_rows_f16(const void* s1, long bs1, const void* s2, long bs2, const int* map, void* out, long bso, int Bt, int n, int C, hipStream_t st);
/* Two row sets through one map: oa[b][p] = sa[b][map[p]], ob[b][p] = sb[b][map[p]] (map NULL = identity; sb / ob NULL = one set).  The VidToMe chain moves a
 * token block and its cosine-normalised rows (the matching metric, merge.py:86-87) together: the survivors of the local merge go straight into their slot of the
 * global match's [src | dst] block and the new bank (patch.py:76-80) into the block of the chunk that will meet it, so no concatenation copy
 * (patch.py:62-70 `torch.cat`) and no second normalisation exist.  bs* / bo*: elements between batch entries. */
int tcl_gather_rows_pair_f16(const void* sa, long bsa, const void* sb, long bsb, const int* map, void* oa, long boa, void* ob, long bob, int Bt, int n, int C,
                             hipStream_t st);
/* h[b][i] += y[b][map[i]]  (unmerge + residual add, patch.py:178-179). */
int tcl_gather_add_rows_f16(void* h, long bsh, const void* y, long bsy, const int* map, int Bt, int n, int C, hipStream_t st);

/* ---- stage-2 input producer ---- */
/* get_soft_mask_bwds  utils/flow_utils.py:40-54: img [N,3,H,W], fwd/past flows [N,2,H,W] -> mask [N,1,H,W];
 * thr_abs = org_images.max() * diff_threshold. */
int tcl_soft_mask_bwds(const float* img, const float* fwd, const float* past, int N, int H, int W, float alpha, float beta, float thr_abs,
                       float* mask, hipStream_t st);
/* get_flowid  utils/flow_utils.py:56-93: ids int32 [N,H,W]; *last_id (device int) ends as the number of ids;
 * thr_abs = frames.max() * rgb_threshold.  Conflicting writes: the largest source index wins (the reference's CPU order). */
size_t tcl_flowid_workspace_bytes(int H, int W);
int tcl_flowid(const float* frames, const float* fwd_flows, const float* masks, int N, int H, int W, float thr_abs, int* ids, int* last_id,
               void* ws, hipStream_t st);

/* Measurement aid (bench.py roofline leg): bracket every flash-kernel launch (head_dim == dfilter, 0 = all) with HIP events
 * on its own stream; _end returns the summed kernel time, the algorithmic FLOPs 4*B*H*Tq*Tk*d and the launch count (a launch =
 * one attention call: the speculative kernel and the gated exact kernel behind it are timed together). */
int tcl_flash_profile_begin(int dfilter);
int tcl_flash_profile_end(double* total_ms, double* total_flops, long* launches);
int tcl_flash_profile_shape(int* shape4);        /* (B, H, Tq, Tk) of the largest launch profiled since _begin */
/* The same for the other two matrix-pipe consumers of path 1 (bench.py `roofline_gemm`, `roofline_match`): mask bit 0 = every
 * tcl_gemm_f16 / tcl_conv3x3_f16 / tcl_ln_gemm_f16 call (work = 2 M N K FLOP, the conv and Linear layers of SURVEY A9), bit 1 = every
 * tcl_tome_match*_f16 call (work = 2 n_src n_dst C Bt FLOP, the score GEMM of merge.py:84-108 / :389-421; the call's threshold and
 * map kernels are inside the bracket).  _end(cls = bit index) synchronises that class's events and switches it off. */
int tcl_prof_begin(int mask);
int tcl_prof_end(int cls, double* total_ms, double* total_work, long* launches);

/* Split-KV attention for ONE entry, head_dim 128 (round 6: the MemFlowNet memory read, memory_manager_skflow.py:44-69 -- one head, 14 400 queries at 1280x720
 * are 114 blocks for 256 CUs).  The keys are cut into nsplit chunks that run as batch entries of the flash kernel; each writes its normalised partial output and
 * log2 of its softmax denominator, a merge kernel joins them.  q [Tq, ldq], k [Tk, ldk], v [Tk, ldv] (head h at column h*d), o [Tq, ldo]; Tk % (64 nsplit) == 0. */
size_t tcl_attention_splitkv_workspace_bytes(int nsplit, int H, int Tq, int Tk, int d);
int tcl_attention_splitkv_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int H, int Tq, int Tk, int d,
                              float scale, int nsplit, void* ws, hipStream_t st);

/* ---- MemFlowNet correlation lookup (utils/evaluation/memflow/core/Networks/MemFlowNet/corr.py:74-120 CorrBlock,
 * computed on demand like the reference's unused alt_cuda_corr extension -- the all-pairs volume never exists).  f32, NHWC feature maps.
 * tcl_avgpool2_nhwc_f32: F.avg_pool2d(2, 2) (floor on odd sizes) -- builds the fmap2 pyramid level by level.
 * tcl_corr_lookup_f32: fmap1 [B,H,W,D]; fmap2_levels / level_h / level_w: HOST arrays of num_levels (<= 4) device pointers [B,h_l,w_l,D] and
 * their sizes; coords [B,2,H,W] (channel 0 = x, 1 = y, in fmap2 pixels of level 0); out = [B, L*(2r+1)^2, H, W] when out_nchw (the
 * reference's layout) else [B,H,W,L*(2r+1)^2]; channel = level*(2r+1)^2 + a*(2r+1) + b with x offset a-r and y offset b-r (the
 * reference's meshgrid(dy, dx) order), scaled by 1/sqrt(D).  D % 64 == 0, D <= 512, radius <= 5. */
int tcl_avgpool2_nhwc_f32(const float* x, float* y, int B, int H, int W, int D, hipStream_t st);
/* as tcl_corr_lookup_f32, written as f16 rows [B*H*W, ld] (channels [0, L*(2r+1)^2), ld >= that; padding channels are left untouched) */
int tcl_corr_lookup_rows_f16(const float* fmap1, const float* const* fmap2_levels, const int* level_h, const int* level_w, int num_levels,
                             const float* coords, void* out_rows, int ld, int B, int H, int W, int D, int radius, hipStream_t st);
int tcl_corr_lookup_f32(const float* fmap1, const float* const* fmap2_levels, const int* level_h, const int* level_w, int num_levels,
                        const float* coords, float* out, int B, int H, int W, int D, int radius, int out_nchw, hipStream_t st);
/* tcl_corr_lookup_rows_f16 for ONE entry and radius 4 with the neighbour rows shared by 8 x 8 pixel tiles (round 6; the windows of a tile's pixels overlap
 * almost completely under a smooth flow): fmap1_h / fmap2_levels_h = the same maps in f16 (level 0 is the encoder's f16 output itself, the pooled levels are
 * rounded once); a tile whose windows span more than 512 points is computed by the per-pixel f32 kernel from fmap1 / fmap2_levels instead (same call).
 * tile_flags: num_levels * ceil(H/8) * ceil(W/8) ints of scratch, rewritten by every call (1 = that tile took the per-pixel route). */
int tcl_corr_lookup_rows_tiled_f16(const void* fmap1_h, const void* const* fmap2_levels_h, const float* fmap1, const float* const* fmap2_levels,
                                   const int* level_h, const int* level_w, int num_levels, const float* coords, void* out_rows, int ld, int H, int W, int D,
                                   int radius, int* tile_flags, hipStream_t st);

/* ---- BriaRMBG-1.4 matting (briarmbg.py, generate.py:147-167).  f32 NCHW.
 * tcl_conv3x3_direct_f32: Conv2d(k=3, padding=dilation, dilation, stride 1|2) over x = cat([x1, x2], channel) (x2 may be NULL, C2 = 0)
 *   with w_t = weight.reshape(Cout, Cin*9).T contiguous ([Cin*9, Cout], tap index ky*3+kx), then y = conv*scale[oc] + shift[oc]
 *   (eval BatchNorm and the conv bias folded in), optional ReLU, then + resid (REBNCONV briarmbg.py:11-25; RSU tail `hx1d + hxin`).
 * tcl_maxpool2_ceil_f32: MaxPool2d(2, stride=2, ceil_mode=True) over BC planes.
 * tcl_resize_bilinear_f32: F.interpolate(size=(Ho,Wo), mode="bilinear") (align_corners=False), result * mul, optional sigmoid / clamp to [0,1]. */
int tcl_conv3x3_direct_f32(const float* x1, int C1, const float* x2, int C2, const float* w_t, const float* scale, const float* shift,
                           const float* resid, float* y, int B, int H, int W, int Cout, int dilation, int stride, int relu, hipStream_t st);
int tcl_maxpool2_ceil_f32(const float* x, float* y, int BC, int H, int W, hipStream_t st);
int tcl_resize_bilinear_f32(const float* x, float* y, int BC, int H, int W, int Ho, int Wo, float mul, int sigmoid, int clamp01, hipStream_t st);

/* ---- MemFlowNet encoders (core/Networks/MemFlowNet/cnn.py:124-216 BasicEncoder) -- the pieces beside tcl_gemm_f16 / tcl_conv3x3_f16.
 * tcl_conv7x7s2_c3_f16: Conv2d(3, 64, 7, stride 2, padding 3) on x [B,3,H,W] f32 NCHW -> y [B,Ho,Wo,64] f16 NHWC; w_t [147,64] f32 with
 *   row c*49 + ky*7 + kx (an eval BatchNorm may be folded into w_t / bias), optional ReLU.
 * tcl_instnorm_f16: InstanceNorm2d (affine=False, biased variance, eps) over [B,HW,C] f16 NHWC, optional ReLU; deterministic.
 *   C % 8 == 0, C <= 256, C / 8 a divisor of 256.  One pass of f32 sums of x - (the channel's value in the sample's first row): a channel whose mean is
 *   large against its spread keeps its variance, an all-zero channel gives exactly 0.
 * tcl_add_act_f16: y = act(a + b), act 0 none / 3 ReLU / 4 GELU(erf); n elements (n % 8 == 0).
 * tcl_subsample2_nhwc_f16: y[b][i][j] = x[b][2i][2j] (the pixel selection of a stride-2 1x1 convolution). */
int tcl_conv7x7s2_c3_f16(const float* x, const float* w_t, const float* bias, void* y, int B, int H, int W, int relu, hipStream_t st);
size_t tcl_instnorm_workspace_bytes(int B, int C);
int tcl_instnorm_f16(const void* x, void* y, int B, int HW, int C, float eps, int relu, void* ws, hipStream_t st);
int tcl_add_act_f16(const void* a, const void* b, void* y, long n, int act, hipStream_t st);
int tcl_subsample2_nhwc_f16(const void* x, void* y, int B, int H, int W, int C, hipStream_t st);

/* ---- MemFlowNet update block (core/Networks/MemFlowNet/sk2.py, MemFlow.py:172-183) -- glue beside the GEMMs, f16 NHWC rows unless noted.
 * tcl_dwconv_gelu_f16: y = gelu(x + depthwise_kxk(x) + bias) (PCBlock4_Deep_nopool_res, sk2.py:26-27); w [k*k, C] f16 (tap-major), k in {1, 7, 15} (the sizes sk2.py:201-202 uses).
 * tcl_nchw_f32_to_rows_f16 / tcl_rows_f16_to_nchw_f32: move Cs channels between an f32 NCHW tensor [B,Cs,P] and channels [c0, c0+Cs) of f16
 *   rows [B*P, ld] (zero_rest clears the other channels; the reverse computes out = alpha*out + beta*value, alpha 0 = overwrite).
 * tcl_axpy_f16: y = a + s*b.   tcl_upsample_flow_f32: MemFlowNet.upsample_flow -- softmax over the 9 taps of mask_scale*mask (rows
 *   [B*h*w, ldm], channel tap*64 + i*8 + j) applied to the 3x3 neighbourhood of 8*flow [B,2,h,w] -> [B,2,8h,8w]. */
/* tcl_context_split_f16: MemFlowNet.encode_context (MemFlow.py:112-115): c rows [P,256] -> net = tanh(c[:, :128]), inp = relu(c[:, 128:]). */
int tcl_context_split_f16(const void* c, void* net, void* inp, long P, hipStream_t st);
int tcl_dwconv_gelu_f16(const void* x, const void* w, const void* bias, void* y, int B, int H, int W, int C, int k, hipStream_t st);
int tcl_nchw_f32_to_rows_f16(const float* x, void* y, int B, int Cs, int P, int ld, int c0, int zero_rest, hipStream_t st);
int tcl_rows_f16_to_nchw_f32(const void* x, float* y, int B, int Cs, int P, int ld, int c0, float alpha, float beta, hipStream_t st);
int tcl_axpy_f16(const void* a, const void* b, float s, void* y, long n, hipStream_t st);
int tcl_upsample_flow_f32(const float* flow, const void* mask, int ldm, float mask_scale, float* up, int B, int h, int w, hipStream_t st);


/* ---- RAFT (utils/evaluation/core/raft.py:73-131, update.py:33-136, extractor.py:139-172) -- the update block and the fnet stem; csrc/raft.hip.
 * tcl_raft_sepconv_f16: one SepConvGRU convolution group (update.py:37-56: convz/convr/convq 1 and 2, 1x5 pad (0,2) when vertical = 0, 5x1 pad (2,0)
 *   when vertical = 1) as an implicit GEMM over x = [src0 | src1] (f16 rows [B*H*W, 128] each; C1 = 0: src1 absent, else 128), W [N, 5*(128+C1)] f16
 *   with column tap*(128+C1) + source*128 + c.  mode 0: out32 [M,N] f32 = conv + bias (the context term of the GRU input, computed once per pair);
 *   mode 1 (N = 256, [convz | convr]): z [M,128] f32 = sigmoid(conv + pbias[:, :128]), rh [M,128] f16 = sigmoid(conv + pbias[:, 128:]) * h (update.py:45-46);
 *   mode 2 (N = 128, convq over [rh | x]): h <- (1 - z) h + z tanh(conv + pbias) in place, f32 blend, one rounding (update.py:47-48). */
int tcl_raft_sepconv_f16(const void* src0, const void* src1, int C1, const void* w, const float* bias, const float* pbias, float* out32, float* z,
                         void* rh, void* h, int B, int H, int W, int N, int vertical, int mode, hipStream_t st);
/* tcl_raft_convf1_f16: BasicMotionEncoder.convf1 + ReLU (update.py:78,85) on flow = coords1 - coords0 read from coords1 [B,2,H,W] f32 NCHW (coords0 is
 *   the pixel grid, utils.py:83-86) -> f16 rows [B*H*W, ldo], channels 0..127; w_t [98,128] f32, row c*49 + ky*7 + kx. */
int tcl_raft_convf1_f16(const float* coords1, const float* w_t, const float* bias, void* y, int ldo, int B, int H, int W, hipStream_t st);
/* tcl_conv7x7s2_instnorm_f16: the instance-norm encoder's stem (extractor.py:139,164-166: conv1 7x7 stride 2 -> InstanceNorm2d(64) -> ReLU) with the
 *   convolution kept in f32 up to the normalisation (two-pass f32 statistics): x [B,3,H,W] f32 NCHW -> y [B,Ho,Wo,64] f16 NHWC; w_t as
 *   tcl_conv7x7s2_c3_f16.  ws: tcl_stem_instnorm_workspace_bytes(B, H, W) bytes. */
size_t tcl_stem_instnorm_workspace_bytes(int B, int H, int W);
int tcl_conv7x7s2_instnorm_f16(const float* x, const float* w_t, const float* bias, void* y, int B, int H, int W, float eps, void* ws, hipStream_t st);

/* ---- warp-error-ssim (evaluate.py:74-78; utils/evaluation/eval_utils.py:265-350: SaveWarpingImage with RAFT flows, warp_flow = cv2.remap INTER_CUBIC /
 *   BORDER_CONSTANT, compute_fwdbwd_mask's bwd_mask, np.uint8, skimage structural_similarity(channel_axis=2)); csrc/evaluate.hip.
 * tcl_eval_warp_mask_u8: pairs i = i0 .. i0+B-1 of edit [N,H,W,3] u8 with fwd = fut[i], bwd = past[i+1] (fut / past [N,2,H,W] f32 as
 *   estimate_flows_raft returns them): cubic remap on cv2's 1/32-pixel grid, mask = |bwd + remap(fwd, bwd)| < 0.5 (|bwd| + |remap(fwd, bwd)|) + 0.5,
 *   warped [B,H,W,3] u8 = u8(mask ? remap(edit[i], bwd) : 0), target [B,H,W,3] u8 = mask ? edit[i+1] : 0 (u8: truncate toward zero, keep 8 bits).
 * tcl_eval_ssim_u8: out[b] (f64) = SSIM of x[b] vs y[b] (u8 [B,H,W,3], 7x7 uniform window, sample covariance, data range 255, mean over the interior
 *   cropped by 3 pixels and the 3 channels); H, W >= 7; ws: tcl_eval_ssim_workspace_bytes(B, H, W) bytes.  Deterministic (fixed-order sums). */
int tcl_eval_warp_mask_u8(const void* edit, const float* fut, const float* past, void* warped, void* target, int N, int H, int W, int i0, int B,
                          hipStream_t st);
size_t tcl_eval_ssim_workspace_bytes(int B, int H, int W);
int tcl_eval_ssim_u8(const void* x, const void* y, double* out, int B, int H, int W, void* ws, hipStream_t st);

/* ---- light-follow (evaluate.py --light): does the relit light obey its light_path?  This project's own figure (the reference has none); csrc/lightfit.hip.
 * Definition.  E (relit) and S (source) are u8 [N,3,H,W] of one size.  Per frame and pixel (x, y):
 *   Ye = ((0.299 R + 0.587 G) + 0.114 B) / 255 of E and Ys likewise of S, in f32, every product, sum and the IEEE division rounded on its own;
 *   w = 1 when both Ye and Ys lie in [2/255, 253/255] (the f32 constants), else 0 -- clipped pixels are dropped;
 *   r = log((Ye + 1/255) / (Ys + 1/255)),  u = (2x + 1)/W - 1,  v = (2y + 1)/H - 1;
 *   sums[n] = (Sw, Swu, Swv, Swuu, Swuv, Swvv, Swr, Swru, Swrv, Swrr).
 *   The host solves the 3x3 normal equations in f64 for r ~ a + gx u + gy v.  Angle, in light_path's convention (the side the light comes FROM: 0
 *   left, 90 top, 180 right, 270 bottom): atan2(-gy, -gx) in degrees mod 360; contrast: hypot(gx, gy); R^2 from Swrr.  A frame has no estimate when
 *   Sw < 3, the system is singular or the contrast is 0; it then counts with cosine 0.  light-follow = mean over frames of cos(angle - wanted angle),
 *   light-contrast = the mean contrast.
 * tcl_light_fit_u8: the f32 sequence per pixel, without fma contraction: a = Ye + fl(1/255); b = Ys + fl(1/255); r = logf(a / b);
 *   u = fl(float(2x + 1 - W) * fl(1 / float(W))), v likewise with y, H; the terms w, wu, wv, (wu)(wu), (wu)(wv), (wv)(wv), wr, (wr)(wu), (wr)(wv),
 *   (wr)(wr).  Summation order: a frame is cut into spans of 16384 consecutive pixels, one block of 256 threads each; thread t adds the terms of the
 *   16 consecutive pixels from span*16384 + j*4096 + t*16, j = 0..3, to f32 accumulators in pixel order (64 pixels per thread, never more); the
 *   accumulators widen to f64; a wave adds its 64 lanes by a xor butterfly (offsets 32 .. 1); the block adds its four waves in order and stores its
 *   partial to ws; a finish launch adds a frame's partials in span order into sums [N,10] f64.  No atomics: results are bit-identical from run to
 *   run and depend on N, H, W alone (16 B loads when H*W % 16 == 0 and E, S are 16 B aligned, byte loads otherwise: the same values, the same order).
 *   ws: tcl_light_fit_workspace_bytes(N, H, W) bytes, 8 B aligned (0 for a shape that is refused).  N outside 1..65535, H or W <= 0, H*W >= 2^31 or a
 *   null pointer return TCL_EINVAL with nothing launched or written. */
size_t tcl_light_fit_workspace_bytes(int N, int H, int W);
int tcl_light_fit_u8(const void* E, const void* S, int N, int H, int W, double* sums, void* ws, hipStream_t st);

/* ---- clip-frame / clip-text (evaluate.py:39-49,119: clip.load("ViT-B/32"); utils/evaluation/eval_utils.py:129-161 clip_text / clip_frame); csrc/clip.hip.
 *   The model is OpenAI CLIP (clip/model.py: VisionTransformer, Transformer / ResidualAttentionBlock, QuickGELU, CLIP.encode_image / encode_text); its
 *   Linears and LayerNorms run on tcl_gemm_f16 / tcl_layernorm_f16, the entry points below are the rest.
 * tcl_clip_resize_geometry: the sizes of `preprocess` (clip.py _transform(n_px): Resize(n_px, BICUBIC) -> CenterCrop(n_px)) for an H x W frame:
 *   h_geom (HOST, 4 ints) = resized height, resized width (short side `side`, long side int(side * long / short)), crop top, crop left
 *   (int(round((size - side) / 2.0)), round half to even).
 * tcl_clip_preprocess_u8: `preprocess(pil)` of eval_utils.py:137,151 on frames [N,H,W,3] u8: PIL Image.resize(BICUBIC) restated in its integer
 *   arithmetic (a = -0.5, support widened by the down-scale factor, normalised coefficients rounded to 22-bit fixed point, horizontal pass rounded and
 *   clipped to u8 before the vertical pass), centre crop, / 255, (x - mean) / std with CLIP's constants.  Only the cropped window is computed.
 *   crop [N,side,side,3] u8 (may be NULL): the resized and cropped image, bit-identical to PIL.  patches [N, (side/patch)^2, 3*patch*patch] f16 (may
 *   be NULL): the normalised pixels as patch rows in the column order of visual.conv1.weight.reshape(width, -1) (channel, row, column), so that
 *   VisionTransformer.conv1 is one tcl_gemm_f16.  Down-scale factors up to about 17. */
int tcl_clip_resize_geometry(int H, int W, int side, int* h_geom);
int tcl_clip_preprocess_u8(const void* frames, void* crop, void* patches, int N, int H, int W, int side, int patch, hipStream_t st);
/* The same two in the convention of transformers' CLIP image processor, which feeds PickScore (evaluate.py:120-121 AutoProcessor of
 *   laion/CLIP-ViT-H-14-laion2B-s32B-b79K; eval_utils.py:163-176 pick_score_func): the same PIL bicubic resize, but `center_crop` starts at
 *   (size - side) / 2 rounded DOWN.  rule: 0 = the rounded crop above, 1 = floor; they differ by one row or column when size - side = 2 (mod 4),
 *   e.g. a 227 x 224 frame.  tcl_clip_preprocess_ld_u8 also takes the stride ldp of a patch row in halves, ldp >= 3*patch*patch and ldp % 64 == 0
 *   (or ldp == 3*patch*patch): columns 3*patch*patch .. ldp-1 of every row are written as zeros, so a patch size whose 3*patch*patch is not a
 *   multiple of tcl_gemm_f16's K step (ViT-H/14: 588 -> ldp 640) still embeds with one GEMM against a conv1 weight zero-padded the same way.  With
 *   rule 0 and ldp = 3*patch*patch it is tcl_clip_preprocess_u8 byte for byte (one kernel serves both).  The u8 crop is bit-identical to PIL. */
int tcl_clip_resize_geometry_rule(int H, int W, int side, int rule, int* h_geom);
int tcl_clip_preprocess_ld_u8(const void* frames, void* crop, void* patches, int N, int H, int W, int side, int patch, int ldp, int rule, hipStream_t st);
/* tcl_clip_attention_f16: nn.MultiheadAttention of ResidualAttentionBlock.attention (self-attention, need_weights=False) after its in_proj: qkv
 *   [B*T, 3*H*d] f16 = [q | k | v], head hh at columns hh*d of each third, read in place; out [B*T, H*d] f16 = softmax(scale q k^T (+ causal mask)) v,
 *   heads concatenated (the operand of out_proj).  causal: key j > query i is masked (CLIP.build_attention_mask, the text tower).  One workgroup per
 *   (sample, head) with the head's K and V in LDS, exact softmax.  d % 16 == 0, d <= 128, T <= 288 and K, V within 160 KB of LDS (d = 64: T <= 288;
 *   d = 80: T <= 288); anything else returns TCL_EINVAL. */
int tcl_clip_attention_f16(const void* qkv, void* out, int B, int T, int H, int d, float scale, int causal, hipStream_t st);
/* tcl_clip_embed_f16: the rows that enter a tower, out [B*T, W] f16.  ids == NULL (VisionTransformer.forward): row 0 of every sample = cls [W], rows
 *   1 .. T-1 = patch [B, T-1, W] (the conv1 GEMM's output), + pos [T, W], then LayerNorm(gamma, beta, eps) = ln_pre.  ids != NULL (CLIP.encode_text):
 *   table[ids[b, t]] + pos[t] (ids int32 [B,T], table [vocab, W]).  gamma / beta NULL: no LayerNorm.  f32 up to the one rounding; W <= 2048. */
int tcl_clip_embed_f16(const void* patch, const void* cls, const int* ids, const void* table, const void* pos, const void* gamma, const void* beta,
                       void* out, int B, int T, int W, int vocab, float eps, hipStream_t st);
/* tcl_clip_quick_gelu_f16: QuickGELU (clip/model.py: x * sigmoid(1.702 * x)), n f16 elements, n % 8 == 0; y may be x. */
int tcl_clip_quick_gelu_f16(const void* x, void* y, long n, hipStream_t st);
/* tcl_clip_scores: feats [N,D] f32, text [D] f32 (may be NULL) -> out2 (device, 2 doubles): out2[0] = clip_frame (eval_utils.py:156-159: the sum of the
 *   off-diagonal entries of the cosine matrix / (N (N - 1))), out2[1] = clip_text (eval_utils.py:140-142: the mean cosine of the rows to `text`; 0 when
 *   text is NULL).  f64 sums in a fixed order, no atomics: the same input gives the same bits.  ws: tcl_clip_scores_workspace_bytes(N) bytes. */
size_t tcl_clip_scores_workspace_bytes(int N);
int tcl_clip_scores(const float* feats, const float* text, int N, int D, double* out2, void* ws, hipStream_t st);
/* tcl_pick_scores: pick-score (evaluate.py:52-56; eval_utils.py:163-176 pick_score_func: logit_scale.exp() * text_embs @ image_embs.T of the
 *   normalised embeddings, averaged over the frames).  feats [N,D] f32, text [D] f32, logit_scale = the log as the checkpoint stores it -> out
 *   (device, N + 1 doubles): out[0] = the mean, out[1 + i] = exp(logit_scale) cos(text, feats[i]).  f64 sums in a fixed order, no atomics: the same
 *   input gives the same bits. */
int tcl_pick_scores(const float* feats, const float* text, int N, int D, float logit_scale, double* out, hipStream_t st);

/* ---- frame-lpips (utils/evaluation/eval_utils.py:368-386 FrameLPIPS: lpips.LPIPS(net='vgg') between each relit frame and its source frame, both in
 *   0..255); csrc/lpips.hip.  The model is LPIPS v0.1 (lpips/lpips.py LPIPS.forward, ScalingLayer, NetLinLayer, normalize_tensor, spatial_average;
 *   lpips/pretrained_networks.py vgg16 = torchvision VGG-16 `features` tapped at relu1_2 .. relu5_3).  features.2 .. features.28 run on
 *   tcl_conv3x3_f16 (act 3); the entry points below are the rest.  Everything here returns TCL_EINVAL, and launches nothing, for a shape it cannot serve.
 * tcl_lpips_stem_f16: ScalingLayer (lpips.py:148-156) + features.0 + ReLU.  img [B,H,W,3] u8 -> y [B,H,W,64] f16 NHWC,
 *   y = relu(bias[o] + sum over the 3x3 taps and 3 channels of w[o][(ky*3+kx)*3 + c] * v), v = img - shift_c inside the frame and 0 outside: the zero
 *   padding is Conv2d's, of the SCALED image.  w [64,27] f32 is the conv weight times (input scale / scale_c), bias [64] f32; f32 sums, one rounding.
 * tcl_maxpool2_f16: MaxPool2d(kernel_size=2, stride=2) of VGG-16 (floor mode: an odd last row / column is dropped).  x [B,H,W,C] -> y [B,H/2,W/2,C]
 *   f16 NHWC, C % 64 == 0, H, W >= 2.  Of equal values the first in window order wins, NaN wins over all: bit-equal to torch's max_pool2d.
 * tcl_lpips_head: one tap of lpips.py:112-123.  f [2B,P,C] f16 (image 0 of pair b at row b, image 1 at row B + b), w [C] f32 (lin{k}.model.1.weight):
 *   per pixel sum_c w_c (f0_c / (|f0| + eps) - f1_c / (|f1| + eps))^2 in f32, summed over blocks of 64 pixels into the workspace, with each block's
 *   count of non-finite features.  h_P (HOST, ntaps ints, ntaps <= 8): the pixel counts of all the taps of this evaluation, tap: which of them f is;
 *   C % 64 == 0.  ws: tap k's section follows those of the taps before it and is B * ceil(h_P[k] / 64) * 8 bytes.
 * tcl_lpips_finish: spatial_average and the sum over the taps (lpips.py:119-128): out [B] f32 = sum_k (partials of tap k, added in index order in
 *   f64) / h_P[k], the taps in order; nonfinite [ntaps] int32 (device) = the non-finite features seen per tap.  No atomics anywhere: the same
 *   input gives the same bits.
 * tcl_lpips_workspace_bytes: the workspace of the five VGG taps of an H x W frame (H x W, then halved with floor four times) for B pairs; 0 when a
 *   pooled size would be 0 (H or W < 16) or B is outside 1..65535. */
int tcl_lpips_stem_f16(const void* img, const float* w, const float* bias, float shift_r, float shift_g, float shift_b, void* y, int B, int H, int W,
                       hipStream_t st);
int tcl_maxpool2_f16(const void* x, void* y, int B, int H, int W, int C, hipStream_t st);
size_t tcl_lpips_workspace_bytes(int B, int H, int W);
int tcl_lpips_head(const void* f, const float* w, int B, const int* h_P, int ntaps, int tap, int C, float eps, void* ws, hipStream_t st);
int tcl_lpips_finish(const void* ws, int B, const int* h_P, int ntaps, float* out, int* nonfinite, hipStream_t st);

/* ===================================================================== spatio-temporal Unique Video Tensor (sceneflow scenes); csrc/voxel.hip */
/* SceneFlowDataParser.rgbd2pcd  utils/dataparsers/sceneflow_dataparsers.py:257-274.  depth [N,H,W], c2w [N,4,4] row-major -> p_world [N,3,H,W]
 *   (planar, so process_frames applies directly).  Per pixel, without fma contraction: x = (px - cx) * d / fx (product, then quotient), y likewise,
 *   p_world[j] = ((x * c2w[j][0] + (-y) * c2w[j][1]) + (-d) * c2w[j][2]) + c2w[j][3].  N in 1..65535, H, W > 0, H * W < 2^31, else TCL_EINVAL. */
int tcl_unproject_sceneflow(const float* depth, const float* c2w, int N, int H, int W, float fx, float fy, float cx, float cy, float* p_world,
                            hipStream_t st);
/* torch_scatter.scatter(values, ids, dim=0, reduce='mean')  utils/general_utils.py:237,239.  values [N,C,H,W] (C <= 3), ids [N,H,W] in [0, K)
 *   (entries outside are skipped) -> mean [K,C], cnt [K] (f32 counts).  PRECONDITION: the ids of every frame are pairwise distinct
 *   (tcl_track_ids_unique == 1).  f32 sums one frame after the other, no atomics, then ONE division by max(cnt, 1): exactly a sequential scatter in
 *   row order, bit for bit. */
int tcl_track_mean_f32(const float* values, const int* ids, int N, int C, int H, int W, size_t K, float* mean, float* cnt, hipStream_t st);
/* The quantisation of utils/general_utils.py:238,243-250: keys [K,6] int32 = (floor_div(xyz - xyz_min, voxel_size) | floor_div(rgb, rgb_vox_size)) in
 *   the order (x, y, z, r, g, b) of torch.cat([coord, rgb]).  mean_rgb, mean_xyz [K,3]; xyz_min: 3 floats (device).  floor_div restates
 *   c10::div_floor_floating (torch div(rounding_mode='floor')) without fma contraction; the float result is converted saturating, NaN -> 0. */
int tcl_voxel_keys(const float* mean_rgb, const float* mean_xyz, const float* xyz_min, float voxel_size, float rgb_vox_size, size_t K, int* keys,
                   hipStream_t st);
/* torch.unique(keys, dim=0, return_inverse=True)  utils/general_utils.py:230,251.  keys [n,C] int32, 1 <= C <= 6 -> inv [n] int32, *count (device
 *   int) = number of distinct rows.  Ids are numbered in order of FIRST APPEARANCE in row order (the reference: lexicographic rank; the same
 *   partition, a permutation of the numbering) and are bit-identical from run to run.  ws: tcl_unique_rows_workspace_bytes(n) bytes; the call
 *   clears what it needs itself, so a workspace may be reused across calls without the caller clearing it.  n > 2^30 or C outside 1..6 returns
 *   TCL_EINVAL (the workspace size is then 0). */
size_t tcl_unique_rows_workspace_bytes(size_t n);
int tcl_unique_rows_i32(const int* keys, size_t n, int C, int* inv, int* count, void* ws, hipStream_t st);

/* ===================================================================== detail transfer (generation.detail_transfer); csrc/detail.hip */
/* tcl_detail_transfer_f32 (replaces the "detail transfer" node of IC-Light workflows -- two Gaussian blurs and a handful of element-wise image
 *   operations): src S, relit R [N,3,H,W] f32 in [0,1], mask m [N,1,H,W] f32 in [0,1] or NULL (= 1 everywhere) -> out O [N,3,H,W] f32; all frames in
 *   one call, every frame on its own.  h_taps is a HOST array of n_taps = 2*radius + 1 floats in [0, 1] (detail.gaussian_taps: exp(-k^2 / 2 sigma^2)
 *   normalised in f64, rounded once to f32), copied into the kernel arguments.  G below is the separable blur with those taps, rows first, then
 *   columns, borders reflected without repeating the edge sample (index -i -> i, L-1+i -> L-1-i).  Each 1-D pass is  a = 0; for k = 0 .. 2r:
 *   a = fmaf(w_k, v_k, a)  in ascending index order; the intermediate between the passes is f32 (the workspace).  Everything else in f32 with no fma
 *   contraction, IEEE division; Y(x) = fmaf(0.114f, x_B, fmaf(0.587f, x_G, 0.299f * x_R));  bm = blend * m (blend when mask is NULL):
 *     TCL_DETAIL_ADD    D = S - R;  P = D - G(D) per channel (luma: P = Y(D) - G(Y(D)), the same for the three channels);
 *                       O = min(max(R + bm * P, 0), 1).  S == R gives D = +0, G(D) = +0, P = 0 and O = R bit for bit for R in [0,1].
 *     TCL_DETAIL_RATIO  q = (G(R) + e) / (G(S) + e) per channel, e = 1.f/255.f (luma: of G(Y(R)) and G(Y(S)), one q for the three channels);
 *                       T = S * q;  O = min(max(R + bm * (T - R), 0), 1).
 *   ws: tcl_detail_transfer_workspace_bytes(N, H, W, mode, luma) bytes = N * planes * H * W * 4 with planes 3 | 1 (add rgb | luma) and 6 | 2 (ratio);
 *   the size is 0 for arguments the call would refuse.  out and ws may alias neither each other nor an input.
 *   Two launches: rows (one block per TCL_DETAIL_ROW_SEG pixels of a row) and columns fused with the combine (one block per TCL_DETAIL_TILE_W x
 *   TCL_DETAIL_TILE_H tile).  TCL_EINVAL, with nothing launched or written: null pointers (mask excepted), N, H, W <= 0, radius outside
 *   1 .. TCL_DETAIL_MAX_RADIUS, n_taps != 2*radius + 1, radius >= min(H, W), an unknown mode, luma other than 0 / 1, blend outside [0,1] or NaN, a tap
 *   outside [0,1], a workspace that is too small, aliasing as above, N > 21845 or H > 65535. */
#define TCL_DETAIL_ROW_SEG 256
#define TCL_DETAIL_TILE_W 64
#define TCL_DETAIL_TILE_H 32
#define TCL_DETAIL_MAX_RADIUS 48
enum { TCL_DETAIL_ADD = 0, TCL_DETAIL_RATIO = 1 };
size_t tcl_detail_transfer_workspace_bytes(int N, int H, int W, int mode, int luma);
int tcl_detail_transfer_f32(const float* src, const float* relit, const float* mask, float* out, int N, int H, int W, const float* h_taps, int n_taps,
                            int radius, int mode, int luma, float blend, void* ws, long ws_bytes, hipStream_t st);

/* ===================================================================== full-resolution output (generation.fullres); csrc/guided.hip */
/* The fast guided filter (He & Sun 2015): fit  R ~ a G + b  in every window of the working size, average a and b once more, upsample them and apply
 * them to the source's native pixels.  Every frame on its own, all frames in one call.
 *
 * tcl_guided_fit_f32: src S, relit R [N,3,h,w] f32 in [0,1] -> abar, bbar [N,3,h,w] f32.  Guide G: luma 0: G_c = S_c (every channel guided by itself);
 *   luma 1: G = Y(S) = fmaf(0.114f, S_B, fmaf(0.587f, S_G, 0.299f * S_R)) for the three channels (detail transfer's Y).  The window of pixel (x, y) is
 *   x-r .. x+r by y-r .. y+r CLIPPED to the image, cnt its true pixel count (exact in f32).  The moments are centred at 0.5 -- one pass, no second
 *   pass over the data.  All in f32, no fma contraction, IEEE division, every sum  s = 0; s = s + t_k  in ascending index order, rows (x) first, the
 *   row sums stored as f32 (the workspace), then columns (y):
 *     g = G - 0.5f;  q = R_c - 0.5f;   T_g, T_q, T_gg, T_gq = the sums of g, q, g * g, g * q over the window;
 *     m_g = T_g / cnt ... m_gq = T_gq / cnt;   var = max(m_gg - m_g * m_g, 0);   cov = m_gq - m_g * m_q;
 *     a = cov / (var + eps);   b = ((m_q - a * m_g) + 0.5f) - 0.5f * a;
 *     abar = (sum of a over the window) / cnt;   bbar = (sum of b over the window) / cnt      -- the same two passes, the row sums again f32.
 *   No atomics: equal inputs give equal bits.  ws: tcl_guided_workspace_bytes(N, h, w) = N * TCL_GUIDED_WS_PLANES * h * w * 4 bytes (12 planes of
 *   moment row sums, reused for the 6 of a and b, + 6 planes a, b); 0 for sizes the call would refuse.  Four launches: moment rows (one block per
 *   TCL_GUIDED_ROW_SEG pixels of a row), columns fused with the solve (TCL_GUIDED_TILE_W x TCL_GUIDED_TILE_H tiles), rows and columns of a, b.
 *   TCL_EINVAL, with nothing launched or written: a null pointer, N outside 1 .. 65535, h or w < 1, h > 65535, N * 18 * h * w > 2^31 - 1, radius
 *   outside 1 .. TCL_GUIDED_MAX_RADIUS, eps outside [1e-4f, 1] or NaN, luma other than 0 / 1, a workspace that is too small or misaligned, abar / bbar /
 *   ws aliasing each other or an input.
 *
 * tcl_guided_apply_u8: abar, bbar [N,3,h,w] f32, src [N,Hc,Wc,3] uint8 (interleaved) -> out [N,Hc,Wc,3] uint8.  For output pixel (X, Y), in f32 with no
 *   fma contraction, sx = (float)w / (float)Wc, sy likewise:
 *     u = ((float)X + 0.5f) * sx - 0.5f;  u = min(max(u, 0), w - 1);  x0 = (int)u;  x1 = min(x0 + 1, w - 1);  fx = u - x0;      v, y0, y1, fy likewise
 *     F(f) = t + fy * (l - t)  with  t = f[y0][x0] + fx * (f[y0][x1] - f[y0][x0]),  l = f[y1][x0] + fx * (f[y1][x1] - f[y1][x0])
 *     out_c = min(max(rint(F(abar_c) * (float)src_c + 255.f * F(bbar_c)), 0), 255)        rint: to nearest, ties to even
 *   The arithmetic is in 0 .. 255 units: abar = 1, bbar = 0 gives the source back byte for byte.  A lane owns four neighbouring pixels of a row and
 *   stores their 12 bytes as three dwords where Wc % 4 == 0 and both images are 4-byte aligned, as bytes otherwise.  TCL_EINVAL, with nothing launched
 *   or written: a null pointer, N outside 1 .. 65535, a size < 1, Hc > 65535, N * 3 * h * w or N * 3 * Hc * Wc > 2^31 - 1, out aliasing an input. */
#define TCL_GUIDED_ROW_SEG 256
#define TCL_GUIDED_TILE_W 64
#define TCL_GUIDED_TILE_H 32
#define TCL_GUIDED_MAX_RADIUS 64
#define TCL_GUIDED_WS_PLANES 18
size_t tcl_guided_workspace_bytes(int N, int h, int w);
int tcl_guided_fit_f32(const float* src, const float* relit, float* abar, float* bbar, int N, int h, int w, int radius, float eps, int luma, void* ws,
                       long ws_bytes, hipStream_t st);
int tcl_guided_apply_u8(const float* abar, const float* bbar, const unsigned char* src, unsigned char* out, int N, int h, int w, int Hc, int Wc,
                        hipStream_t st);

/* ===================================================================== keyframe relighting (generation.keyframes); csrc/keyframe.hip */
/* Only every K-th frame (the keys) is denoised; the gain field relit / source of the two neighbouring keys is carried to the frames in between along
 *   the chained flows.  All tensors f32 NCHW, contiguous.  Pixel centres sit at integer coordinates, p = (x, y).  fut [N,2,H,W]: fut[i] maps frame i to
 *   i+1 (fut[N-1] = 0); past [N,2,H,W]: past[i] maps i to i-1 (past[0] = 0); channel 0 is dx, channel 1 dy.  Everything in f32 with no fma contraction,
 *   IEEE division and square root, in the order written.
 *     inb(q)     0 <= qx <= W-1 && 0 <= qy <= H-1                                                                    (false for a NaN)
 *     bil(T, q)  qx' = min(max(qx, 0), W-1), qy' likewise (a q that is inb is unchanged; the clamp keeps every address inside the frame);
 *                x0 = floor(qx'), x1 = min(x0 + 1, W-1), fx = qx' - x0, the same in y;  top = T[y0,x0] + fx * (T[y0,x1] - T[y0,x0]);
 *                bot = T[y1,x0] + fx * (T[y1,x1] - T[y1,x0]);  bil = top + fy * (bot - top)
 *   h_keys: HOST int32 [M], the frame numbers of the keys, strictly increasing from 0 to N-1, no gap (difference of neighbours) above
 *   TCL_KEYFRAME_MAX_GAP.  Gap g lies between keys g and g+1.  One call works on the gaps g0 <= g < g1 (a batch): the frames f0 = h_keys[g0] ..
 *   f1 = h_keys[g1], at most TCL_KEYFRAME_BATCH_FRAMES of them, so the workspace stays bounded whatever N is.
 *   ws: [f1 - f0 + 1 slots][2 directions][3][H][W] f32, slot = frame - f0, direction 0 = CL (towards the left key), 1 = CR (right key), planes
 *   (dx, dy, valid); the slots of key frames are not touched.  tcl_keyframe_workspace_bytes(N, H, W, K) = min(N, TCL_KEYFRAME_BATCH_FRAMES) * 24 * H * W
 *   is enough for every batch of a clip whose gaps are at most K; 0 for arguments the calls would refuse (K outside 1 .. TCL_KEYFRAME_MAX_GAP).
 *
 * tcl_flow_chain_f32: for every non-key frame j of the batch, with its keys a < j < b, CL[j] = the flow from j to a and CR[j] = the flow from j to b.
 *   Left direction, d = j - a (the right direction is the mirror image: fut and past exchanged, j+1 for j-1, CR for CL, d = b - j):
 *     A = past[j](p);  q = p + A;  g = bil(fut[j-1], q) per component;
 *     e = A + g;  fb = e.x*e.x + e.y*e.y < t*t  with  t = alpha * (sqrt(A.x*A.x + A.y*A.y) + sqrt(g.x*g.x + g.y*g.y)) + alpha;
 *     d = 1:  C = A;                          valid = inb(q) && fb
 *     d > 1:  C = A + bil(CL[j-1].xy, q);     valid = inb(q) && fb && the four taps (y0|y1, x0|x1) of CL[j-1].valid at q are all 1
 *     CL[j](p) = valid ? (C.x, C.y, 1) : (0, 0, 0): the workspace never holds a value computed from outside the frame.
 *   One launch per distance d = 1 .. (longest gap of the batch) - 1 covers both directions of all gaps of the batch (one block per TCL_KEYFRAME_TILE_W
 *   x TCL_KEYFRAME_TILE_H pixels of one frame and direction): at most TCL_KEYFRAME_MAX_GAP - 1 launches, each reading what the one before wrote.
 *
 * tcl_keyframe_propagate_f32: source S [N,3,H,W], relit_keys R [M,3,H,W] (R_k: the relit frame h_keys[k]) -> out [N,3,H,W], holes [N] u32, both
 *   written for the frames f0 .. f1 of the batch only.  HOST tables over all N frames, copied into the kernel arguments: h_left / h_right int32 [N],
 *   the index into h_keys of the last key at or before / the first key at or after frame i (a key frame: its own index twice), and h_tw f32 [2,N]:
 *   ta = (b - i) / (b - a) in [0][i], tb = 1 - ta in [1][i], a and b the FRAME numbers of the two keys, each computed in f64 and rounded once
 *   (a key frame: 1, 0).  A key frame is copied from relit_keys bit for bit, holes 0.  A non-key frame i, per pixel p and key k in {a, b} with
 *   C_k = CL[i] | CR[i] of the workspace tcl_flow_chain_f32 filled for the same batch:
 *     q = p + C_k.xy;  s_c = bil(S_k,c, q);  r_c = bil(R_k,c, q);  m = max(max(|s_0 - S_i,0(p)|, |s_1 - S_i,1(p)|), |s_2 - S_i,2(p)|);
 *     w_k = t_k * C_k.valid * (m < diff_threshold ? 1 : 0);  G_k,c = (r_c + eps) / (s_c + eps)
 *     w = w_a + w_b;  w > 0:   G_c = (w_a * G_a,c + w_b * G_b,c) / w
 *                     else:    a hole, visible in neither key: G_c = ta * G'_a,c + tb * G'_b,c with G'_k,c = (R_k,c(p) + eps) / (S_k,c(p) + eps),
 *                              the gains unwarped at p itself; holes[i] is incremented (an integer atomic: the count is exact in any order)
 *     out_c = (S_i,c(p) + eps) * G_c - eps.                            No clamping: the frames stay unclamped until they are saved.
 *   One launch (and one clear of holes[f0 .. f1]) per call.
 *
 * TCL_EINVAL from both, with nothing launched or written: a null pointer, N, H, W, M <= 0, H * W > 2^30, H > 65535 * TCL_KEYFRAME_TILE_H, alpha or
 *   diff_threshold not a finite number > 0, eps outside (0, 0.25], h_keys not as above, g0 / g1 outside 0 <= g0 <= g1 <= M-1 or a batch of more than
 *   TCL_KEYFRAME_BATCH_FRAMES frames, a workspace below (f1 - f0 + 1) * 24 * H * W bytes, h_left / h_right that do not agree with h_keys, a weight
 *   outside [0, 1]. */
#define TCL_KEYFRAME_TILE_W 64
#define TCL_KEYFRAME_TILE_H 4
#define TCL_KEYFRAME_MAX_GAP 16
#define TCL_KEYFRAME_BATCH_FRAMES 33
size_t tcl_keyframe_workspace_bytes(int N, int H, int W, int K);
int tcl_flow_chain_f32(const float* fut, const float* past, const int* h_keys, int M, int g0, int g1, int N, int H, int W, float alpha, void* ws,
                       long ws_bytes, hipStream_t st);
int tcl_keyframe_propagate_f32(const float* source, const float* relit_keys, float* out, unsigned* holes, const int* h_keys, int M, int g0, int g1,
                               const int* h_left, const int* h_right, const float* h_tw, int N, int H, int W, float diff_threshold, float eps,
                               const void* ws, long ws_bytes, hipStream_t st);

/* ===================================================================== flow-warped noise (generation.noise_mode warp); csrc/noisewarp.hip */
/* The noise of a clip as a field F_t [4,H,W] f32 at PIXEL resolution (H, W multiples of TCL_NOISE_WARP_CELL = 8), carried from frame to frame along the
 *   backward flow so that it stays white and unit-variance in every frame.  past_flows [N,2,H,W] f32 (channel 0 dx, 1 dy; frame t to t-1), mask_bwds
 *   [N,1,H,W] f32, G (the fresh field of frame t) and F_prev / F [4,H,W] f32, all contiguous.  Everything in f32 unless said, no fma contraction, IEEE
 *   division and square root, in the order written.  Per pixel p = (x, y) of frame t >= 1, with (u, v) = past_flows[t, :, y, x]:
 *     qx = rintf((float)x + u), qy = rintf((float)y + v)                       (round to nearest, ties to even: torch.round)
 *     valid(p) = qx >= 0 && qx <= W-1 && qy >= 0 && qy <= H-1 && mask_bwds[t, 0, y, x] > 0.5     (false for a NaN anywhere, an inf flow)
 *     k(q) = the number of valid p with source q;  S_c(q) = the sum over them of llrintf(G[c, p] * 16777216.f) in int64 (two's complement)
 *     invalid p:          F[c, p] = G[c, p]
 *     valid p, k(q) == 1: F[c, p] = F_prev[c, q]                                 (the bits)
 *     valid p, k(q) > 1:  mean = (float)((double)S_c(q) / (16777216.0 * (double)k));  a = F_prev[c, q] / sqrtf((float)k);  b = G[c, p] - mean;
 *                         F[c, p] = a + b
 *   Frame 0: F = G.  The latent noise of the frame, z[t] [4,h,w] with h = H/8, w = W/8:
 *     row_i = ((((((F[c,8y+i,8x] + F[c,8y+i,8x+1]) + F[c,8y+i,8x+2]) + ...) + F[c,8y+i,8x+7]     (the 8 pixels of a row, left to right)
 *     z[t, c, y, x] = (((row_0 + row_1) + row_2) + ... + row_7) * 0.125f                          (the 8 rows, top to bottom)
 *   ws: int64 S [4,H,W] first, then int32 k [H,W]; tcl_noise_warp_workspace_bytes(H, W) = 36 * H * W, 0 for a size the calls would refuse.  8 B aligned.
 *
 * tcl_noise_warp_count: frame t >= 1.  Clears the workspace (one memset), then one launch: k and S of every source, by integer atomics -- the result
 *   is the same bits whatever order the adds arrive in.
 * tcl_noise_warp_apply_f32: frame t.  One launch: recomputes q, writes F and, fused, z[t] into the caller's z [N,4,h,w].  t == 0: F = G and the
 *   reduction; past_flows, mask_bwds, F_prev and ws are not read and may be null.  F_prev, G and F must be three different buffers.
 *   A pixel with k == 1 reads k and F_prev[q] only; S is read where k > 1.  Safe for any flow: an invalid pixel reads nothing outside its own address.
 *
 * TCL_EINVAL from both, with nothing launched or written: a null pointer among those read, H or W not a positive multiple of 8, H * W > 2^30,
 *   H > 4 * 65535, N <= 0, t outside [1, N) (count) / [0, N) (apply), a workspace below 36 * H * W bytes or not 8 B aligned, F_prev, G, F not distinct. */
#define TCL_NOISE_WARP_TILE_W 64
#define TCL_NOISE_WARP_CELL 8
size_t tcl_noise_warp_workspace_bytes(int H, int W);
int tcl_noise_warp_count(const float* past_flows, const float* mask_bwds, const float* G, int t, int N, int H, int W, void* ws, long ws_bytes,
                         hipStream_t st);
int tcl_noise_warp_apply_f32(const float* past_flows, const float* mask_bwds, const float* G, const float* F_prev, float* F, float* z, int t, int N,
                             int H, int W, const void* ws, long ws_bytes, hipStream_t st);

#ifdef __cplusplus
}
#endif
#endif
