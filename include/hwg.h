/*
 * hwg.h — C-ABI of libhwg_hip.so, the MI355X (gfx950) kernel library behind the
 * GAN training hot path of herobd/handwriting_line_generation.
 *
 * The reference has no FFI layer: every op below replaces an ATen
 * call made by the reference's Python modules; the reference call site each entry
 * point stands in for is cited next to it (paths relative to the reference root).
 *
 * Conventions
 *  - all tensors are device pointers to contiguous fp32, activations are NHWC
 *    ([N,H,W,C], C fastest) unless stated otherwise; integer tensors are int32/int64
 *    as stated;
 *  - the caller owns every buffer (including workspaces); the library never
 *    allocates device memory and never synchronises, all work is enqueued on
 *    `stream` (a hipStream_t passed as void*);
 *  - every function returns HWG_OK (0) or a negative hwg_status; the message is
 *    available from hwg_last_error() (thread local). Nothing throws across the ABI.
 */
#ifndef HWG_H_
#define HWG_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum hwg_status {
  HWG_OK = 0,
  HWG_ERR_ARG = -1,      /* unsupported / inconsistent arguments */
  HWG_ERR_LAUNCH = -2,   /* hipLaunch / runtime failure */
  HWG_ERR_WORKSPACE = -3 /* workspace too small */
} hwg_status;

const char* hwg_last_error(void);
/* library/ABI version, bumped when a signature changes */
int hwg_abi_version(void);
/* 1 when a HIP device is present and usable */
int hwg_device_ok(void);
/* Schedules (tile, split factor, kernel variant) are planned once per geometry and cached per thread; the tuning knobs of the
 * environment (HWG_WINO, HWG_WINO_FORCE, HWG_CONV_FORCE, HWG_WGRAD_FORCE, HWG_WINO_WGRAD, HWG_WGRAD_NARROW, ...) are read at plan time.
 * A process that changes them afterwards calls hwg_tuning_reload() (drops every cached plan). hwg_last_plan() reports what the process's
 * last convolution-family launch ran (any thread: backward passes launch from the autograd engine's thread): out[0] engine (the hwg_prof_stop kind codes), out[1] schedule id, out[2] split factor -
 * how the parity tests assert that a forced schedule was the one launched. */
int hwg_tuning_reload(void);
int hwg_last_plan(int* engine_cfg_nsplit);
/* Stream dependencies for kernels launched off the caller's main stream (weight gradients on a side stream: nothing in a backward pass
 * waits for them, only the optimizer does). fork: `side_stream` waits for everything enqueued on `main_stream` so far; join: `main_stream`
 * waits for everything enqueued on `side_stream` so far. Host cost: one event record + one stream wait on a reused event. */
int hwg_stream_fork(void* main_stream, void* side_stream);
int hwg_stream_join(void* side_stream, void* main_stream);

/* Launch profiler for the matrix-core kernels (bench.py's roofline measurement): between hwg_prof_start() and hwg_prof_stop() every
 * MFMA convolution / weight-gradient launch (and their reduce passes) is bracketed by a HIP event pair on its stream. hwg_prof_tag()
 * labels the launches of the calling thread's next calls. hwg_prof_stop() waits for the recorded events and returns, per launch,
 * kind (0 conv MFMA, 1 wgrad MFMA, 2 conv split reduce, 3 wgrad reduce, 4 direct conv, 5 direct wgrad incl. its reduce, 6 Winograd conv, 7 Winograd wgrad), tag, algorithmic work (flops; bytes for the reduce passes) and ms.
 * Returns the number of records written. */
int hwg_prof_start(int max_records);
int hwg_prof_enable(int on);   /* pause / resume recording inside an open profile (sampled profiling: the event pairs cost ~7 % of a step) */
int hwg_prof_tag(int tag);
int hwg_prof_stop(int* kinds, int* tags, double* work, float* ms, int capacity);

/* activation codes used by fused epilogues */
enum { HWG_ACT_NONE = 0, HWG_ACT_RELU = 1, HWG_ACT_LRELU = 2, HWG_ACT_TANH = 3 };

/* ------------------------------------------------------------------------------------------
 * Convolution engine (implicit GEMM on fp32 MFMA, direct kernels for 1-channel ends).
 * Replaces nn.Conv2d / nn.Conv1d / nn.ConvTranspose2d / F.conv_transpose2d / nn.Linear at
 * model/pure_gen.py:161-197,268-278,286; model/discriminator_ap.py:77-131;
 * model/cnn_only_hwr.py:31-32,78-92; model/char_style.py:65-71,90-93,162-168;
 * model/count_cnn.py:12-23; model/autoencoder.py:307-330,346-395,601-617.
 * ------------------------------------------------------------------------------------------ */
typedef struct hwg_conv_desc {
  int N, H, W, C;             /* gathered tensor  [N,H,W,C]            */
  int K, R, S;                /* K channels on the anchor grid, RxS taps */
  int stride_h, stride_w;
  int pad_h, pad_w;
  int dil_h, dil_w;
  int P, Q;                   /* anchor grid     [N,P,Q,K]             */
  int transposed;             /* 0: anchor(p,q) <-> gathered(p*stride-pad+r*dil)   (convolution)
                                 1: fractionally strided gather (conv-transpose with stride>1), dil must be 1:
                                    out(p,q) += x(ih,iw) * w(r,s)  where  ih*stride-pad+r == p            */
} hwg_conv_desc;

/* Re-layout a weight tensor into the engine's [R*S][A][Bpad] form (b fastest, zero padded to Bpad).
 * src element (a,b,r,s) lives at src[a*sa + b*sb + r*sr + s*ss]; flip!=0 mirrors the taps. */
int hwg_conv_pack_weight(const float* src, float* dst, int A, int B, int Bpad, int R, int S,
                         long long sa, long long sb, long long sr, long long ss, int flip, void* stream);

/* The same re-layout for many weights in one launch (after an optimizer step). table: device array of n_entries records
 * { const float* src; float* dst; int A, B, Bpad, R, S, flip; long long sa, sb, sr, ss, total, first_block; int mode, Apad; }
 * (96 bytes) where total = R*S*A*Bpad and first_block = running sum of ceil(total/1024); total_blocks = that sum over all entries.
 * mode 1 = the Winograd filter transform of hwg_wino_pack_weight (then Apad = ceil16(A), Bpad = ceil16(B), total = Apad*Bpad);
 * mode 2 = hwg_wino_s2_pack_weight (A = Kc, B = Cc, sa = sk, sb = sc, flip = dgrad; Apad / Bpad = the image's padded extents, total = Apad*Bpad). */
int hwg_conv_pack_weight_multi(const void* table, int n_entries, long long total_blocks, void* stream);
/* ... and for weights that are a device-side scalar multiple of a stored tensor: the spectral-norm layers' W_bar / sigma
 * (model/discriminator_ap.py:31-32, recomputed on every forward pass). Records of 112 bytes: the 96-byte record above followed by
 * { long long dst_off; int scale_idx; int pad; }: the image goes to dst_base + dst_off floats (the record's own dst is ignored), every source
 * element is multiplied (rounded product) by scale_base[scale_idx] - all images a pass through the network needs, one launch per forward. */
int hwg_conv_pack_weight_multi_scaled(const void* table, int n_entries, long long total_blocks, float* dst_base, const float* scale_base, void* stream);

/* y[N,P,Q,K] = gather-conv(x[N,H,W,C], w[R*S][K][C]) (+ bias[K] if bias != NULL).
 * transposed==0: standard convolution. transposed==1: conv-transpose with stride>1.
 * accumulate!=0 adds into y instead of overwriting it.
 * Layers with few output pixels but a long contraction (taps x channels) are scheduled split-K: partial outputs go to the
 * caller's workspace (hwg_conv_fwd_workspace() bytes, 0 when the schedule does not split) and are summed in a fixed order. */
size_t hwg_conv_fwd_workspace(const hwg_conv_desc* d);
int hwg_conv_fwd(const hwg_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                 int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* Data gradient of a convolution whose input has ONE channel (first layers; stride 1), second half: the caller first forms the
 * per-pixel tap matrix t[N,P,Q,R*S] = dy[N,P,Q,K] x W[K][R*S] with hwg_conv_fwd (1x1, on the matrix cores), then
 * dx[n,ih,iw] = sum_{r,s} t[n, ih+pad_h-r*dil_h, iw+pad_w-s*dil_w, r*S+s]. */
int hwg_col2im_taps(const float* t, float* dx, int N, int H, int W, int P, int Q, int R, int S, int pad_h, int pad_w, int dil_h, int dil_w,
                    void* stream);

/* weight gradient: dw(k,c,r,s) = sum_{n,p,q} u[n,p,q,k] * v[n, p*stride-pad+r*dil, q*stride-pad+s*dil, c]
 * written to dw[k*sa + c*sb + r*sr + s*ss] (so it lands directly in the PyTorch parameter layout).
 * u is the tensor living on the anchor grid [N,P,Q,K], v the gathered one [N,H,W,C]; d->transposed is ignored.
 * accumulate!=0 adds into dw. dbias (may be NULL) additionally receives the column sums of u, dbias[k] = sum_{n,p,q} u[n,p,q,k]
 * (the bias gradient when u is the output gradient), taken from the u tiles the kernel stages anyway; bias_accumulate!=0 adds.
 * Not available on the direct path (K <= 2 or C <= 2 without the taps-as-N kernel): use hwg_colsum there. */
size_t hwg_conv_wgrad_workspace(const hwg_conv_desc* d);
int hwg_conv_wgrad(const hwg_conv_desc* d, const float* u, const float* v, float* dw,
                   long long sa, long long sb, long long sr, long long ss, int accumulate,
                   float* dbias, int bias_accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* Gradient sets: `sets` weight gradients of one layer whose anchors differ (u / dy = the sets' [N,P,Q,K] tensors back to back) and whose
 * gathered tensor (v / x, [N,H,W,C]) is shared - the two or three upstream gradients a balanced lesson sends through the generator
 * (reference trainer/hw_with_style_trainer.py:300-338 runs one backward() per loss group on the same activations). One launch; set s is
 * summed into the buffers dw_ptrs[s] / dbias_ptrs[s] (host arrays of device addresses). d describes ONE set; workspace =
 * hwg_*_wgrad_sets_workspace(d, sets) bytes (the pixel ranges are planned for the whole launch and shared out over the sets). set_on_v != 0 (hwg_conv_wgrad_sets only): the sets differ in the GATHERED tensor v instead and share the anchor u
 * (transposed layers, whose anchor is the layer input); no fused bias gradient then. hwg_conv_wgrad_sets_supported: the layer runs on the MFMA path (not the K <= 2 / C <= 2 direct kernels). */
int hwg_conv_wgrad_sets_supported(const hwg_conv_desc* d);
size_t hwg_conv_wgrad_sets_workspace(const hwg_conv_desc* d, int sets);
size_t hwg_wino_wgrad_sets_workspace(const hwg_conv_desc* d, int sets);
int hwg_conv_wgrad_sets(const hwg_conv_desc* d, const float* u, const float* v, int sets, int set_on_v, const long long* dw_ptrs,
                        long long sa, long long sb, long long sr, long long ss, int accumulate,
                        const long long* dbias_ptrs, int bias_accumulate, void* workspace, size_t workspace_bytes, void* stream);
int hwg_wino_wgrad_sets(const hwg_conv_desc* d, const float* dy, const float* x, int sets, const long long* dw_ptrs, long long sa,
                        long long sb, long long sr, long long ss, int accumulate, const long long* dbias_ptrs, int bias_accumulate,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Deferred sum of the weight-gradient partial images (reference: the per-parameter gradient accumulation autograd does after every backward
 * node, trainer/hw_with_style_trainer.py:300-338 reads the results only after the pass). hwg_conv_wgrad / hwg_wino_wgrad write one partial
 * image per pixel range into the workspace and sum them into dw (+dbias) with a launch of their own - 65 such launches per training step, most
 * too small to stream at memory rate. hwg_wgrad_defer_next() marks the calling thread's NEXT weight-gradient call: its sum is queued instead of
 * launched, and the caller must keep that call's workspace alive and untouched (its own arena, not a shared scratch buffer) until
 * hwg_wgrad_defer_flush(stream, &launches) has been enqueued, which sums everything queued so far (any thread) with one table-driven launch
 * per 32 gradients: every gradient runs the schedule it would have run alone (bit-identical results), several gradients of the same tensor
 * are summed in queue order by consecutive launches. dw / dbias are undefined between the call and the flush. The mark is consumed by the next
 * hwg_conv_wgrad / hwg_wino_wgrad call whatever path it takes (paths without partial images simply ignore it). */
int hwg_wgrad_defer_next(void);
long long hwg_wgrad_defer_pending(void);
int hwg_wgrad_defer_flush(void* stream, int* launches);

/* Winograd F(2x2,3x3) path for 3x3 / stride 1 / dilation 1 convolutions with C % 16 == 0 and K >= 16 (same call sites as
 * hwg_conv_fwd: the 3x3 layers of model/discriminator_ap.py:84-131, model/cnn_only_hwr.py:31-32, model/pure_gen.py:161-197,
 * model/char_style.py:65-71, model/autoencoder.py:346-395 and their data gradients). Input, filter and output transforms are
 * fused into the kernel; the 16 transform-domain GEMMs run on v_mfma_f32_16x16x4_f32 (2.25x fewer MACs than the direct form).
 * hwg_wino_pack_weight turns a weight (element (a,b,r,s) at src[a*sa+b*sb+r*sr+s*ss], a = output channel of THIS product,
 * b = contracted channel, flip mirrors the taps) into U = G g G^T laid out [ceil16(B)/16][16][ceil16(A)][16]
 * (hwg_wino_weight_floats(A, B) floats). d describes the product as for hwg_conv_fwd (transposed must be 0). */
int hwg_wino_supported(const hwg_conv_desc* d);
/* 1 when the library's cost models put the Winograd schedule ahead of the direct one for this product (callers pick the weight image accordingly) */
int hwg_wino_preferred(const hwg_conv_desc* d);
size_t hwg_wino_weight_floats(int A, int B);
int hwg_wino_pack_weight(const float* src, float* dst, int A, int B, long long sa, long long sb, long long sr, long long ss,
                         int flip, void* stream);
size_t hwg_wino_conv_workspace(const hwg_conv_desc* d);
int hwg_wino_conv_fwd(const hwg_conv_desc* d, const float* x, const float* u, const float* bias, float* y,
                      int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* 4x4 stride-2 pad-0 dilation-1 convolutions (d->transposed = 0; reference: the style extractor's down-sampling convolutions,
 * model/char_style.py:154 Conv2dBlock(dim, 2*dim, 4, 2, 1): a pad layer followed by nn.Conv2d(.., 4, 2), :69-71) and their data gradients (d->transposed = 1, described like the
 * fractionally strided product of hwg_conv_fwd: input = dy [N,H,W,C], output = dx [N,P,Q,K] with P = 2H + 2, Q = 2W + 2) as stride-1 two-tap
 * convolutions on the space-to-depth image in the Winograd domain F(3x3, 2x2) (conv_wino.hip). The filter image (hwg_wino_s2_weight_floats
 * floats) is packed from the CONVOLUTION's weight: element (output channel kc, input channel cc, r, s) at src[kc*sk + cc*sc + r*4 + s];
 * dgrad = 1 packs the image of the data-gradient product. hwg_wino_s2_preferred: 1 when the cost models put it ahead of the direct kernels. */
int hwg_wino_s2_supported(const hwg_conv_desc* d);
int hwg_wino_s2_preferred(const hwg_conv_desc* d);
size_t hwg_wino_s2_weight_floats(int Kc, int Cc, int dgrad);
int hwg_wino_s2_pack_weight(const float* src, float* dst, int Kc, int Cc, long long sk, long long sc, int dgrad, void* stream);
size_t hwg_wino_s2_workspace(const hwg_conv_desc* d);
int hwg_wino_s2_conv(const hwg_conv_desc* d, const float* x, const float* u, const float* bias, float* y,
                     int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* (Their weight gradient goes through hwg_wino_wgrad* below, which accept these descriptors as well.) */

/* Diagnostic, like hwg_last_plan: the schedule hwg_wino_conv_fwd (3x3 stride 1) / hwg_wino_s2_conv (4x4 stride 2 pad 0, either direction) would
 * run for this product, without launching anything. out[8] = {tile config, uniform channel split, balanced tail workgroups (0 = uniform
 * schedule), whole-tile lead workgroups, most pieces a cut tile is written in (= workspace images), workgroup tiles, channel chunks, most tiles
 * one tail workgroup touches}; all -1 when the product is not supported. */
int hwg_wino_conv_describe(const hwg_conv_desc* d, int* out);

/* Weight gradient of a 3x3 stride-1 dilation-1 convolution in the Winograd domain F(3x3, 2x2) - or of a 4x4 stride-2 pad-0 one as the two-tap
 * problem on the space-to-depth image, F(2x2 taps, 3x3 gradient tiles) - (conv_wino_wgrad.hip): same operands and weight
 * strides as hwg_conv_wgrad (dy = anchor [N,P,Q,K], x = gathered [N,H,W,C]; reference: the weight gradients autograd produces for
 * model/pure_gen.py, model/discriminator_ap.py and model/cnn_only_hwr.py's 3x3 layers). dbias (or null): the bias gradient, column sums of dy,
 * taken from the dy tiles on their way through the kernel. */
int hwg_wino_wgrad_supported(const hwg_conv_desc* d);
int hwg_wino_wgrad_preferred(const hwg_conv_desc* d);
size_t hwg_wino_wgrad_workspace(const hwg_conv_desc* d);
int hwg_wino_wgrad(const hwg_conv_desc* d, const float* dy, const float* x, float* dw, long long sa, long long sb, long long sr, long long ss,
                   int accumulate, float* dbias, int bias_accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* out[C] (+)= sum over rows of x[rows][C]  (bias gradients, channel sums) */
size_t hwg_colsum_workspace(long long rows, int C);
int hwg_colsum(const float* x, long long rows, int C, float* out, int accumulate,
               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Normalisation + activation epilogues (NHWC, x is [N][HW][C]).
 * mode: 0 InstanceNorm, 1 GroupNorm(groups), 2 BatchNorm in training mode (batch statistics,
 * running stats updated with `momentum` when running_mean != NULL).
 * y = act(mask[n,c] * (gamma * xhat + beta)); gamma/beta are [C] or, with affine_per_sample, [N][C] (dgamma / dbeta likewise; InstanceNorm
 * and GroupNorm only: BatchNorm with affine_per_sample is refused).
 * Replaces nn.GroupNorm (+Dropout2d +ReLU/LeakyReLU) at model/discriminator_ap.py:78-79,103-104,
 * model/autoencoder.py:346-395,307-330, model/char_style.py:41,91,100,166, model/count_cnn.py:13-21;
 * nn.BatchNorm2d/1d at model/cnn_only_hwr.py:36,80-89; nn.InstanceNorm2d at model/pure_gen.py:56.
 * mean/rstd are [N][C] outputs kept for the backward pass.
 * hwg_norm_bwd takes the forward call's gamma / beta: with relu / leaky relu fused it recomputes the activation gate (the sign of the
 * pre-activation, bit-identical to the forward pass) from x instead of reading y - `y` may be NULL then; tanh needs y.
 * CONSTRAINT: gamma / beta must still hold the forward call's values (no optimizer step or in-place write between forward and backward);
 * ops._Norm stamps the parameters' version / optimizer epoch at forward time and refuses a backward pass after a change.
 * ------------------------------------------------------------------------------------------ */
size_t hwg_norm_workspace(int N, int HW, int C);
int hwg_norm_fwd(const float* x, float* y, int N, int HW, int C, int mode, int groups, float eps,
                 const float* gamma, const float* beta, int affine_per_sample, const float* chan_mask,
                 int act, float slope, float* mean, float* rstd, float* running_mean, float* running_var,
                 float momentum, void* ws, size_t ws_bytes, void* stream);
int hwg_norm_bwd(const float* dy, const float* x, const float* y, float* dx, int N, int HW, int C, int mode, int groups,
                 const float* gamma, const float* beta, int affine_per_sample, const float* chan_mask, int act, float slope,
                 const float* mean, const float* rstd, float* dgamma, float* dbeta, int accumulate,
                 void* ws, size_t ws_bytes, void* stream);

/* BatchNorm in eval mode (running statistics); mean/rstd are [N][C] scratch outputs */
int hwg_norm_frozen_fwd(const float* x, float* y, int N, int HW, int C, const float* running_mean, const float* running_var, float eps,
                        const float* gamma, const float* beta, int act, float slope, float* mean, float* rstd, void* stream);

/* Generator epilogue, model/pure_gen.py:205-214 (NoiseInjection -> LeakyReLU -> AdaptiveInstanceNorm):
 *   u = lrelu(x + noise_w[c]*noise_scale*noise, slope);  y = gamma[n,c] * IN(u) + beta[n,c]
 * backward also returns the conv-bias gradient (sum of d/dx) and the raw noise-weight gradient. */
int hwg_adain_fwd(const float* x, const float* noise, const float* noise_w, float noise_scale, float slope,
                  const float* gamma, const float* beta, float eps, float* u, float* y, float* mean, float* rstd,
                  int N, int HW, int C, void* ws, size_t ws_bytes, void* stream);
/* the same with the noise drawn in the kernel (forward-only calls): element i of the [N][HW][C] tensor takes the value hwg_randn(seed, offset)
 * writes to element i of a tensor of that size; no noise tensor exists. u may alias x. */
int hwg_adain_fwd_rng(const float* x, unsigned long long seed, unsigned long long offset, const float* noise_w, float noise_scale, float slope,
                      const float* gamma, const float* beta, float eps, float* u, float* y, float* mean, float* rstd, int N, int HW, int C,
                      void* ws, size_t ws_bytes, void* stream);
int hwg_adain_bwd(const float* dy, const float* u, const float* noise, float noise_scale, float slope,
                  const float* gamma, const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta,
                  float* dnoise_w, float* dbias, int accumulate_params, int N, int HW, int C,
                  void* ws, size_t ws_bytes, void* stream);

/* y = act(mask[row/HW][c] * (x + bias[c])) on x[rows][C]; backward takes y (nn.ReLU / nn.LeakyReLU / nn.Dropout2d sites) */
int hwg_bias_act_fwd(const float* x, const float* bias, const float* chan_mask, float* y, long long rows, int HW, int C,
                     int act, float slope, void* stream);
int hwg_bias_act_bwd(const float* dy, const float* y, const float* chan_mask, float* dx, long long rows, int HW, int C,
                     int act, float slope, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pooling / resampling / padding / concatenation (NHWC).
 * nn.AvgPool2d (discriminator_ap.py:88-127, autoencoder.py:350-389), nn.MaxPool2d/1d (cnn_only_hwr.py:45-55,
 * char_style.py:164), nn.Upsample nearest (pure_gen.py:176-178), Blur (pure_gen.py:80-137),
 * F.pad / ReplicationPad2d (char_style.py:19-21,198-202; trainer :590-595,727-737,771-795), torch.cat.
 * ------------------------------------------------------------------------------------------ */
int hwg_avgpool_fwd(const float* x, float* y, int N, int H, int W, int C, int kh, int kw, void* stream);
int hwg_avgpool_bwd(const float* dy, float* dx, int N, int H, int W, int C, int kh, int kw, void* stream);
/* y = avgpool(act(chan_mask[n][c] * x)) in one pass, and its backward (gate recomputed from x): model/discriminator_ap.py:84-131, the
 * SN conv -> Dropout2d -> LeakyReLU -> AvgPool2d runs of the discriminator; bit-identical to hwg_bias_act_fwd + hwg_avgpool_fwd (resp. their
 * backward kernels) without the full-resolution activation / gradient round trips. act: none / relu / leaky relu; chan_mask may be NULL */
int hwg_act_avgpool_fwd(const float* x, const float* chan_mask, float* y, int N, int H, int W, int C, int kh, int kw, int act, float slope,
                        void* stream);
int hwg_act_avgpool_bwd(const float* dy, const float* x, const float* chan_mask, float* dx, int N, int H, int W, int C, int kh, int kw,
                        int act, float slope, void* stream);
int hwg_maxpool_fwd(const float* x, float* y, int* idx, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                    int P, int Q, void* stream);
int hwg_maxpool_bwd(const float* dy, const int* idx, float* dx, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph,
                    int pw, int P, int Q, void* stream);
/* max-pool with the ReLU that precedes it in the reference riding along (model/cnn_only_hwr.py:31-43: conv -> ReLU -> MaxPool2d):
 * y = relu(maxpool(x)) == maxpool(relu(x)) exactly; backward: dx = scatter(dy * [y > 0]) - same bits as the separate ReLU passes */
int hwg_maxpool_relu_fwd(const float* x, float* y, int* idx, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                         int P, int Q, void* stream);
int hwg_maxpool_relu_bwd(const float* dy, const float* y, const int* idx, float* dx, int N, int H, int W, int C, int kh, int kw, int sh, int sw,
                         int ph, int pw, int P, int Q, void* stream);
int hwg_upsample_nearest_fwd(const float* x, float* y, int N, int H, int W, int C, int fh, int fw, void* stream);
int hwg_upsample_nearest_bwd(const float* dy, float* dx, int N, int H, int W, int C, int fh, int fw, void* stream);
int hwg_blur3(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* mode 0 constant(value) (negative pads crop), 1 replicate */
int hwg_pad2d_fwd(const float* x, float* y, int N, int H, int W, int C, int pt, int pb, int pl, int pr, int mode, float value, void* stream);
int hwg_pad2d_bwd(const float* dy, float* dx, int N, int H, int W, int C, int pt, int pb, int pl, int pr, int mode, void* stream);
/* dst[row][doff+c] (+)= src[bcast ? row/HW : row][soff+c], c < Cn */
int hwg_copy_channels(const float* src, int Cs, int soff, float* dst, int Cd, int doff, int Cn, long long rows, int HW, int bcast,
                      int accumulate, void* stream);
/* dst[row][c] = c < C ? src[row][c] : 0 for c < Cpad (Cpad % 4 == 0): the zero-padded channel copy the MFMA paths take when a contraction
 * side is not a multiple of their channel step (model/cnn_only_hwr.py:92: the RIMES recogniser's 78 classes) - copy and fill in ONE launch
 * (it was a torch-side zero fill plus hwg_copy_channels; the fill was invisible to a recorded call list) */
int hwg_pad_channels(const float* src, int C, float* dst, int Cpad, long long rows, void* stream);
/* out[n][c] (+)= sum_hw src[n*HW+hw][soff+c] */
int hwg_reduce_rows(const float* src, int Cs, int soff, float* out, int Cn, int N, int HW, int accumulate, void* stream);
/* label [L][B] int32 -> out[b][l][doff + cls] one-hot rows of width ncls inside rows of width Cd (HWWithStyle.onehot, hw_with_style.py:333-337) */
int hwg_onehot(const int* label, float* out, int L, int B, int ncls, int Cd, int doff, void* stream);
/* the same one-hot in both layouts at once: out_blc [B][L][ncls] (NHWC rows, what the networks read) and out_lbc [L][B][ncls] (the reference's
 * time-major tensor, hw_with_style.py:333-337) - one launch instead of a one-hot and two permutes */
int hwg_onehot_both(const int* label, float* out_blc, float* out_lbc, int L, int B, int ncls, void* stream);
/* FusedUpsample weight transform, model/pure_gen.py:268-276: [A][B][3][3] -> [A][B][4][4] (AB = A*B) and its adjoint */
int hwg_fused_upsample_weight_fwd(const float* w3, float* w4, long long AB, float mult, void* stream);
int hwg_fused_upsample_weight_bwd(const float* dw4, float* dw3, long long AB, float mult, void* stream);
/* the adjoint ADDED into dw3 (the parameter's gradient buffer): saves the add launch behind it */
int hwg_fused_upsample_weight_bwd_acc(const float* dw4, float* dw3, long long AB, float mult, void* stream);
int hwg_permute4(const float* in, float* out, int d0, int d1, int d2, int d3, long long s0, long long s1, long long s2, long long s3, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sequence ops: LogSoftmax (cnn_only_hwr.py:92, autoencoder.py:617), F.ctc_loss (model/loss.py:28-30),
 * DTW alignment correct_pred (model/hw_with_style.py:18-74), gt-count scan (trainer :670-697).
 * ------------------------------------------------------------------------------------------ */
/* rows of x are (b,t) ordered; with transpose_bt the output rows are (t,b) ordered ([T][B][C], what F.ctc_loss takes) */
int hwg_log_softmax_fwd(const float* x, float* y, long long rows, int C, int B, int T, int transpose_bt, void* stream);
int hwg_log_softmax_bwd(const float* dy, const float* y, float* dx, long long rows, int C, int B, int T, int transpose_bt, void* stream);
/* log_probs [T][B][C]; targets [B][Lmax] int32 (blank = 0); reduction 'mean'; an infinite mean is reported as 0.
 * hwg_ctc_bwd must be called with the same workspace contents hwg_ctc_fwd left behind. */
size_t hwg_ctc_workspace(int T, int B, int Lmax);
int hwg_ctc_fwd(const float* log_probs, const int* targets, const int* input_lengths, const int* target_lengths, int T, int B, int C,
                int Lmax, float* loss, void* ws, size_t ws_bytes, void* stream);
int hwg_ctc_bwd(const float* log_probs, const int* targets, const int* input_lengths, const int* target_lengths, int T, int B, int C,
                int Lmax, const float* grad_out, float* grad, void* ws, size_t ws_bytes, void* stream);
/* the same pair with the beta recursion moved into the forward launch (it needs log_probs only; blocks B..2B-1 run it beside alpha):
 * hwg_ctc_bwd_grad starts at the gradient kernel and must follow hwg_ctc_fwd_beta on the same workspace. Same bits as the pair above. */
int hwg_ctc_fwd_beta(const float* log_probs, const int* targets, const int* input_lengths, const int* target_lengths, int T, int B, int C,
                     int Lmax, float* loss, void* ws, size_t ws_bytes, void* stream);
int hwg_ctc_bwd_grad(const float* log_probs, const int* targets, const int* input_lengths, const int* target_lengths, int T, int B, int C,
                     int Lmax, const float* grad_out, float* grad, void* ws, size_t ws_bytes, void* stream);
/* pred [T][B][C] log-probs, label [L][B] int32 -> out int64 [T+2L+1][B] zero padded, lens[B] path lengths (bit exact) */
size_t hwg_dtw_workspace(int T, int B, int L);
int hwg_dtw_align(const float* pred, const int* label, int T, int B, int C, int L, long long* out, int* lens, void* ws, size_t ws_bytes,
                  void* stream);
/* index_spaced int64 [Tp][B], label int32 [L][B] -> gt [L][B][2] (caller zero-fills), minpos (caller sets to INT_MAX), mismatch counter */
int hwg_gt_counts(const long long* index_spaced, const int* label, int Tp, int B, int L, float* gt, int* minpos, int* mismatch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Spectral norm (model/discriminator_ap.py:11-65), losses (model/loss.py:16-27, trainer :797-821),
 * PixelNorm (pure_gen.py:306-311) and small vector helpers.
 * ------------------------------------------------------------------------------------------ */
size_t hwg_spectral_workspace(int R, int K);
int hwg_spectral_update(const float* W, float* u, float* v, int R, int K, float eps, float* sigma, float* inv_sigma, void* ws,
                        size_t ws_bytes, void* stream);
/* the same iteration (u, v updated in place) that also writes the new vectors to u_copy / v_copy (either may be null): the snapshot a forward
 * pass keeps for its backward pass, without a separate copy (discriminator_ap.py:31-45 clones them) */
int hwg_spectral_update_to(const float* W, float* u, float* v, float* u_copy, float* v_copy, int R, int K, float eps, float* sigma,
                           float* inv_sigma, void* workspace, size_t workspace_bytes, void* stream);
/* the same iteration for n layers at once (four launches in total): `table` = n device records {const float* W; float* u; float* v;
 * long long copy_off; long long ws_off; int R; int K;} (48 bytes); layer i writes its snapshot to copies + copy_off (u [R], then v [K]), uses
 * ws + ws_off (K + R floats) as scratch and leaves (sigma, 1/sigma) in sig[2i], sig[2i+1] */
int hwg_spectral_update_multi(const void* table, int n, int max_R, int max_K, float eps, float* workspace, float* copies, float* sig, void* stream);
int hwg_scale_by_ptr(const float* x, const float* scale, float* out, long long n, void* stream);
int hwg_spectral_bwd(const float* dWsn, const float* Wbar, const float* u, const float* v, const float* sigma, float* dWbar, int R, int K,
                     int accumulate, void* ws, size_t ws_bytes, void* stream);
/* the same for up to 16 layers in two launches (block -> layer, each layer on its own partial schedule: bit-identical to n single calls).
 * table: n host records of 64 bytes {dWsn, Wbar, u, v, sigma, dWbar: 8-byte addresses; R, K, accumulate, pad: 4-byte ints}
 * (reference: the ten SpectralNorm layers of DiscriminatorAP walk backward one by one, model/discriminator_ap.py:11-65) */
size_t hwg_spectral_bwd_multi_workspace(int n);
int hwg_spectral_bwd_multi(const void* table, int n, void* ws, size_t ws_bytes, void* stream);
size_t hwg_loss_workspace(void);
/* out (+)= scale * mean(term); mode 0 |a-b|, 1 (a-b)^2, 2 a, 3 relu(1-a), 4 relu(1+a) */
int hwg_loss_fwd(const float* a, const float* b, long long n, int mode, float scale, float* out, int accumulate, void* ws, size_t ws_bytes,
                 void* stream);
int hwg_loss_bwd(const float* a, const float* b, long long n, int mode, float scale, const float* grad_out, float* da, float* db,
                 int accumulate, void* stream);
/* Foreground-masked L1 of the GAN trainer's `no_bg_loss` (trainer/hw_with_style_trainer.py:596-601: L1Loss(recon * fg_mask, image * fg_mask)).
 * recon, image: [rows][W] fp32 (rows = B * H); mask: [rows][Wm] fp32 with 1 <= Wm <= W, columns >= Wm count as 0 (the reference's
 * F.pad(fg_mask, (0, toPad), value=0), not copied). rows * W < 2^31.
 * _fwd: *out = mean over all rows * W elements of |fl(r m) - fl(x m)| (both products rounded to fp32, no fused multiply-add), summed in the
 *   partial layout and order of hwg_loss_fwd mode 0 (same workspace): a mask of ones gives that call's bits. Two launches.
 * _bwd: d_recon = sign(fl(r m) - fl(x m)) * m * *grad_out / (rows * W), 0 at ties; every element is written. One launch. Image and mask
 *   are data: no gradient. */
int hwg_masked_l1_fwd(const float* recon, const float* image, const float* mask, long long rows, int W, int Wm, float* out, void* ws,
                      size_t ws_bytes, void* stream);
int hwg_masked_l1_bwd(const float* recon, const float* image, const float* mask, long long rows, int W, int Wm, const float* grad_out,
                      float* d_recon, void* stream);
int hwg_pixelnorm_fwd(const float* x, float* y, int rows, int C, float eps, void* stream);
int hwg_pixelnorm_bwd(const float* dy, const float* x, float* dx, int rows, int C, float eps, void* stream);
/* scaled[i] = weights[i] * *x_i and *sum = their left-to-right sum (x_ptrs: HOST array of n <= 16 device addresses of scalars, weights: HOST
 * array; both read during the call) - the trainer's weighted loss accumulation (trainer/hw_with_style_trainer.py:280-298) as one launch,
 * rounded like the chain of hwg_axpby launches it replaces; _bwd: grads[i] = weights[i] * *grad_out */
int hwg_weighted_sum(const void* x_ptrs, const float* weights, int n, float* scaled, float* sum, void* stream);
int hwg_weighted_sum_bwd(const float* grad_out, const float* weights, int n, float* grads, void* stream);
/* out[b] = bank[ij[b]] * w[b] + bank[ij[B + b]] * w[B + b] over rows of D floats (bank [K][D], ij int32 [2][B], w [2][B], all on the device): the
 * interpolation of two stored styles per generated line (trainer/hw_with_style_trainer.py:974-988), products and sum rounded to fp32 */
int hwg_style_mix(const float* bank, const int* ij, const float* w, float* out, int K, int B, int D, void* stream);
int hwg_axpby(const float* x, float a, const float* y, float b, float* out, long long n, void* stream);
/* y = x*scale[c] + shift[c] on x[rows][C] (CountCNN output scaling, count_cnn.py:44); out = a*b elementwise */
int hwg_channel_affine(const float* x, const float* scale, const float* shift, float* y, long long rows, int C, void* stream);
int hwg_mul(const float* a, const float* b, float* out, long long n, void* stream);
int hwg_tanh_fwd(const float* x, float* y, long long n, void* stream);
int hwg_tanh_bwd(const float* dy, const float* y, float* dx, long long n, void* stream);
int hwg_argmax_rows(const float* x, int* out, long long rows, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Character-specific style extraction helpers (model/char_style.py:204-235,286).
 * ------------------------------------------------------------------------------------------ */
/* patches[k][j][c] = x[idx_b[k]][idx_pos[k] - window + j][c], j < 2 window + 1; a position outside [0, Wx) reads as 0, and a window whose
 * CENTRE (idx_b[k], idx_pos[k]) lies outside [0, B) x [0, Wx) is all zeros (also where it reaches back inside): no index is a precondition. */
int hwg_gather_windows(const float* x, int B, int Wx, int C, const int* idx_b, const int* idx_pos, int n, int window, float* patches, void* stream);
/* gradient of hwg_gather_windows: dx[b][pos][c] = sum of the window entries that cover (b, pos), gathered in a fixed order (no atomics).
 * At most one window may be centred on a given (sample, column) - true for the arg-max map the windows come from. A window whose centre lies
 * outside [0, B) x [0, Wx) contributes nothing. win_of: B*Wx ints of scratch, written by the call (no more than that, no contents expected). */
int hwg_scatter_windows(const float* dpatches, int B, int Wx, int C, const int* idx_b, const int* idx_pos, int n, int window, int* win_of,
                        float* dx, void* stream);
/* out[b][c] = sum_{k: seg[k] == b} wgt[k] v[k][c] / wsum[b] (the plain sum where wsum[b] == 0), wsum[b] = sum of those wgt[k]; a member whose
 * seg[k] lies outside [0, B) belongs to no line. The backward, dv[k][c] = wgt[k] / wsum[seg[k]] * dout[seg[k]][c], has no B to check against:
 * PRECONDITION seg[k] in [0, B) for every k, B the line count of the forward call that wrote wsum (it reads wsum[seg[k]] and dout[seg[k]]). */
int hwg_segment_weighted_mean(const float* v, const float* wgt, const int* seg, int n, int C, int B, float* out, float* wsum, void* stream);
int hwg_segment_weighted_mean_bwd(const float* dout, const float* wgt, const int* seg, const float* wsum, int n, int C, float* dv, void* stream);
/* out[k] = exp(x[idx_b[k]][idx_pos[k]][idx_cls[k]]), x [B][Wx][C]; an index outside [0, B) x [0, Wx) x [0, C) gives out[k] = 0 */
int hwg_gather_scores(const float* x, int B, int Wx, int C, const int* idx_b, const int* idx_pos, const int* idx_cls, int n, float* out, void* stream);

/* Bank of L linear layers that share one input (the generator's ten AdaIN style -> (gamma, beta) affines, pure_gen.py:52-69, in one
 * launch instead of ten): y_l = x W_l^T + b_l, x [B][I] (forward: any B, 16 rows per block; backward: B <= 16), W_l [O_l][I] and b_l [O_l] through device pointer tables.
 * Layer l's outputs are written as `halves` contiguous [B][O_l/halves] blocks starting at y + off[l]; first_wave[L+1] is the
 * running sum of O_l (neuron -> layer map), total_outputs = first_wave[L]. The backward ADDS dW_l / db_l into the tables'
 * buffers and writes dx [B][I] (optional); dyptr[l*halves + h] is the gradient of block h of layer l (0 = unused output).
 * Null tables and entries. wptr, dyptr and gwptr are tables of L (dyptr: L*halves) entries and must not be null; every wptr[l] must
 * point to a weight. Forward: bptr == NULL = no layer has a bias; a bptr that is given has L non-null entries. Backward: gwptr[l] == 0 =
 * the weight of layer l is frozen (its bias still trains through gbptr[l]); gbptr == NULL = no bias trains, gbptr[l] == 0 = that bias is
 * frozen; a frozen buffer is neither read nor written. dx == NULL = no input gradient: then no workspace is used and workspace may be NULL
 * with any workspace_bytes. With dx the workspace is checked before anything is launched: a call refused with HWG_ERR_WORKSPACE has
 * written nothing. */
int hwg_linear_bank_fwd(const float* x, const void* wptr, const void* bptr, const int* O, const int* first_wave, const void* off, int L, int B,
                        int I, int halves, int total_outputs, float* y, void* stream);
size_t hwg_linear_bank_bwd_workspace(int total_outputs, int B, int I);
int hwg_linear_bank_bwd(const float* x, const void* dyptr, const void* wptr, const void* gwptr, const void* gbptr, const int* O,
                        const int* first_wave, int L, int B, int I, int halves, int total_outputs, float* dx, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Chain of L square Linear(D,D)+LeakyReLU layers (the generator's style-embedding MLP, pure_gen.py:29-38) in one single-workgroup
 * launch per direction: h_{l+1} = lrelu(W_l h_l + b_l, slope). acts [L+1][B][D] receives every h_l (acts[0] = x, acts[L] = output) and is
 * what the backward consumes; the backward ADDS dW_l / db_l into the tables' buffers (null entry = frozen) and writes dx (optional).
 * D = 64 or 128, L <= 8; forward: any B (one workgroup per 8 / 16 rows), backward: B <= 16.
 * Null tables and entries. wptr and bptr (forward) are tables of L non-null entries: a chain layer always has a bias. Backward: gwptr is a
 * table of L entries, gwptr[l] == 0 = the weight of layer l is frozen; gbptr == NULL = no bias trains, gbptr[l] == 0 = that bias is
 * frozen; a frozen buffer is neither read nor written, the data gradient still passes through the layer. dx == NULL = no input gradient. */
int hwg_mlp_chain_fwd(const float* x, const void* wptr, const void* bptr, int L, int B, int D, float slope, float* acts, void* stream);
int hwg_mlp_chain_bwd(const float* dout, const float* acts, const void* wptr, const void* gwptr, const void* gbptr, int L, int B, int D,
                      float slope, float* dx, void* stream);
/* the same backward pass as two launches: the sequential chain of data gradients on one workgroup (every delta_l kept in the workspace), then
 * all layers' dW_l / db_l in parallel (L x D*D/1024 workgroups) - 69 -> ~25 us per call; bit-identical to hwg_mlp_chain_bwd */
size_t hwg_mlp_chain_bwd_workspace(int L, int B, int D);
int hwg_mlp_chain_bwd_split(const float* dout, const float* acts, const void* wptr, const void* gwptr, const void* gbptr, int L, int B, int D,
                            float slope, float* dx, void* workspace, size_t workspace_bytes, void* stream);

/* Grouped "one expert per window" layers for the 79 character-style experts (model/char_style.py:84-124, 210-235).
 * x [n][R][Cin] -> y [n][R][Cout]; wptr/bptr are device tables (int64 addresses, one per expert) of weights in the Conv1d layout
 * [Cout][Cin][S] and biases; R <= 8; (S, pad) is (1, 0) or (3, 1). Windows are sorted by expert: seg_start[G+1] / seg_eid[G] describe
 * the runs; the rows of a run (windows x R positions) are cut into work tiles of at most 64 rows, tile_seg[t] = run and
 * tile_row0[t] = first row of tile t. Every run is one small GEMM on the matrix cores against its expert's weights.
 * wgrad and segment_accumulate ADD into the buffers addressed by the grad-pointer tables.
 * Null tables and entries. The tables are indexed by expert id; only the entries of the experts named in seg_eid are read, and those must
 * not be null (an absent expert's entry may hold anything; its buffers are never touched). bptr == NULL (forward) = no bias is added,
 * gbptr == NULL (wgrad) = no bias gradient is formed. Forward: Cin % 8 == 0; data gradient: Cout % 4 == 0; wgrad: ntiles >= G. */
int hwg_grouped_conv1d_fwd(const float* x, const int* seg_start, const int* seg_eid, const int* tile_seg, const int* tile_row0, int ntiles,
                           const void* wptr, const void* bptr, float* y, int R, int Cin, int Cout, int S, int pad, void* stream);
int hwg_grouped_conv1d_dgrad(const float* dy, const int* seg_start, const int* seg_eid, const int* tile_seg, const int* tile_row0, int ntiles,
                             const void* wptr, float* dx, int R, int Cin, int Cout, int S, int pad, void* stream);
size_t hwg_grouped_conv1d_wgrad_workspace(int ntiles, int Cin, int Cout, int S);
/* the weight gradient uses its own tiling of at most tile_rows rows per tile; run_tile0[G+1] = first tile of every run. The tiles'
 * partial images go to the workspace and are added to the experts' buffers in tile order (deterministic). */
int hwg_grouped_conv1d_wgrad(const float* dy, const float* x, const int* seg_start, const int* seg_eid, int G, const int* tile_seg,
                             const int* tile_row0, const int* run_tile0, int ntiles, int tile_rows, const void* gwptr, const void* gbptr, int R,
                             int Cin, int Cout, int S, int pad, void* workspace, size_t workspace_bytes, void* stream);
int hwg_gather_rows_ptr(const void* ptrs, const int* eid, float* out, int n, int C, void* stream);
int hwg_segment_accumulate_ptr(const float* rows, const int* seg_start, const int* seg_eid, int G, const void* gptrs, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-tensor optimizer-side ops (trainer/hw_with_style_trainer.py:300-391) and RNG.
 * Tensor lists are device tables: ptrs (int64 addresses, 0 = absent), numel (int64), and a chunk table
 * (chunk_tensor int32, chunk_off int64) with `chunk` elements per entry.
 * ------------------------------------------------------------------------------------------ */
/* out_sums[t] = sum |x| over tensor t (all nt tensors; absent ones give 0). Two stages, no atomics: per-chunk partials (chunk_partials,
 * nchunks doubles of scratch), then the chunks of a tensor - consecutive entries of the chunk table - are added in table order. */
int hwg_mt_abs_sum(const void* ptrs, const void* numel, const void* chunk_tensor, const void* chunk_off, int nchunks, int chunk,
                   int nt, double* chunk_partials, double* out_sums, void* stream);
/* the same for nsets tensor lists at once (ptrs [nsets][nt], chunk_partials [nsets][nchunks], out_sums [nsets][nt]): the current gradients and
 * every stashed set of a balanced lesson (trainer :340-359) in two launches instead of two per set; per set the arithmetic of hwg_mt_abs_sum */
int hwg_mt_abs_sum_sets(const void* ptrs, int nsets, const void* numel, const void* chunk_tensor, const void* chunk_off, int nchunks,
                        int chunk, int nt, double* chunk_partials, double* out_sums, void* stream);
int hwg_mt_balance_coef(const double* sumD, const double* sumR, const void* numel, const void* ptr_grad, const void* ptr_R,
                        const float* xs, int nsets, int nt, float* coef, void* stream);
int hwg_mt_axpy(const void* ptrs_dst, const void* ptrs_src, const float* coef, const void* numel, const void* chunk_tensor,
                const void* chunk_off, int nchunks, int chunk, void* stream);
/* dst_t += coef[0][t] * src_0t, then += coef[1][t] * src_1t, ...: the balanced adds of all stashed sets (trainer :360-377) in ONE pass over the
 * gradients (ptrs_src, coef: [nsets][nt], nsets <= 8) - per element the same chain of fused multiply-adds in the same order as nsets calls of
 * hwg_mt_axpy, bit for bit */
int hwg_mt_axpy_sets(const void* ptrs_dst, const void* ptrs_src, const float* coef, int nsets, int nt, const void* numel,
                     const void* chunk_tensor, const void* chunk_off, int nchunks, int chunk, void* stream);
/* op 0: a=0, 1: clamp(a,-c,c), 2: flag |= any non-finite, 3: b=a, 4: b=a then a=0 */
int hwg_mt_unary(const void* ptrs_a, const void* ptrs_b, int op, float c, int* flag, const void* numel, const void* chunk_tensor,
                 const void* chunk_off, int nchunks, int chunk, void* stream);
int hwg_mt_adam(const void* ptrs_p, const void* ptrs_g, const void* ptrs_m, const void* ptrs_v, const float* step_size,
                const float* bc2_sqrt, float beta1, float beta2, float eps, float clip, const void* numel, const void* chunk_tensor,
                const void* chunk_off, int nchunks, int chunk, void* stream);
/* clip_grad_value_(clip) + the NaN asserts + Adam of one stepping lesson in ONE launch (trainer/hw_with_style_trainer.py:379-391): a tensor with a
 * gradient entry and a NULL parameter entry is clipped only (touched, but not stepped in this lesson); a tensor with both is clipped and
 * stepped, *flag |= 1 when a freshly written parameter is not finite (flag is sticky: never cleared here). Gradients are stored back only
 * where clipping changed them. Same arithmetic per element as hwg_mt_unary(op 1) followed by hwg_mt_adam. */
int hwg_mt_clip_adam(const void* ptrs_p, const void* ptrs_g, const void* ptrs_m, const void* ptrs_v, const float* step_size,
                     const float* bc2_sqrt, float beta1, float beta2, float eps, float clip, int* flag, const void* numel,
                     const void* chunk_tensor, const void* chunk_off, int nchunks, int chunk, void* stream);
/* Weight averaging (SWA / EMA) over the same tables. avg is one fp32 buffer laid out like the flat gradient buffer: tensor t at float
 * offsets[t] (int64 table, multiples of 4), the padding between segments is never touched. A chunk-table entry ends where the tensor's next
 * entry begins, so no chunk size is passed.
 * hwg_weight_average: avg_t[j] = fadd_rn(fmul_rn(avg_t[j], one_minus_alpha), fmul_rn(p_t[j], alpha)) - two roundings and no FMA, bit for bit
 * torch's `a *= (1 - alpha); a += p * alpha` on fp32 tensors; the parameters are only read.
 * hwg_weight_exchange: p_t[j] <-> avg_t[j] in place; two calls restore every bit. */
int hwg_weight_average(const void* param_ptrs, const void* chunk_tensor, const void* chunk_off, const void* numel, const void* offsets,
                       int nchunks, float* avg, float one_minus_alpha, float alpha, void* stream);
int hwg_weight_exchange(const void* param_ptrs, const void* chunk_tensor, const void* chunk_off, const void* numel, const void* offsets,
                        int nchunks, float* avg, void* stream);
int hwg_randn(float* out, long long n, unsigned long long seed, unsigned long long offset, void* stream);
int hwg_dropmask(float* out, long long n, float p, unsigned long long seed, unsigned long long offset, void* stream);
/* the Dropout2d masks of one network pass in ONE launch (model/discriminator_ap.py:84-131 has up to six, model/autoencoder.py:341-410 four):
 * nseg (<= 16) segments of seg_elems[j] floats (multiples of 4; HOST arrays, read during the call) laid out back to back in `out`, segment
 * j with drop probability seg_p[j]. Same values as nseg consecutive hwg_dropmask calls at offsets offset + sum_{i<j} seg_elems[i] / 4. */
int hwg_dropmask_multi(float* out, int nseg, const long long* seg_elems, const float* seg_p, unsigned long long seed,
                       unsigned long long offset, void* stream);

/* `insert_spaces` (model/hw_with_style.py:302-328) with the device generator: plan = per character of every line the number of blank columns
 * before it and of repeats, drawn as round(N(count, count_std)) / round(N(duplicates, dup_std)) (half to even, negative -> 0) from Philox block
 * offset + (line * L + character); lens_max [B+1] = expanded length per line, then max(ceil(max counts), 3) (the reference's tail padding);
 * fill writes the character runs into the zero-initialised index map idx [T][B] (0 = blank). counts [L][B][2], label [L][B]. */
int hwg_insert_spaces_plan(const float* counts, const int* label_lengths, int L, int B, float count_std, float dup_std, int count_duplicates,
                           unsigned long long seed, unsigned long long offset, int* reps, int* starts, int* lens_max, void* stream);
int hwg_insert_spaces_fill(const int* label, const int* label_lengths, const int* reps, const int* starts, int L, int B, int T, int* idx,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Line augmentation of the recogniser pre-training on the collated batch: Tensmeyer brightness + mesh warp
 * (utils/augmentation.py:5-31 tensmeyer_brightness / apply_tensmeyer_brightness, utils/grid_distortion.py:11-66 warp_image; called per
 * line from datasets/hw_dataset.py:143-152, datasets/author_hw_dataset.py:429-432, datasets/author_rimeslines_dataset.py:428-434).
 * x / y: [B][H][W] fp32 images holding 1 - level/128 (levels 0..255), padding columns -1. Per-line tables on the device:
 *   lines_i [B][4] int32 = {valid width w, lattice rows gy (0: no warp), lattice columns gx, first valid column x_off};
 *   lines_f [B][lf_stride] = {foreground scale, background scale, row sigma, column sigma, src_y[GY], src_x[GX]}: the control lattice of
 *     grid_distortion.py:25-41 (src_y[i], src_x[j] = the np.mgrid coordinates), GY / GX = the batch's largest gy / gx;
 *   draws [B][draw_stride] = {fg, bg, row displacement [gy][gx], column displacement [gy][gx]}: unit draws (hwg_randn) that the kernels
 *     multiply by the scales / sigmas of lines_f, or explicit values with scales of 1.
 * hwg_augment_stats: stats [B][258] int32 = {Otsu threshold t (lowest level maximising the between-class variance, fp64), border level m =
 *   round-half-even(mean of the re-lit line), LUT q(p) = trunc(clamp(p + (p > t ? bg : fg), 0, 255)) in fp32}; one workgroup per line.
 * hwg_augment_warp: y = bilinear resample (taps outside the line = m, result rounded half to even to a level) of the LUT-mapped line at the
 *   inverse map = piecewise-linear interpolation of lattice -> lattice + displacement over the lattice cells, each split along the diagonal
 *   that is locally Delaunay (what scipy.interpolate.griddata(destination, source, pixels, "linear") computes wherever every lattice
 *   triangle is a Delaunay triangle); pixels outside the mesh take m; lines with gy = 0, H <= 5 or w <= 5 get the LUT only
 *   (grid_distortion.py:12). map_out (optional, tests): [B][2][H][W] = (map_y, map_x) in line coordinates, NaN outside the mesh / the line.
 * lines_i is a device array, the caller's to check (ops.augment_lines validates it on the host before the upload). Both entries CLAMP an
 *   extent that is bad all the same rather than refusing the row: x_off' = max(x_off, 0), w' = max(min(w, W - x_off'), 0); the row is then
 *   exactly the row of the table (w', x_off'), and nothing is read past the image row.
 * ------------------------------------------------------------------------------------------ */
int hwg_augment_stats(const float* x, const int* lines_i, const float* lines_f, int lf_stride, const float* draws, int draw_stride,
                      int B, int H, int W, int* stats, void* stream);
int hwg_augment_warp(const float* x, const int* lines_i, const float* lines_f, int lf_stride, const float* draws, int draw_stride,
                     const int* stats, int B, int H, int W, int GY, int GX, float* y, float* map_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Generated lines as 8-bit grey pictures, ragged (generate.py:303, 344, 426, 496, 525, 622, 692, 718, 786:
 * ((1 - im) * 127.5).astype(np.uint8), there on the host after downloading the padded fp32 batch).
 * img: the generator's image [B][1][H][W] fp32; widths [B] int32 and offsets [B] int64 on the device: line b becomes the H x widths[b]
 * picture out[offsets[b] : offsets[b] + H * widths[b]] (row stride widths[b]); columns >= widths[b] are never read.
 * Pixel: (1 - x) * 127.5 in fp32, clamped to [0, 255] (numpy wraps outside [-1, 1]), NaN -> 0, truncated toward zero.
 * W % 4 == 0 (checked here); 4 <= widths[b] <= W, widths[b] % 4 == 0 and offsets[b] % 4 == 0 are the caller's to check (device arrays:
 * ops.lines_to_u8 validates them on the host before the upload). One 16-byte load and one 32-bit store per lane. A width that is bad all
 * the same is CLAMPED, the row is not refused: the kernel works with w' = min(widths[b], W) & ~3 (nothing for w' <= 0) - row stride w',
 * no read past the image row, no byte outside out[offsets[b] : offsets[b] + H * w'] written.
 * ------------------------------------------------------------------------------------------ */
int hwg_lines_to_u8(const float* img, int B, int H, int W, const int* widths, const long long* offsets, unsigned char* out, void* stream);

/* The inverse: ragged 8-bit lines in the layout hwg_lines_to_u8 writes -> a collated fp32 batch, mixed with the rows of a real batch
 * (datasets/hw_dataset.py:21-67 collate over :135 `1 - img / 128` items - there on the host, per line read from disk).
 * One launch writes every element of out [B][1][H][W]. select [B] int32 (device): select[b] = k >= 0 takes line k of the pool - pixels
 * (uint8), offsets [n_lines] int64, widths [n_lines] int32, all on the device; row-major H x widths[k] at pixels + offsets[k] - as
 * out[b][y][x] = 1 - p / 128 for x < widths[k] and -1 (the padding constant) beyond; select[b] = -1 - r copies row r of
 * real [Br][1][H][Wr] (fp32, any Wr <= W, 4-byte aligned) and writes -1 beyond column Wr. real may be NULL (then Br and Wr are ignored).
 * Every level is exact in fp32. One 32-bit load (pool row) or four scalar loads (real row) and one 16-byte store per lane; columns >=
 * widths[k] are never read.
 * Checked here: no NULL, B, H, W > 0, W % 4 == 0, out 16-byte and pixels 4-byte aligned, Wr <= W, and min_select - the smallest entry of
 * select as the caller states it (the table itself is a device array) - not below -Br, i.e. not negative without a real batch. The tables
 * are the caller's to check (ops.lines_from_u8 validates them on the host before the upload); the kernel turns a row whose entry is bad
 * all the same (k >= n_lines, r >= Br, a width that is no multiple of 4 or above W, an offset that is negative or no multiple of 4, a line
 * that ends behind pixel_bytes) into padding without reading anything through it. The bounds hold for ANY 64-bit offset: they are the
 * predicates of csrc/table_guard.h, which never form off + H * w (that sum wraps for an offset near 2^63) but compare H * w with
 * pixel_bytes - off. The same holds for every entry below that reads a pool or a frame table. */
int hwg_lines_from_u8(const unsigned char* pixels, long long pixel_bytes, const long long* offsets, const int* widths, int n_lines,
                      const int* select, int min_select, const float* real, int Br, int Wr, int B, int H, int W, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Line images of any height fitted to the recognisers' height (csrc/fit_lines.hip; datasets/hw_dataset.py:128-131 resize + :157
 * `1 - img / 128` + :21-67 collate, generate.py:655-663 - there per line on the host, through cv2.resize; this package's loaders use PIL,
 * data/author_hw_dataset.py `_resize`, and PIL's bytes are what this entry reproduces).
 * pixels: a ragged uint8 pool of grey pictures of differing heights and widths, any byte offsets. lines [B][10] int64 (device), per output
 * row b: {byte offset of the row-major in_h x in_w picture, in_h, in_w, out_w, htab, hks, vtab, vks, order, 0}. coef (int32, device, coef_elems
 * elements): the axis tables. The table of an axis of `in` pixels resized to `n` (n = out_w for the horizontal axis at element htab with
 * ks = hks, n = H for the vertical one at vtab with ks = vks) is first[n], count[n], k[n][ks]: output index i reads the pixels first[i] ..
 * first[i] + count[i] - 1 of its row / column with the 22-bit fixed-point weights k[i][0 .. count[i]). ks = 0: the pass is skipped, legal
 * only where in == n. The tables are Pillow's (Resample.c, 8 bits per channel, bicubic a = -0.5), computed on the host in fp64
 * (data/fit_tables.py resample_table).
 * One launch writes every element of out [B][1][H][W] fp32: the horizontal pass first, acc = 2^21 + sum pixel * k in 32-bit integers,
 * byte = clamp(acc >> 22, 0, 255), into an 8-bit intermediate that stays in LDS; then the vertical pass over those bytes in the same
 * arithmetic; element = 1 - byte / 128 (exact in fp32) for columns < out_w, -1 (the padding constant) beyond. With the host's tables
 * this is Image.resize((out_w, H), Image.BICUBIC) of an `L` image bit for bit. order = 1 runs the vertical pass first and the horizontal
 * pass over its bytes, as Image.resize does for a picture more than 100 times as tall as wide that shrinks vertically; it is served for
 * pictures of at most 64 columns. One workgroup owns 64 output columns of one line; a line's
 * values depend on its own entry alone (no atomics, nothing shared between workgroups).
 * Limits, checked here before the launch (HWG_ERR_ARG): no NULL; B, H, W, pixel_bytes, coef_elems, max_in_h > 0; B <= 65535, H <= 1024,
 * W <= 2^20, W % 4 == 0; max_in_h - the tallest picture as the caller states it, it sizes the LDS - <= 1024; out and coef 16-byte
 * aligned, lines 8-byte aligned. The tables are the caller's to check (device arrays: ops.fit_lines builds them on the host); the kernel
 * turns a row whose entry is bad all the same into padding (the WHOLE row, every workgroup of it checks the whole entry) without reading
 * anything through it: a picture that does not lie inside pixel_bytes (csrc/table_guard.h, any 64-bit offset), in_h outside
 * [1, max_in_h], in_w outside [1, 2^20], out_w outside [1, W], ks outside [0, 2^16] or 0 where the sizes differ, an axis table that starts
 * at no multiple of 4 or starts or ends outside coef_elems, a window with first < 0, count < 0, count > ks or first + count > in, an order other than 0 or 1, or 1 with in_w > 64.
 * ------------------------------------------------------------------------------------------ */
int hwg_fit_lines(const unsigned char* pixels, long long pixel_bytes, const long long* lines, const int* coef, long long coef_elems,
                  int max_in_h, int B, int H, int W, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Foreground masks of grey lines (csrc/fg_mask.hip; datasets/author_hw_dataset.py:197-220: cv2.threshold(BINARY + OTSU), 255 - that,
 * cv2.dilate with getStructuringElement(MORPH_ELLIPSE, (9, 9)) - there per line on the host).
 * pixels (uint8, pixel_bytes of them), offsets [B] int64 and widths [B] int32 on the device: line b is the row-major H x widths[b] picture
 * at pixels + offsets[b]; any width >= 1 and any byte offset. out: a pool of the same layout (a different buffer); line b's bytes become
 * 255 (foreground) or 0, no other byte of out is written. Threshold t per line: the Otsu level of hwg_augment_stats (256-bin histogram in
 * exact integers, (s0 w1 - s1 w0)^2 / (w0 w1) with the square and the quotient each rounded once in fp64, lowest level on ties, 0 for a
 * constant line); foreground p <= t; dilated by the 57-cell ellipse (half-widths 0 3 3 4 4 4 3 3 0 for dy = -4 .. 4), pixels outside the
 * line never count. thresholds (optional): [B] int32, t per line. One launch, one workgroup per line, no atomics.
 * Checked here: no NULL, out != pixels, B > 0, 1 <= H <= 64. The tables are the caller's to check (device arrays: ops.fg_masks validates
 * them on the host before the upload - widths >= 1, H * width <= 2^22 for the exact sums, every line inside the pool, no two lines
 * overlapping); the kernel skips a line whose entry is bad all the same - width < 1, a negative offset, a line that ends behind
 * pixel_bytes, for any 64-bit offset (csrc/table_guard.h) - with threshold -1 and without touching anything: no byte of out is written,
 * the bytes the bad entry names included.
 * ------------------------------------------------------------------------------------------ */
int hwg_fg_masks(const unsigned char* pixels, long long pixel_bytes, const long long* offsets, const int* widths, int B, int H,
                 unsigned char* out, int* thresholds, void* stream);

/* ------------------------------------------------------------------------------------------
 * GAN batches from a device-resident line store (csrc/line_store.hip; datasets/author_hw_dataset.py:386-470 __getitem__ + :27-112 collate
 * with utils/augmentation.py:61-72 affine_trans - there on the host per line read from disk, through cv2.warpAffine).
 * pixels: a ragged uint8 pool in the layout of hwg_fg_masks - offsets [n_lines] int64 and widths [n_lines] int32 on the device, line k the
 * row-major H x widths[k] picture at pixels + offsets[k], any width >= 1 and any byte offset. masks (optional): a second pool of the same
 * layout and size, bytes 0 / 255. Per output row b, device tables: line[b] int32 (which line), out_w[b] int32 (columns it fills),
 * strech[b] and m[b] fp64 (horizontal stretch; m = tan(skew), computed on the host).
 * One launch writes every element of out [B][1][H][W] fp32 and, with masks, of out_mask [B][1][H][W] fp32; W is any positive integer.
 * fp64 without contraction, in this order: h = H / 2.0; sx = ((double)x - m * ((double)y - h)) / strech; x0 = floor(sx); f = sx - x0;
 * p0, p1 = the bytes at columns x0, x0 + 1 of row y of the line, or the border value outside [0, widths[k]) (255 for lines, 0 for masks:
 * cv2.warpAffine's constant border, blended into the edge pixels); v = p0 + f * (p1 - p0).
 * Line: level = clamp(floor(v + 0.5), 0, 255), element 1 - level / 128 (exact in fp32). Mask: p = byte / 255, element (float)v.
 * Columns x >= out_w[b]: -1 in out, 0 in out_mask. strech = 1, m = 0 reproduces the line's bytes.
 * A lane owns 4 consecutive floats of the flat output (one 16-byte store per tensor, byte loads from the pool); out_elems: the floats out
 * (and out_mask) hold, at least B*H*W rounded up to 4 - the surplus elements of the last word are written as padding, none beyond them.
 * Checked here before the launch: no NULL, masks and out_mask both given or both absent, B, H, W, n_lines, pixel_bytes > 0, out / out_mask
 * 16-byte aligned, the tables aligned to their element, B*H*W in 64 bits, out_elems. The tables are the caller's to check (device arrays:
 * ops.store_batch validates them on the host before the upload - line in [0, n_lines), 0 <= out_w <= W, strech finite and positive, m
 * finite, every line inside pixel_bytes, no two lines overlapping); the kernel turns a row whose entry is bad all the same into padding
 * (-1 in out, 0 in out_mask) without reading anything through it; "inside pixel_bytes" holds for any 64-bit offset (csrc/table_guard.h).
 * ------------------------------------------------------------------------------------------ */
int hwg_store_batch(const unsigned char* pixels, const unsigned char* masks, long long pixel_bytes, const long long* offsets,
                    const int* widths, int n_lines, const int* line, const int* out_w, const double* strech, const double* m, int B, int H,
                    int W, float* out, float* out_mask, long long out_elems, void* stream);

/* ------------------------------------------------------------------------------------------
 * Recogniser pre-training batches from the device-resident line store (csrc/store_warp.hip): the brightness + mesh warp of
 * hwg_augment_stats / hwg_augment_warp executed on the bytes of the pool (the layout of hwg_store_batch: pixels, offsets [n_lines] int64,
 * widths [n_lines] int32 on the device) instead of on an uploaded, collated fp32 batch. The arithmetic is that of the two entry points above,
 * from the same source (csrc/augment_warp.h): a batch through hwg_store_warp_batch equals the same lines collated, uploaded and put through
 * hwg_augment_stats + hwg_augment_warp with the same tables, bit for bit, padding included.
 * hwg_store_line_stats: once per pool, one workgroup per line -> thr [n_lines] int32, the Otsu level of hwg_augment_stats (exact integer
 *   sums, fp64 between-class variance, lowest level on ties), and hist [n_lines][256] int32, the line's histogram. Both depend on the
 *   stored bytes alone. H * width <= 2^22 (the exact sums) is the caller's to check with the rest of the pool's tables
 *   (ops.store_line_stats, on the host); a line whose entry lies outside pixel_bytes gets thr -1 and an empty histogram, nothing is read.
 * hwg_store_warp_batch: one launch writes every element of out [B][1][H][W] (and of map_out [B][2][H][W], optional, tests; NaN outside
 *   the mesh / the line), W any positive integer. Per output row b: line[b] int32, the pool line it shows, and the tables of
 *   hwg_augment_warp - lines_i [B][4] = {w = widths[line[b]], gy, gx, x_off}, lines_f [B][lf_stride], draws [B][draw_stride], GY / GX the
 *   batch's largest lattice. One workgroup per row x 64 columns: LUT[256] in LDS from thr[line[b]] and the row's two draws (identity for
 *   scales or draws of 0: a row whose brightness is off), the border level round-half-even(sum hist * LUT / (H w)) by an exact integer
 *   reduction, then the lattice / diagonal / barycentric / bilinear path of hwg_augment_warp with taps LUT[pool byte]. Columns outside
 *   [x_off, x_off + w) are -1; rows with gy = 0, H <= 5 or w <= 5 get the LUT alone.
 *   Checked here before the launch: no NULL (map_out may be), B, H, W, n_lines, pixel_bytes > 0, B <= 65535, 0 <= GY <= 16, GX >= 0, the
 *   strides against the lattice, the tables and outputs aligned to their element, B*H*W in 64 bits and <= out_elems (the floats out holds).
 *   The tables are the caller's to check (device arrays: ops.store_warp_batch validates them on the host before the upload); the kernel
 *   turns a row whose entry is bad all the same - line outside [0, n_lines), a line outside pixel_bytes, w != widths[line], x_off < 0 or
 *   x_off + w > W - into padding (NaN in map_out) without reading anything through it. Both entries: "outside pixel_bytes" holds for any
 *   64-bit offset (csrc/table_guard.h).
 * ------------------------------------------------------------------------------------------ */
int hwg_store_line_stats(const unsigned char* pixels, long long pixel_bytes, const long long* offsets, const int* widths, int n_lines, int H,
                         int* thr, int* hist, void* stream);
int hwg_store_warp_batch(const unsigned char* pixels, long long pixel_bytes, const long long* offsets, const int* widths, int n_lines,
                         const int* thr, const int* hist, const int* line, const int* lines_i, const float* lines_f, int lf_stride,
                         const float* draws, int draw_stride, int B, int H, int W, int GY, int GX, float* out, float* map_out,
                         long long out_elems, void* stream);

/* ------------------------------------------------------------------------------------------
 * The stretch film's labels (csrc/stretch.hip; generate.py:830-852 interpolate_horz: per frame a dense one-hot, permute(1,2,0),
 * F.interpolate(scale_factor=s, mode='linear'), permute(2,0,1) - 79 times per film).
 * label [T][B] int32: the aligned line (generate.py:298 correct_pred), blanks 0. frames: a device array of F records. Frame f is the
 * one-hot of `label` re-sampled along time to T_out steps, written twice: as [B][T_out][ncls] at out_blc + off_blc (NHWC rows, what
 * the generator reads) and as [T_out][B][ncls] at out_lbc + off_lbc (the reference's time-major tensor); offsets count floats and are
 * multiples of 4. One launch writes every element of every frame, zeros included; nothing else of the two buffers is touched.
 * Arithmetic (torch's CPU kernel, bit for bit): identity != 0 (the host sets it where T_out == T: torch copies then, whatever s is)
 * gives the plain one-hot; otherwise src = fmaf(r, t + 0.5f, -0.5f) with ONE rounding, src = max(src, 0), i0 = min((int)src, T - 1),
 * i1 = min(i0 + 1, T - 1), w1 = src - i0, w0 = 1 - w1, out[c] = w0 * [label[i0] == c] + w1 * [label[i1] == c]. The host computes
 * T_out = floor((double)T * s) and r = (float)(1.0 / s).
 * Checked here before the launch: no NULL, T, B, ncls, max_T_out >= 1, 1 <= F <= 65535, T < 2^23, B * max_T_out * ncls below 2^31,
 * buffers 16-byte aligned. The table is the caller's to check (ops.stretch_onehot validates it on the host before the upload, and the
 * labels: a class outside [0, ncls) is an error there); a record that is bad all the same - T_out outside [1, max_T_out], a misaligned
 * block, a negative offset or a block that ends behind blc_elems / lbc_elems floats, for any 64-bit offset (csrc/table_guard.h) - writes
 * nothing to either buffer, and a label outside [0, ncls) matches no class. identity != 0 in a record whose T_out is not T is ignored:
 * the frame is re-sampled like any other (an identity frame of another length would read labels behind step T - 1).
 * ------------------------------------------------------------------------------------------ */
typedef struct hwg_stretch_frame {
  int T_out;                  /* steps of this frame                                   */
  float r;                    /* (float)(1.0 / s)                                      */
  int identity;               /* T_out == T: the plain one-hot                         */
  int reserved;
  long long off_blc, off_lbc; /* first float of the frame in out_blc / out_lbc         */
} hwg_stretch_frame;
int hwg_stretch_onehot(const int* label, int T, int B, int ncls, const hwg_stretch_frame* frames, int F, int max_T_out, float* out_blc,
                       long long blc_elems, float* out_lbc, long long lbc_elems, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sample sheets of GAN training (trainer/hw_with_style_trainer.py:992-1010: torchvision's save_image(1 - images, nrow, normalize=True),
 * there on the host after downloading the fp32 batch). x: images [B][1][H][W] fp32, n = B * H * W.
 * v = 1 - x; lo / hi = min / max of the finite v over the whole tensor; d = (float)max((double)hi - (double)lo, 1e-5);
 * level = trunc(clamp(((clamp(v, lo, hi) - lo) / d) * 255 + 0.5, 0, 255)), every operation rounded to fp32 on its own (no fma).
 * A NaN pixel is 0; v = +inf is 255, v = -inf is 0; without any finite value the whole sheet is 0.
 * B == 1: the sheet is the H x W image. Otherwise xmaps = min(nrow, B), ymaps = ceil(B / xmaps): (H + 2) ymaps + 2 rows of
 * (W + 2) xmaps + 2 bytes, image k at row (k / xmaps)(H + 2) + 2 and column (k % xmaps)(W + 2) + 2, everything else 0.
 * hwg_sheet_minmax: partials [n_parts][2] fp32 = (min, max) per workgroup, n_parts = hwg_sheet_parts(n) (at most 256); no atomics.
 * hwg_sheet_compose: folds the partials in every workgroup, then writes EVERY byte of the sheet, one aligned 32-bit store per lane
 * (a lane owns 4 consecutive bytes of the flat sheet; W is arbitrary). out_bytes: the bytes out holds, at least the sheet rounded up to
 * 4 bytes; the bytes between the sheet's end and that bound are written 0, none beyond it is touched.
 * Checked here before the launch: no NULL, B, H, W > 0, nrow >= 1, n_parts, sheet rows, columns and bytes fit int, out_bytes, x / partials
 * / out 4-byte aligned.
 * hwg_sheet_row_means: out[r] = fp32 mean of src[r * stride .. r * stride + n) for r < rows (the per-line discriminator means of
 * gen_text_*.txt, :1016-1021), one workgroup per row.
 * ------------------------------------------------------------------------------------------ */
int hwg_sheet_parts(long long n);
int hwg_sheet_minmax(const float* x, long long n, float* partials, int n_parts, void* stream);
int hwg_sheet_compose(const float* x, int B, int H, int W, int nrow, const float* partials, int n_parts, unsigned char* out,
                      long long out_bytes, void* stream);
int hwg_sheet_row_means(const float* src, long long stride, int rows, int n, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation pictures of new_eval.py (evaluators/hwdataset_eval.py:141-262, there numpy and OpenCV on the host): per line the real line
 * above its reconstruction, framed. image [B][1][H][Wi], recon [B][1][H][Wr] fp32 -> out [B][Hp][Wp][3] uint8, interleaved RGB,
 * Wp = max(Wi, Wr), Hp = 2 H + 2 + S; S = hwg_eval_strip_rows() = 50 with a caption strip (codes != NULL), else 0.
 * Level of a value x: v = 1 - (1 + x) / 2 in fp32, byte = trunc(clamp(v * 255, 0, 255)) - the fp32 product gives the exact product's byte for every v in [0, 1] -; NaN -> 0.
 * The narrower input is centred (|Wi - Wr| / 2 columns of level 0 on its left, the rest on its right); pr / pg = that left padding of
 * the real line / of the reconstruction. Rows 0..H-1 the real line, H and H+1 level 0, H+2..2H+1 the reconstruction.
 * Real frame (0,255,0): rows 0 and H over columns [pr, Wp - pr), rows 0..H-1 at columns pr and Wp-1-pr.
 * Reconstruction frame (0,0,255): rows H+1 and 2H+1 over [pg, Wp - pg), rows H+2..2H+1 at columns pg and Wp-1-pg.
 * Strip: S rows of level 0 below; cell j of line b shows glyph codes[b * L + j] of atlas [G][gh][gw] (grey bytes) at columns
 * 2 + j gw .., rows (S - gh) / 2 .. of the strip, clipped at Wp; a negative code (and a code >= G) leaves the cell empty. atlas and codes
 * are device arrays; without a strip atlas, G, gh, gw, codes, L are NULL / 0.
 * One launch writes EVERY byte of out, one aligned 32-bit store per lane; out_bytes: the bytes out holds, at least 3 B Hp Wp rounded up
 * to 4; the bytes between the pictures' end and that bound are written 0, none beyond it is touched.
 * Checked here before the launch: no NULL, sizes > 0, gh <= S, everything fits int, out_bytes, image / recon / codes / out 4-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int hwg_eval_strip_rows(void);
int hwg_eval_pairs(const float* image, const float* recon, int B, int H, int Wi, int Wr, const unsigned char* atlas, int G, int gh, int gw,
                   const int* codes, int L, unsigned char* out, long long out_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Recognition error rates on the device (trainer/hw_with_style_trainer.py:894-914 getCER, utils/string_utils.py naive_decode,
 * utils/error_rates.py:2-26 cer / wer - there on the host, after downloading the whole prediction).
 * pred [T][B][C] fp32 (the recogniser's output as it stands); class_code [C] int32: the code point class c compares as (32 for every
 * white-space class, lower-cased for a case-insensitive comparison; entry 0, the blank, is unused); ref_codes / ref_offsets [B+1] int32: the
 * reference lines as code points, ragged, already white-space normalised (and lower-cased) by the host; max_ref_len: the longest of them.
 * out int32 [8 * B + B * T]: per line stats[8] = {decoded length, character edit distance, hypothesis characters after white-space
 * normalisation, word edit distance, hypothesis words, 0, 0, 0}, then decoded [B][T]: the greedy class ids before normalisation
 * (row b: stats[0] ids, then zeros).
 * Arg-max as np.argmax (first maximum; a NaN beats every number, the first NaN wins); greedy CTC (class 0 dropped, a class equal to its
 * predecessor in the raw sequence dropped); hypothesis as " ".join(h.split()); Levenshtein with unit costs over code points, and over words
 * split at spaces (two words are equal only if all their code points are).
 * Limits, checked here before any launch: T <= 8192, C <= 1024, max_ref_len <= 2047. Two launches: row arg-max, one wavefront per line.
 * ------------------------------------------------------------------------------------------ */
int hwg_ctc_error_rates(const float* pred, int T, int B, int C, const int* class_code, const int* ref_codes, const int* ref_offsets,
                        int max_ref_len, int* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * CTC prefix beam search in front of the same counts (csrc/ctc_beam.hip; the reference decodes greedily only - this is the standard
 * decoder of a CTC-trained model, which sums the alignments of a text instead of scoring the single best one).
 * pred [T][B][C] fp32, read as log-probabilities as they stand (no renormalisation; class 0 the blank; a NaN reads as -inf). Per line a
 * beam of at most `beam` prefixes (sequences of classes 1 .. C-1), each with pb / pnb, the log-mass of its alignments ending in a blank /
 * in a non-blank, tot = pb (+) pnb with (+) = log-add-exp; start {(): pb 0, pnb -inf}. Frame t, for every beam prefix l, into a fresh table:
 *   new[l].pb (+)= lp[t][0] + tot(l);   l not empty: new[l].pnb (+)= lp[t][last(l)] + pnb(l);
 *   every c >= 1: new[l+c].pnb (+)= lp[t][c] + (pb(l) if c == last(l) else tot(l))
 * (l+c may itself be in the beam: one entry - prefixes are equal when their class sequences are, decided on the trie node, never by a
 * hash alone), then the `beam` entries of largest tot; a tot of -inf never enters. Of exactly equal totals the candidate of the earlier
 * (better) beam slot wins, within a slot the prefix itself before its extensions in ascending class order. Fixed summation orders: two
 * runs give the same bits, a line's result depends neither on B nor on the other lines.
 * out: the layout of hwg_ctc_error_rates - per line stats[8], then decoded [B][T]: the prefix of largest final tot (the empty text when
 * the beam is empty), row b: stats[0] ids, then zeros; the stats are those of that text. scores fp32 [B][beam]: the final totals,
 * descending, padded with -inf. ws: hwg_ctc_beam_workspace(T, B, C, beam) bytes, 8-byte aligned, contents irrelevant; HWG_ERR_WORKSPACE
 * when it is NULL or smaller. Every element of out and scores is written.
 * Limits, checked here before any launch: 1 <= beam <= 32, T <= 2048, C <= 1024, max_ref_len <= 2047; pred, out, scores 4-byte aligned.
 * Two launches: one workgroup per line with the frame loop inside, then the line kernel of hwg_ctc_error_rates on the best prefix
 * written as its shortest CTC path.
 * ------------------------------------------------------------------------------------------ */
size_t hwg_ctc_beam_workspace(int T, int B, int C, int beam);
int hwg_ctc_beam_error_rates(const float* pred, int T, int B, int C, int beam, const int* class_code, const int* ref_codes,
                             const int* ref_offsets, int max_ref_len, int* out, float* scores, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Writer retrieval over style vectors (eval_writer_id.py:15-29 topN over the :70-81 all-pairs l1 / l2 / gt matrices - there nested
 * Python loops, two N x N fp64 matrices and a Python sort per row).
 * styles [N][D] fp32, author_id [N] int32 (equal ids = same writer); metric 0: sum |a - b|, 1: sum (a - b)^2 (no root), both one fp32
 * chain over d ascending. Row i's columns are ordered by the key (distance, column) - a stable sort by distance -; pos_i(j) is column
 * j's place in that order. first_rank [N] int32: min{pos_i(j) : author_id[j] == author_id[i], pos_i(j) >= 1} (j == i included: the row's
 * own column counts unless it is at place 0), N where no such column exists; nearest_same [N] fp32: the distance at that place, +inf
 * where there is none. Every entry of both is written. No N x N storage, no workspace: two launches (targets, counts), each computing
 * all distances, bit-identically.
 * Checked here before any launch: no NULL, N, D >= 1, metric 0 or 1, N <= 2^20, D <= 65536, styles 16-byte and the rest 4-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int hwg_writer_first_rank(const float* styles, const int* author_id, int N, int D, int metric, int* first_rank, float* nearest_same,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * One bidirectional LSTM layer (csrc/lstm.hip; torch.nn.LSTM gate order i, f, g, o and arithmetic, accurate expf / tanhf).
 * The input projection x W_ih^T + b_ih is NOT part of these calls (it is a linear layer, run and differentiated as one): xproj_f / xproj_r
 * are its two halves, [T][B][4H] each, for the forward and the reverse direction. whh_* [4H][H], bhh_* [4H].
 * y [T][B][2H]: forward direction in [..., :H], reverse in [..., H:]; step t reads h_{t-1} out of y's neighbouring time row.
 * training != 0: also writes gates [2][T][B][4H] (post-activation), c [2][T][B][H] and hseq [2][T+1][B][H] (direction 0: row t + 1 = h_t, row 0
 * zero; direction 1: row t = h_t, row T zero - so that rows 0..T-1 of direction 0 and rows 1..T of direction 1 are the h_prev matrices of the
 * W_hh gradient's GEMM). training == 0: gates / hseq may be NULL and c is a [2][2][B][H] ping-pong workspace.
 * One launch per time step, both directions in it; no allocation, no host synchronisation, nothing waits on another workgroup inside a
 * launch. Summation order of the recurrent dot product: fixed, documented at the top of csrc/lstm.hip (depends on H alone).
 * hwg_lstm_bwd walks t the other way: launch t forms dh_rec = dgates[t+-1] W_hh for its units from whh_t, the [2][H][4H] transposed image
 * written by hwg_lstm_pack_whh (once per weight epoch), then the gate backward, and writes dgates [2][T][B][4H] (= d xproj; its column sums
 * are d b_hh, dgates[d]^T hseq-rows[d] is d W_hh[d] - both through the existing kernels). dc_ws: [2][2][B][H] ping-pong workspace, [slot][direction]: the launch of
 * step n (n = 0 .. T-1 in the backward walk) writes dc_t f_t, the cell gradient handed to the next launch, to slot n & 1 and reads slot (n + 1) & 1;
 * after the call slot (T - 1) & 1 holds the last launch's value and, for T >= 2, the other slot the one before it.
 * Limits, checked before any launch: T, B >= 1, H a multiple of hwg_lstm_unit_slice() and <= 1024, T*B*4H < 2^31; W_hh, y, dgates and whh_t
 * 16-byte aligned. A batch wider than hwg_lstm_batch_tile(H) lines (the LDS image, min(32, 16384 / H)) is walked in tiles of that many.
 * ------------------------------------------------------------------------------------------ */
int hwg_lstm_unit_slice(void);
int hwg_lstm_batch_tile(int H);
int hwg_lstm_fwd(const float* xproj_f, const float* xproj_r, const float* whh_f, const float* whh_r, const float* bhh_f, const float* bhh_r,
                 float* y, float* gates, float* c, float* hseq, int T, int B, int H, int training, void* stream);
int hwg_lstm_bwd(const float* dy, const float* gates, const float* c, const float* whh_t, float* dgates, float* dc_ws, int T, int B, int H,
                 void* stream);
int hwg_lstm_pack_whh(const float* whh_f, const float* whh_r, int H, float* whh_t, void* stream);

/* ------------------------------------------------------------------------------------------
 * The style-space map of umap_styles.py (csrc/style_map.hip; reference umap_styles.py:105-110 - there umap-learn on the host).
 * hwg_knn_rows: styles [N][D] fp32 -> idx [N][K] int32, d2 [N][K] fp32: per row the K nearest OTHER rows (the row's own column is excluded
 * by index, an exact duplicate is a neighbour at distance 0), ascending by the key (d2, column); d2 = sum (a - b)^2 as one fp32 chain
 * fma(diff, diff, acc) over d ascending, the bits of hwg_writer_first_rank's squared L2. One launch, no workspace, nothing N x N.
 * Checked before the launch: no NULL, D >= 1, 1 <= K <= 64, K <= N - 1, N <= 2^20, D <= 65536, styles 16-byte, idx and d2 4-byte aligned.
 *
 * hwg_umap_layout: the layout epochs n = epoch_begin + 1 .. epoch_end of n_epochs over a graph in CSR form (row_ptr [N+1], col [E],
 * period_q [E] int32: edge e is drawn in epoch n iff (n * 65536) / period_q[e] > ((n - 1) * 65536) / period_q[e], integer division).
 * y [N][2] fp32 holds the positions before and after; y_scratch [N][2] is the second buffer: one launch per epoch reads one and writes
 * the other (an odd number of epochs starts with a copy), so epochs 0..2 then 2..5 leave the bytes of 0..5.
 * Epoch n, vertex i, all positions those at the start of the epoch, alpha = (float)(1 - (n - 1) / (double) n_epochs): per drawn edge e
 * (j = col[e]) the attraction 2 clamp(c (y_i - y_j), -4, 4) with c = -2 a b s^(b-1) / (a s^b + 1), s = |y_i - y_j|^2 (nothing if s = 0),
 * then for t = 0 .. neg-1 the repulsion from r = (word * N) >> 32, word = philox4x32-10(seed, (n E + e) ceil(neg / 4) + t / 4)[t % 4]:
 * nothing if r == i, else clamp(c (y_i - y_r), -4, 4) with c = 2 b / ((0.001 + s)(a s^b + 1)), (4, 4) if s = 0;
 * y_i' = y_i + alpha * sum (fp32, in the fixed order stated at the top of csrc/style_map.hip).
 * Checked before any launch: no NULL, y != y_scratch, N <= 2^20, E >= 1, 1 <= neg <= 16, 1 <= n_epochs <= 32767 (a period is at most
 * 65536 n_epochs), 0 <= epoch_begin <= epoch_end <= n_epochs, a, b positive and finite, y and y_scratch 8-byte aligned. What lies in
 * device memory - row_ptr monotone from 0 to E, 0 <= col < N, period_q >= 1 - is the caller's to check (ops.umap_graph does).
 * ------------------------------------------------------------------------------------------ */
int hwg_knn_rows(const float* styles, int N, int D, int K, int* idx, float* d2, void* stream);
int hwg_umap_layout(const int* row_ptr, const int* col, const int* period_q, int N, int E, float* y, float* y_scratch, int epoch_begin,
                    int epoch_end, int n_epochs, float a, float b, int neg, unsigned long long seed, void* stream);

/* ------------------------------------------------------------------------------------------
 * Same-writer / different-writer distances in style space (csrc/style_pairs.hip; reference play_styles.py:19-39 - there a double Python
 * loop over all N (N - 1) / 2 pairs and three Python lists of that length - and :43-53, the writer x writer mean / std matrices behind
 * its exit(), keyed by line where a writer was meant).
 * styles [N][D] fp32 with the rows ordered so that writer [N] int32 (values 0 .. A-1) never decreases. Per unordered pair i < j:
 * d2 = sum (a - b)^2 as one fp32 chain fma(diff, diff, acc) over d ascending (the bits of hwg_writer_first_rank's metric 1 and of
 * hwg_knn_rows), d = sqrt((double) d2). Per cell: count int64, sum of d and sumsq of (double) d2 in fp64, in a fixed order.
 *   mode 0: count, sum, sumsq [2]: cell 0 the pairs of one writer, cell 1 the pairs of two writers.
 *   mode 1: count, sum, sumsq [A][A]: cell (a, b) the pairs with one line of writer a and one of writer b ((a, a): both of a); (b, a)
 *           holds the same numbers as (a, b); a cell without pairs is (0, 0.0, 0.0).
 * d2_range [2] fp32: the smallest and the largest d2 over all pairs (+inf, -inf when N == 1).
 * edge2 [bins + 1] fp32 ascending with hist [2][bins] int64 (both or neither; neither: bins == 0): hist[0] over the pairs of one writer,
 * hist[1] over the pairs of two; a pair is counted in bin k iff edge2[k] <= d2 < edge2[k + 1], compared in fp32 on the bits of d2; pairs
 * below edge2[0], at or above edge2[bins] or with a NaN d2 are in no bin.
 * Every entry of every output is written; two calls on the same input give the same bits. Nothing N x N is stored, no floating-point
 * atomics (the histogram's counters are integer atomics), nothing crosses a workgroup inside a launch: mode 0 is two launches (sweep over
 * the upper triangle, reduce), mode 1 four (writer bounds, sweep, range, cells); with a histogram one memset in front.
 * workspace: hwg_style_pair_stats_workspace(N, A, mode) bytes (0 for sizes the entry point refuses), 16-byte aligned, contents ignored.
 * Checked here before any launch: no NULL (edge2 / hist excepted, as a pair), N, D >= 1, 1 <= A <= N, mode 0 or 1, 1 <= bins <= 256 with
 * edge2, N <= 2^20, D <= 65536, A <= 4096 in mode 1, styles and workspace 16-byte, count / sum / sumsq / hist 8-byte, writer / edge2 /
 * d2_range 4-byte aligned, workspace_bytes large enough. What lies in device memory is the caller's to check (ops.style_pair_stats does,
 * on the host): writer non-decreasing within 0 .. A-1, edge2 ascending. The kernels stay inside their buffers whatever it holds (ids
 * outside 0 .. A-1 are dropped), but the sums of an unsorted writer array mean nothing.
 * ------------------------------------------------------------------------------------------ */
size_t hwg_style_pair_stats_workspace(int N, int A, int mode);
int hwg_style_pair_stats(const float* styles, const int* writer, int N, int D, int A, int mode, const float* edge2, int bins,
                         long long* count, double* sum, double* sumsq, float* d2_range, long long* hist, void* workspace,
                         size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HWG_H_ */
