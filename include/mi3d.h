/*
 * mi3d.h — C ABI of libmi3d.so: the MI355X-native (gfx950, hand-written HIP) 3D U-Net training hot path.
 *
 * The reference (fransiskusbudi/multimodal_segmentation_project) has NO FFI/plugin boundary: its hot path is
 * reached through Python objects (models/unet.py UNet3D, models/unet_dann.py UNet3D, utils/metrics.py losses and
 * metrics, train_dann.py GradientReversal/DomainDiscriminator) whose arithmetic is delegated to PyTorch.  This
 * header is therefore the boundary a maintainer binds with ctypes underneath those objects (INTEGRATION.md shows
 * the stub); every entry point names the reference interface (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.  `stream` is a hipStream_t passed as void* (NULL = default).
 *   - the library NEVER allocates, frees or synchronises: every buffer (inputs, outputs, saved activations,
 *     scratch) is caller-owned device memory; sizes come from the *_workspace_bytes() queries.
 *   - return 0 on success; < 0 argument/shape/dtype error; > 0 hipError_t.  mi3d_last_error() (thread-local)
 *     describes the last failure.  No C++ exception crosses the boundary.
 *   - callable from any host thread (PyTorch runs backward on its autograd thread); launches go to the stream
 *     given; no thread-local device state is kept.
 *   - external tensor layout = PyTorch's: NCDHW contiguous, float32 data, int64 labels.  Internally activations
 *     are channels-last in `dtype` (MI3D_F32 exact path, MI3D_BF16 fast path with fp32 accumulation/statistics).
 */
#ifndef MI3D_H
#define MI3D_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI3D_DTYPE_F32 0
#define MI3D_DTYPE_BF16 1
#define MI3D_MAX_LEVELS 6

const char* mi3d_last_error(void);
int mi3d_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Whole-network plan: UNet3D forward / backward.
 * Replaces models/unet.py:64-90 (UNet3D.forward) and models/unet_dann.py:65-98 (forward with return_features),
 * i.e. DoubleConv blocks (unet.py:6-22: Conv3d k3 p1 -> BatchNorm3d -> ReLU -> Dropout3d, twice), MaxPool3d(2,2)
 * (:40,71), ConvTranspose3d(k2,s2) + cat(skip, x) (:56-58,79-84) and the final 1x1x1 conv (:62,87), plus their
 * autograd backward (train_unet.py:225 accelerator.backward).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct mi3d_unet_desc {
    int32_t in_channels, out_channels;      /* UNet3D(in_channels, out_channels, ...)  unet.py:34 */
    int32_t n_levels;                       /* len(features), <= MI3D_MAX_LEVELS */
    int32_t features[MI3D_MAX_LEVELS];      /* default [16,32,64,128] */
    int32_t N, D, H, W;                     /* per-GPU batch and volume; D,H,W divisible by 2^n_levels */
    int32_t dtype;                          /* internal activation dtype */
    float bn_momentum, bn_eps;              /* 0.1, 1e-5 (nn.BatchNorm3d defaults) */
} mi3d_unet_desc;

/* Parameter / buffer pointer tables follow nn.Module.parameters() / .buffers() order of the reference model:
 *   params : for each DoubleConv in [encoder.0..L-1, bottleneck] : conv0.w, conv0.b, bn0.w, bn0.b, conv1.w, conv1.b,
 *            bn1.w, bn1.b ; then upconvs.0..L-1 : w, b ; then decoder.0..L-1 (8 each) ; then final_conv.w, .b
 *   buffers: for each DoubleConv in [encoder..., bottleneck, decoder...] : bn0.running_mean, bn0.running_var,
 *            bn0.num_batches_tracked(int64), bn1.(same three)
 * grads uses the params order; entries may be NULL to skip a gradient. */
int mi3d_unet_num_params(const mi3d_unet_desc* d);
int mi3d_unet_num_buffers(const mi3d_unet_desc* d);
size_t mi3d_unet_workspace_bytes(const mi3d_unet_desc* d);
/* number of Dropout3d scale entries (sum over the 2*(2L+1) dropout layers of N*C); layout = block order
 * [encoder..., bottleneck, decoder...], half 0 then half 1, each [N][C] */
int64_t mi3d_unet_dropout_count(const mi3d_unet_desc* d);

/* training != 0: batch statistics + running-stat update (BN train mode); == 0: running stats (eval mode).
 * training == 2: batch statistics with the running-stat update DEFERRED -- buffers[i] of every running_mean slot then points
 * at a device double[2*C] side buffer (the running_var / num_batches_tracked slots are ignored) into which the forward
 * publishes (batch mean, unbiased batch variance); mi3d_unet_bn_apply_deferred applies them to the real buffers later.  For
 * two forwards of ONE model on two streams (train_dann.py:268-272: source then target): the second one's updates of the
 * shared buffers are applied after both have run, in the reference's order, bit-identically to the serial execution.
 * training | 4 (with 1 or 2): another forward runs beside this one on a second stream -- the BatchNorm apply passes stay thin
 * (a finalize launch per layer at levels 0-1) instead of the wide whole-CU consumers, which slow each other down there.
 * drop_scales: device float[mi3d_unet_dropout_count] holding 0 or 1/(1-p), or NULL (p = 0 / eval).
 * logits: device float (N,out_channels,D,H,W), or NULL: the 1x1x1 head is not run (DANN target pass, whose logits nobody reads;
 * or the caller runs head + loss with mi3d_unet_head_loss_forward).  gap_out: device float (N, 2*features[L-1]) or NULL
 * (unet_dann.py:77-79).  The workspace keeps everything backward needs until the next forward. */
int mi3d_unet_forward(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* buffers,
                      const float* drop_scales, int training, float* logits, float* gap_out, void* workspace,
                      size_t workspace_bytes, void* stream);

int mi3d_unet_bn_apply_deferred(const mi3d_unet_desc* d, void* const* buffers, const void* const* side, void* stream);

/* Inference forward (eval mode, no backward possible afterwards).  Replaces model.eval() + forward of
 * train_unet.py:259-305 (evaluate), test_model.py:242-251 and the frozen teacher of distill_unet.py:109-111,216-220:
 * eval-mode BatchNorm3d is folded into the preceding Conv3d (filter * gamma/sqrt(running_var+eps) at pack time, bias
 * replaced), ReLU runs in the conv epilogue, Dropout3d is the identity, and each conv writes the activated tensor
 * directly -- no raw conv outputs, statistics or saved activations.  Same workspace size as mi3d_unet_forward; buffers
 * (running statistics) are read-only here.  logits = NULL: as for mi3d_unet_forward. */
int mi3d_unet_infer(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* buffers, float* logits,
                    float* gap_out, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the last mi3d_unet_forward on this workspace.  dlogits (N,out,D,H,W) float or NULL (target pass of
 * DANN: only the GAP branch carries gradient, train_dann.py:271-285); dgap (N,2*features[L-1]) float or NULL, its
 * contribution is scaled by gap_scale (gradient reversal folds in as gap_scale = -lambda, train_dann.py:29).
 * accumulate != 0: grads += ; else grads = .
 * Segments allow the caller to interleave gradient all-reduces: segment 0 = final_conv,
 * 1..L = decoder.L-1..0 (+ its upconv), L+1 = bottleneck, L+2..2L+1 = encoder.L-1..0.  Run [seg_begin, seg_end). */
int mi3d_unet_num_segments(const mi3d_unet_desc* d);
int mi3d_unet_backward(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* grads,
                       const float* drop_scales, const float* dlogits, const float* dgap, float gap_scale,
                       int accumulate, int seg_begin, int seg_end, void* workspace, size_t workspace_bytes,
                       void* stream, void* aux_stream, void* const* events, int aux_join);
/* aux_stream/events (both NULL = single stream): a second hipStream_t and 4 hipEvent_t handles (mi3d_event_create).
 * The backward's critical path is then the input-gradient chain alone (train_unet.py:225 fixes no order between the two
 * gradients of a layer): the dy of every decoder conv at the full-resolution levels and of every conv at the deep levels is
 * kept in its own buffer, and those weight gradients run on aux_stream -- the decoder's under the latency-bound deep-level
 * chain, the deep levels' under the bandwidth-bound encoder backward -- behind at most three forks (events[0..2], recorded
 * on `stream`) per call.  events[3] is recorded on aux_stream when it has finished the call's work; aux_join != 0 makes
 * `stream` wait for it before the call returns (the call is then stream-ordered for the caller), aux_join == 0 leaves that
 * to the caller: whatever consumes the gradients (optimizer, gradient exchange) and the end of a hipGraph capture must wait
 * for events[3] / aux_stream.  Results are bit-identical to the single-stream route. */
/* Exchange marks (data-parallel step, round 4): events[i] is recorded on the backward's stream as soon as every gradient of the
 * segments <= segs[i] is complete -- set for the NEXT mi3d_unet_backward / _backward_loss call of the calling thread (n <= 4,
 * n = 0 clears).  The backward then stays ONE call over all segments (a call cut at an exchange costs a slab-sum launch and a
 * host round trip); the exchange stream waits for the mark (mi3d_stream_wait_event) and all-reduces the bucket while the
 * remaining segments run.  Marks are consumed by that call. */
int mi3d_unet_backward_marks(const int* segs, void* const* events, int n);
int mi3d_stream_wait_event(void* stream, void* event);
int mi3d_event_create(void** event_out);
int mi3d_event_destroy(void* event);
/* A non-blocking hipStream_t of a priority class: -1 = the device's highest, 0 = middle, +1 = lowest.  torch.cuda.Stream only
 * offers high / normal; the aux stream of the deferred weight gradients wants the LOWEST class, so that the wave dispatcher
 * gives a free workgroup slot to the data-gradient chain first.  The caller owns the stream (mi3d_stream_destroy). */
int mi3d_stream_create(int priority_class, void** stream_out);
int mi3d_stream_destroy(void* stream);
/* Route switches: every kernel-selection switch of the library ("no_persist", "no_fused_bwd", "conv8", ... -- the table
 * in INTEGRATION.md) is read from the environment (MI3D_<NAME>=<int>) ONCE, when the library is first used; afterwards only
 * these calls change one.  Debug / test interface: do not call it concurrently with launches; a captured hipGraph keeps the
 * routes it was captured with.  Unknown names fail. */
int mi3d_debug_set_route(const char* name, int value);
int mi3d_debug_get_route(const char* name, int* value_out);
int mi3d_debug_route_count(void);
const char* mi3d_debug_route_name(int index);
/* Measurement hook (bench.py `roofline`: HIP events around ONE kernel on the stream it is launched on, also the aux stream).
 * mi3d_time_next_conv3_kernel arms it for the calling thread: the next launch of `kind` for the layer (Cin, Cout as that
 * launcher sees them) records start/stop -- timing events from mi3d_timing_event_create -- tightly around its kernel.
 *   kind 0 = fused full-resolution conv backward (input + weight gradient in one launch; Cin, Cout of the layer)
 *        1 = stand-alone conv weight gradient (Cin, Cout of the layer)
 *        2 = persistent full-resolution conv with BatchNorm partial sums (the training forward; Cin, Cout of the conv)
 *        3 = persistent full-resolution conv without (the input gradient: Cin = the layer's Cout, Cout = the layer's Cin)
 * One-shot.  mi3d_time_hook_fired() returns 1 when the armed launch happened and disarms the hook either way (call it before
 * reading the events: events that were never recorded cannot be waited for); NULL events disarm.
 * mi3d_event_elapsed_ms synchronises on `stop`. */
/* mi3d_debug_occupy_cus: a stand-in for a resident collective kernel (RCCL all-reduce) on a 1-GPU box: `workgroups` x 512
 * threads x 128 VGPRs hold their CU slots for `microseconds` on `stream` and read through buf[0..n) meanwhile
 * (bench.py --emulate-comm: what a collective beside the encoder backward costs the persistent grids). */
int mi3d_debug_occupy_cus(int workgroups, int microseconds, float* buf, int64_t n, void* stream);
int mi3d_timing_event_create(void** event_out);
int mi3d_time_next_conv3_kernel(void* start_event, void* stop_event, int kind, int Cin, int Cout);
int mi3d_time_hook_fired(void);
int mi3d_event_elapsed_ms(void* start_event, void* stop_event, float* ms_out);
/* params-table index ranges whose gradients segment `seg` produces: ranges = {first0, last0, first1, last1}
 * (half-open; the second range is the segment's upconv for decoder segments, otherwise {-1,-1}) */
int mi3d_unet_segment_params(const mi3d_unet_desc* d, int seg, int* ranges);

/* ------------------------------------------------------------------------------------------------------------
 * Losses and metrics.  Replace utils/metrics.py:14-40 (combined_loss), :137-156 (tversky_loss), :158-167
 * (combined_ce_tversky_loss), :169-190 (distillation_loss), train_unet.py:186-198 ('dice' variant) and
 * utils/metrics.py:65-129 (calculate_iou / calculate_dice / calculate_accuracy, incl. its class-loop bound).
 *   loss = w_ce*CE_mean + w_reg*mean_{c>=1} region_c + w_kd*T^2*mean_{n,c,v} KL(teacher||student)
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct mi3d_loss_cfg {
    float w_ce;
    int32_t region_kind;        /* 0 none, 1 soft Dice (eps 1e-5), 2 Tversky(alpha,beta) (eps 1e-6) */
    float w_reg, alpha, beta, eps;
    float w_kd, temperature;    /* distillation: w_ce,w_reg pre-multiplied by alpha_kd; w_kd = 1-alpha_kd */
} mi3d_loss_cfg;
#define MI3D_LOSS_COEF_FLOATS 20
size_t mi3d_seg_loss_workspace_bytes(int C);
/* logits/teacher (N,C,V) float, labels (N,V) int64; loss_out: device float[1]; coef: device float[20] kept for bwd */
int mi3d_seg_loss_forward(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int64_t V,
                          const mi3d_loss_cfg* cfg, float* loss_out, float* coef, void* workspace, void* stream);
/* grad_out: device float[1] upstream gradient (NULL = 1) */
int mi3d_seg_loss_backward(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int64_t V,
                           const mi3d_loss_cfg* cfg, const float* coef, const float* grad_out, float* dlogits,
                           void* stream);
/* The training step needs the loss AND the metrics of the same logits (train_unet.py:224-232): one pass over
 * logits + labels for both.  metrics_out as mi3d_seg_metrics (device float[3]), workspaces as the two calls. */
int mi3d_seg_loss_metrics_forward(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int D,
                                  int64_t V, const mi3d_loss_cfg* cfg, float* loss_out, float* coef, float* metrics_out,
                                  void* loss_workspace, void* metrics_workspace, void* stream);
/* The training step (train_unet.py:224-232, train_dann.py:268-281, distill_unet.py:107-115) uses the logits only inside the loss,
 * so the 1x1x1 head (models/unet.py:62,87) and the loss can be one pass each way and neither logits nor dlogits ever reach memory:
 *   mi3d_unet_forward_loss      = mi3d_unet_forward + mi3d_seg_loss_metrics_forward   (logits_opt: NULL, or where to keep them)
 *   mi3d_unet_head_loss_forward = the head + loss part alone, on the decoder output that mi3d_unet_forward / mi3d_unet_infer called
 *                                 with logits = NULL left in the workspace (distillation: the teacher's forward runs on another
 *                                 stream and is joined in between; evaluation: infer, then this)
 *   mi3d_unet_backward_loss     = mi3d_seg_loss_backward + mi3d_unet_backward         (grad_scale: device float[1] or NULL = 1)
 * teacher_logits: (N,C,V) float, required iff cfg->w_kd != 0 (distillation_loss, utils/metrics.py:169-190), else NULL.
 * Every logit has the bits of the unfused head; the forward sums add the voxels in another order (loss equal to a few ulp,
 * the integer counts behind the metrics exactly), the backward is bit-identical to the unfused pair given the same `coef`.
 * mi3d_unet_head_loss_supported: 1 if the configuration has the fused kernels (bf16 activations, features[0] == 16,
 * <= 4 classes), else 0 and the calls fail with MI3D_EINVAL. */
int mi3d_unet_head_loss_supported(const mi3d_unet_desc* d, const mi3d_loss_cfg* cfg);
/* The two fused passes as operators (z: the decoder output, channels-last bf16 (N,V,zcs); w (C,Cin), bias (C) float;
 * workspace of mi3d_head_loss_backward: mi3d_conv1_workspace_bytes(Cin, C)). */
int mi3d_head_loss_supported(int dtype, int Cin, int C, const mi3d_loss_cfg* cfg);
int mi3d_head_loss_forward(const void* z, int zcs, int Cin, const float* w, const float* bias, const int64_t* labels,
                           const float* teacher, int N, int C, int D, int64_t V, const mi3d_loss_cfg* cfg, float* loss_out, float* coef,
                           float* metrics_out, void* loss_workspace, void* metrics_workspace, float* logits_opt, void* stream);
int mi3d_head_loss_backward(const void* z, int zcs, int Cin, const float* w, const float* bias, const int64_t* labels,
                            const float* teacher, int N, int C, int64_t V, const mi3d_loss_cfg* cfg, const float* coef,
                            const float* grad_scale, void* dz, int dzcs, float* dW, float* db, int accumulate, void* workspace,
                            size_t workspace_bytes, void* stream);
int mi3d_unet_forward_loss(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* buffers,
                           const float* drop_scales, int training, const int64_t* labels, const float* teacher_logits,
                           const mi3d_loss_cfg* cfg, float* loss_out, float* coef, float* metrics_out, void* loss_workspace,
                           void* metrics_workspace, float* logits_opt, float* gap_out, void* workspace, size_t workspace_bytes,
                           void* stream);
int mi3d_unet_head_loss_forward(const mi3d_unet_desc* d, const void* const* params, const int64_t* labels, const float* teacher_logits,
                                const mi3d_loss_cfg* cfg, float* loss_out, float* coef, float* metrics_out, void* loss_workspace,
                                void* metrics_workspace, float* logits_opt, void* workspace, size_t workspace_bytes, void* stream);
int mi3d_unet_backward_loss(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* grads,
                            const float* drop_scales, const int64_t* labels, const float* teacher_logits, const mi3d_loss_cfg* cfg,
                            const float* coef, const float* grad_scale, const float* dgap, float gap_scale, int accumulate, int seg_begin,
                            int seg_end, void* workspace, size_t workspace_bytes, void* stream, void* aux_stream, void* const* events,
                            int aux_join);
/* Ignore value: the loss of partly labelled volumes (torch's ignore_index; self-training on pseudo-labels, partial annotations,
 * padded or warped-in voxels).  Every loss entry above has a `_masked` sibling that takes `int64_t ignore_index` right after
 * `cfg` and is otherwise the same call; the entry without it is the sibling with no voxel ignored and launches the kernels it
 * always launched (same bits).  With m_v = [t_v != ignore_index] over all N*V voxels (any value that fits int32, inside [0, C)
 * or outside; a value beyond int32 is MI3D_EINVAL) and M_valid = sum_v m_v:
 *   forward   CE_mean = sum_v m_v (lse_v - z_v[t_v]) / M_valid, and 0 when M_valid = 0 (a deviation: torch gives NaN there);
 *             I_c = sum_v m_v p_c [t = c], P_c = sum_v m_v p_c, T_c = sum_v m_v [t = c]; region terms, A_c and B_c as above on
 *             those sums.  The distillation term needs no label: it stays over ALL voxels and its divisor stays N*V*C, so a
 *             teacher still teaches where nothing is labelled.
 *   coef      the same 20 floats; ce_s = w_ce / M_valid (0 when M_valid = 0), kd_s unchanged.
 *   backward  a voxel that counts: the unmasked expression.  An ignored voxel: what that expression gives with
 *             A = B = ce_s = 0, i.e. grad_out * kd[c]; without a teacher a zero (of either sign).
 *   metrics   n_inter, n_pred, n_label, n_correct leave the ignored voxels out; accuracy = n_correct / M_valid (0 when
 *             M_valid = 0); the class-loop bound D stays.
 * M_valid is not counted separately: it is sum_c T_c, the exact integer label histogram over [0, C) that the forward already
 * takes from wave ballots (and sum_c n_label[c] for the accuracy), so a label that is neither in [0, C) nor ignore_index is
 * outside the contract, as it is for the unmasked entries.  No float atomics, fixed-order partial rows: the same bits on
 * every run.  Selecting a term away adds no rounding, so with no voxel ignored every output has the unmasked entry's bits.
 * mi3d_*_supported answer for the masked entries too. */
int mi3d_seg_loss_forward_masked(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int64_t V,
                                 const mi3d_loss_cfg* cfg, int64_t ignore_index, float* loss_out, float* coef, void* workspace,
                                 void* stream);
int mi3d_seg_loss_backward_masked(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int64_t V,
                                  const mi3d_loss_cfg* cfg, int64_t ignore_index, const float* coef, const float* grad_out,
                                  float* dlogits, void* stream);
int mi3d_seg_loss_metrics_forward_masked(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int D,
                                         int64_t V, const mi3d_loss_cfg* cfg, int64_t ignore_index, float* loss_out, float* coef,
                                         float* metrics_out, void* loss_workspace, void* metrics_workspace, void* stream);
int mi3d_head_loss_forward_masked(const void* z, int zcs, int Cin, const float* w, const float* bias, const int64_t* labels,
                                  const float* teacher, int N, int C, int D, int64_t V, const mi3d_loss_cfg* cfg, int64_t ignore_index,
                                  float* loss_out, float* coef, float* metrics_out, void* loss_workspace, void* metrics_workspace,
                                  float* logits_opt, void* stream);
int mi3d_head_loss_backward_masked(const void* z, int zcs, int Cin, const float* w, const float* bias, const int64_t* labels,
                                   const float* teacher, int N, int C, int64_t V, const mi3d_loss_cfg* cfg, int64_t ignore_index,
                                   const float* coef, const float* grad_scale, void* dz, int dzcs, float* dW, float* db, int accumulate,
                                   void* workspace, size_t workspace_bytes, void* stream);
int mi3d_unet_forward_loss_masked(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* buffers,
                                  const float* drop_scales, int training, const int64_t* labels, const float* teacher_logits,
                                  const mi3d_loss_cfg* cfg, int64_t ignore_index, float* loss_out, float* coef, float* metrics_out,
                                  void* loss_workspace, void* metrics_workspace, float* logits_opt, float* gap_out, void* workspace,
                                  size_t workspace_bytes, void* stream);
int mi3d_unet_head_loss_forward_masked(const mi3d_unet_desc* d, const void* const* params, const int64_t* labels,
                                       const float* teacher_logits, const mi3d_loss_cfg* cfg, int64_t ignore_index, float* loss_out,
                                       float* coef, float* metrics_out, void* loss_workspace, void* metrics_workspace, float* logits_opt,
                                       void* workspace, size_t workspace_bytes, void* stream);
int mi3d_unet_backward_loss_masked(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* grads,
                                   const float* drop_scales, const int64_t* labels, const float* teacher_logits,
                                   const mi3d_loss_cfg* cfg, int64_t ignore_index, const float* coef, const float* grad_scale,
                                   const float* dgap, float gap_scale, int accumulate, int seg_begin, int seg_end, void* workspace,
                                   size_t workspace_bytes, void* stream, void* aux_stream, void* const* events, int aux_join);
/* Pseudo-labels for self-training: from the uint8 label map and the float32 confidence map (both (N, V)) that the ensemble and
 * sliding-window predictions return,
 *     target[n][v] = (label < C and conf >= thresholds[label]) ? label : ignore_index          int64, what the masked loss takes
 * A NaN confidence compares false and is ignored, and so is a label >= C.  thresholds: C <= 8 host floats, one per class.
 * table: device int64 (N, C + 1), per sample the voxels kept per class and, last, the voxels ignored (integer adds only: exact,
 * the same on every run).  One streaming pass, 13 bytes per voxel; groups of four voxels with 16-byte accesses where V % 4 == 0,
 * labels is 4-byte and confidence and target are 16-byte aligned, one voxel at a time otherwise.  Nothing synchronises. */
int mi3d_pseudo_labels(const uint8_t* labels, const float* confidence, int N, int64_t V, int C, const float* thresholds,
                       int64_t ignore_index, int64_t* target, int64_t* table, void* stream);
/* The boundary loss of Kervadec et al. (MIDL 2019): a surface term beside the overlap losses above.  logits (N, C, V) float32,
 * C <= 8; phi (N, K, V) float32, the signed distance maps of the target (mi3d_signed_distance_maps); channels: a HOST array of K
 * distinct logit channels in [0, C), map k belongs to channel channels[k].  labels (N, V) int64 and ignore_index (a HOST int64,
 * read before the call returns): both, or both NULL = every voxel counts.  weight: a host float.  grad_scale: device float[1] or
 * NULL = 1 (the pointer the other backward calls take).  loss_out: device float[1].  dlogits (N, C, V) float32, or NULL for the
 * value alone.  flags: MI3D_BD_ADD_LOSS adds to *loss_out instead of storing, MI3D_BD_ADD_GRAD adds into dlogits instead of storing.
 *   p = softmax over the C logits of a voxel
 *   t(x) = sum_{k<K} p[channels[k]] phi[k]                                   0 at an ignored voxel
 *   L    = sum_n sum_x t(x) / (N K V)                                        *loss_out (+)= weight L
 *   dlogits[j](x) (+)= grad_scale weight p_j (phi~_j - t(x)) / (N K V)       phi~_j = phi[k] if j = channels[k], else 0
 *                      0, or untouched (bit for bit) under MI3D_BD_ADD_GRAD, at an ignored voxel
 * The divisor is N K V WHETHER OR NOT voxels are ignored: an ignored voxel contributes nothing and the mean stays over the volume.
 * This is deliberate and unlike the masked CE above, which divides by the voxels that count: the gradient of a voxel then needs
 * no global count, so value and gradient leave one pass over the logits, which can run behind the loss kernels without touching
 * them.  The sum is taken in double from the per-voxel float32 terms through fixed slots added in a fixed order by a second tiny
 * launch: no float atomics, the same bits on every run.  16-byte accesses, four voxels per thread, where V % 4 == 0 and logits, phi,
 * dlogits and labels are 16-byte aligned; one voxel at a time otherwise.  Every argument is checked before the first launch; nothing
 * allocates or synchronises.  workspace: mi3d_boundary_loss_workspace_bytes(N, V) bytes, 8-byte aligned. */
#define MI3D_BD_ADD_LOSS 1
#define MI3D_BD_ADD_GRAD 2
size_t mi3d_boundary_loss_workspace_bytes(int N, int64_t V);
int mi3d_boundary_loss(const float* logits, const float* phi, int N, int C, int K, int64_t V, const int32_t* channels, const int64_t* labels,
                       const int64_t* ignore_index, float weight, const float* grad_scale, float* loss_out, float* dlogits, int flags,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Entropy minimisation (MinEnt of ADVENT, Vu et al., CVPR 2019): the unsupervised term that makes the network confident where nothing
 * is labelled.  logits (N, C, V) float32, 2 <= C <= 8 (C = 1 has ln C = 0 and is refused).  mode selects the voxels:
 *   MI3D_ENT_ALL      every voxel; labels and ignore_index may be NULL (given, they are not read)
 *   MI3D_ENT_COUNTED  the voxels with labels != ignore_index         MI3D_ENT_IGNORED  the voxels with labels == ignore_index
 * labels (N, V) int64 and ignore_index (a HOST int64, read before the call returns): both or neither; both label modes require them.
 * weight: a host float.  grad_scale: device float[1] or NULL = 1.  loss_out: device float[1].  dlogits (N, C, V) float32, or NULL for
 * the value alone.  flags: MI3D_ENT_ADD_LOSS adds to *loss_out instead of storing, MI3D_ENT_ADD_GRAD adds into dlogits instead of
 * storing (what the MI3D_BD_* pair means).  Per voxel, in the log-sum-exp form, which never forms p log p (a saturated voxel gives
 * exactly 0 and no NaN):
 *   d_j = z_j - max_j z_j,  e_j = exp(d_j),  se = sum_j e_j,  p_j = e_j / se,  H = log(se) - sum_j p_j d_j
 *   *loss_out (+)= weight sum_{selected voxels} H / (N V ln C)                                in [0, weight], as in ADVENT
 *   dlogits[k](x) (+)= grad_scale weight p_k (log(se) - d_k - H) / (N V ln C)                 at a selected voxel
 *                      0, or untouched (bit for bit) under MI3D_ENT_ADD_GRAD, at an unselected voxel
 * The divisor is N V ln C WHATEVER is selected, for the boundary term's reason: the gradient of a voxel then needs nothing but the
 * voxel (no global count), so value and gradient leave ONE pass over the logits.  The sum is float32 per voxel and double from the
 * thread's accumulator on, through fixed slots added in a fixed order by a second tiny launch: no float atomics, the same bits on
 * every run.  16-byte accesses, four voxels per thread, where V % 4 == 0 and logits, dlogits and the labels that are read are 16-byte
 * aligned; one voxel at a time otherwise.  Every argument is checked before the first launch; nothing allocates or synchronises.
 * workspace: mi3d_entropy_loss_workspace_bytes(N, V) bytes, 8-byte aligned. */
#define MI3D_ENT_ALL 0
#define MI3D_ENT_COUNTED 1
#define MI3D_ENT_IGNORED 2
#define MI3D_ENT_ADD_LOSS 1
#define MI3D_ENT_ADD_GRAD 2
size_t mi3d_entropy_loss_workspace_bytes(int N, int64_t V);
int mi3d_entropy_loss(const float* logits, int N, int C, int64_t V, const int64_t* labels, const int64_t* ignore_index, int mode,
                      float weight, const float* grad_scale, float* loss_out, float* dlogits, int flags,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t mi3d_seg_metrics_workspace_bytes(int C);
/* out: device float[3] = {iou, dice, accuracy}; D = first spatial dim (reference loop bound, metrics.py:74,101) */
int mi3d_seg_metrics(const float* logits, const int64_t* labels, int N, int C, int D, int64_t V, float* out,
                     void* workspace, void* stream);
/* Evaluation.  Replaces the per-class mask/sum loops of test_model.py:255-276: exact counts of
 * pred = argmax(logits) against labels in one pass.  counts: device int64[3*C + 1] =
 * { n_inter[C] (pred==c && label==c), n_pred[C], n_label[C], n_correct };  same workspace as mi3d_seg_metrics. */
int mi3d_seg_class_counts(const float* logits, const int64_t* labels, int N, int C, int64_t V, int64_t* counts,
                          void* workspace, void* stream);
/* Segmenting with a trained model (test_model.py:242-285: model(x), torch.argmax(outputs, dim=1), the per-sample per-class
 * counts, pred_classes.cpu()): the 1x1x1 head, the argmax and the counts in ONE pass over the decoder output, so the logits are
 * never written.  z, zcs, Cin, w, bias: the operands of mi3d_conv1_forward (channels-last `dtype` [N][V] rows of stride zcs, any
 * Cin; w (Cout,Cin), bias (Cout) float, bias may be NULL); Cout <= 8; any V >= 1, tails are handled in the kernel.
 *   labels_out  uint8 (N,V): the first maximum, under a strict `>` scan from class 0, of the logits mi3d_conv1_forward gives for the
 *               same dtype, bit for bit (both take them from one device function).  Finite logits are the contract; NaN behaves as
 *               in mi3d_seg_class_counts: a NaN never wins a comparison, so a NaN logit is chosen only where it is logit 0.
 *   target      int64 (N,V), or NULL.  With it, counts: device int64 (N, 3*Cout + 1), per SAMPLE { n_inter[Cout], n_pred[Cout],
 *               n_label[Cout], n_correct } in the order of mi3d_seg_class_counts; exact integers, no atomics.  A target value
 *               outside [0, Cout) counts nowhere; it is compared as int64, whereas mi3d_seg_class_counts narrows the label to
 *               32 bits first (2^32 + 1 counts as class 1 there, nowhere here), so the sum over the samples equals
 *               mi3d_seg_class_counts' row for targets inside the int32 range.  Both NULL or both given.
 *   workspace   mi3d_head_labels_workspace_bytes(N, Cout) bytes, 8-byte aligned; read only with a target (else may be NULL).
 * mi3d_unet_head_labels runs it on the decoder output that the last mi3d_unet_infer / mi3d_unet_forward called with logits = NULL
 * left in `workspace` (the sibling of mi3d_unet_head_loss_forward); labels_out (N,D,H,W), head_workspace as above. */
size_t mi3d_head_labels_workspace_bytes(int N, int Cout);
int mi3d_head_labels(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, int Cout, int N, int64_t V,
                     uint8_t* labels_out, const int64_t* target, int64_t* counts, void* workspace, void* stream);
int mi3d_unet_head_labels(const mi3d_unet_desc* d, const void* const* params, const int64_t* target, uint8_t* labels_out,
                          int64_t* counts, void* head_workspace, void* workspace, size_t workspace_bytes, void* stream);
/* Flip and model ensembles (test-time mirroring over the axes random_flip trains with, utils/dataloader.py:207-213, and the same
 * average over several checkpoints): ONE VIEW per call, the 1x1x1 head, its softmax and the add into a vote volume in one pass
 * over the decoder output, so the logits and the probabilities of a view are never written.  A view is (a model, a flip code):
 * bit 0 of `flip` mirrors W, bit 1 H, bit 2 D.  z is the decoder output of model(torch.flip(x, those dims)); operands as for
 * mi3d_head_labels, the volume given as D, H, W (D * H * W < 2^31).  For view = 0 .. views - 1, in that order:
 *     p      = softmax over the classes, in float32, of the logits mi3d_conv1_forward gives (bit for bit), flipped back
 *     votes  float (N,Cout,D,H,W): view 0 stores p (the volume needs no clearing), a later view adds p: float32 adds in view order
 *     last view: the total stays in registers; labels_out uint8 (N,D,H,W) = its first maximum (strict `>` scan from class 0);
 *            confidence float (N,D,H,W), optional = total[label] / (float)views (IEEE division); target / counts / workspace
 *            as for mi3d_head_labels (workspace: mi3d_head_votes_workspace_bytes(N, Cout)); the total is written to `votes`
 *            only with MI3D_VOTES_KEEP in `flags`.
 * views = 1 is first and last at once; `votes` may then be NULL unless it is kept.  labels_out, confidence, target and counts
 * must be NULL on every view but the last.  One thread owns a voxel and nothing is atomic: the same inputs give the same bits.
 * Every argument is checked before anything is launched.  mi3d_unet_head_votes runs a view on the decoder output that the
 * last mi3d_unet_infer with logits = NULL left in `workspace` (the sibling of mi3d_unet_head_labels). */
#define MI3D_VOTES_KEEP 1
size_t mi3d_head_votes_workspace_bytes(int N, int Cout);
int mi3d_head_votes(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, int Cout, int N, int D, int H,
                    int W, int flip, int view, int views, int flags, float* votes, uint8_t* labels_out, float* confidence,
                    const int64_t* target, int64_t* counts, void* workspace, void* stream);
int mi3d_unet_head_votes(const mi3d_unet_desc* d, const void* const* params, int flip, int view, int views, int flags, float* votes,
                         uint8_t* labels_out, float* confidence, const int64_t* target, int64_t* counts, void* head_workspace,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Sliding-window inference (the network sees windows of the size it was trained on; overlapping predictions are blended with an
 * importance map): the vote pass of mi3d_head_votes for N WINDOW samples of sides d x h x w, each added, weighted, into a sub-box of
 * ONE accumulator acc float (Cout,D,H,W), contiguous, D * H * W < 2^31.  Operands z, zcs, Cin, w, bias, Cout, dtype as for
 * mi3d_head_votes (z holds the N samples one after another).  Host arrays, read at call time: flips (N codes; bit 0 mirrors W,
 * bit 1 H, bit 2 D, WITHIN the window) and origins (N x 3 ints {od, oh, ow}).  Device float tables g_d (d), g_h (h), g_w (w).
 * For sample n = 0 .. N - 1 in that order, for every window voxel x = (xd, xh, xw):
 *     p        = softmax over the classes, in float32, of the logits mi3d_conv1_forward gives (bit for bit), flipped back
 *     weight   = (g_d[xd] * g_h[xh]) * g_w[xw]                      float32, each product rounded on its own
 *     acc[c][o + x] = acc[c][o + x] + weight * p[c]                 the product rounded, then the sum: never contracted
 * The samples of a call may overlap in acc; the result is that of one call per sample in sample order (one launch per sample on
 * the stream).  One thread owns a voxel and nothing is atomic: the same inputs give the same bits.  The caller clears acc
 * (0 + x is exact).  16-byte plane accesses are taken where W, w and the origin's ow are multiples of 4, the one-voxel route
 * elsewhere; both give the same bits.  Every argument is checked before anything is launched (every origin + window inside the
 * volume, Cout <= 8, non-NULL tables, D * H * W < 2^31, flip codes in [0, 8)): a bad call leaves acc untouched.
 * mi3d_unet_head_votes_window runs it on the decoder output that the last mi3d_unet_infer with logits = NULL left in `workspace`:
 * N and the window are the descriptor's.
 *
 * mi3d_votes_finish turns the weighted totals into the outputs of mi3d_head_votes' last view.  n_d (D), n_h (H), n_w (W): device
 * float tables, n_axis[i] = the float32 rounding of the float64 sum of that axis's importance-table entries over the windows that
 * cover index i (the windows form a tensor grid, so the weight sum of a voxel factorises).  Per voxel (xd, xh, xw):
 *     labels_out uint8 (D,H,W) = the first maximum of acc over the classes (strict `>` scan from class 0)
 *     norm       = ((n_d[xd] * n_h[xh]) * n_w[xw]) * (float)views_per_window        float32, each product rounded on its own
 *     confidence float (D,H,W), optional = acc[label] / norm                        IEEE division
 *     with MI3D_VOTES_NORMALIZE in `flags`: acc[c] = acc[c] / norm in place, the mean probabilities (IEEE division)
 *     target int64 (D*H*W) / counts int64 (3*Cout + 1) / workspace (mi3d_head_votes_workspace_bytes(1, Cout)) as for mi3d_head_votes
 * Every argument is checked before anything is launched. */
#define MI3D_VOTES_NORMALIZE 1
int mi3d_head_votes_window(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, int Cout, int N, int d, int h,
                           int wd, const int* flips, const float* g_d, const float* g_h, const float* g_w, const int* origins, float* acc,
                           int D, int H, int W, void* stream);
int mi3d_unet_head_votes_window(const mi3d_unet_desc* d, const void* const* params, const int* flips, const float* g_d, const float* g_h,
                                const float* g_w, const int* origins, float* acc, int D, int H, int W, void* workspace,
                                size_t workspace_bytes, void* stream);
int mi3d_votes_finish(float* acc, int Cout, int D, int H, int W, const float* n_d, const float* n_h, const float* n_w,
                      int views_per_window, int flags, uint8_t* labels_out, float* confidence, const int64_t* target, int64_t* counts,
                      void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * DANN head.  Replaces train_dann.py:34-49 (DomainDiscriminator MLP 256-256-128-64-2, ReLU, Dropout 0.2) and
 * :283 (nn.CrossEntropyLoss on the concatenated domain predictions).  GradientReversal (:22-32) is the
 * gap_scale argument of mi3d_unet_backward plus gx_scale here.
 * ---------------------------------------------------------------------------------------------------------- */
int mi3d_linear_forward(const float* x, const float* w, const float* b, float* y, int M, int K, int Nout, int relu,
                        const float* drop, void* stream);
/* y = the forward's output (ReLU mask); gx = gx_scale * dL/dx (gx_scale = -lambda folds the gradient reversal);
 * workspace: M*Nout floats */
int mi3d_linear_backward(const float* x, const float* w, const float* y, const float* gy, int M, int K, int Nout,
                         int relu, const float* drop, float* gx, float* gw, float* gb, int accumulate,
                         float gx_scale, float* workspace, void* stream);
/* y = alpha * (alpha_dev ? *alpha_dev : 1) * x over n floats.  GradientReversal.backward (train_dann.py:27-29:
 * grad_output.neg() * lambda_) is alpha = -lambda; the row-CE backward multiplies by the upstream gradient alpha_dev. */
int mi3d_scale(const float* x, float* y, int64_t n, float alpha, const float* alpha_dev, void* stream);
/* mean CE over M rows; dlogits = scale * d(loss)/d(logits) (may be NULL) */
int mi3d_softmax_ce_rows(const float* logits, const int64_t* labels, int M, int C, float* loss, float* dlogits,
                         float scale, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Optimizer and RNG helpers on the step path.
 * mi3d_adamw_step replaces torch.optim.AdamW(...).step() (train_unet.py:378,226) over one flat fp32 arena.
 * step_dev: device int64 holding the number of steps taken so far (incremented by the call).
 * ---------------------------------------------------------------------------------------------------------- */
int mi3d_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, float grad_scale, int64_t* step_dev, void* stream);
/* Same update over ONE contiguous range of the arena without (increment = 0) or with the step increment: a step over
 * several trainable ranges (frozen encoder, train_unet.py:31-43,413-431) = one call per range, increment on the last;
 * n = 0 with increment = 1 only advances the counter. */
int mi3d_adamw_apply(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, float grad_scale, int64_t* step_dev, int increment, void* stream);
/* Dropout3d (unet.py:14,18) channel masks: out[i] = 0 w.p. p else 1/(1-p); state_dev = device uint64[2]
 * {seed, counter}, counter advanced by n.  Counter-based RNG: same distribution as torch, different stream. */
int mi3d_dropout_scales(float* out, int64_t n, float p, uint64_t* state_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Input pipeline: the per-volume arithmetic of CombinedDataset.__getitem__ (utils/dataloader.py:148-200)
 * on the device.  in/out: device float (n voxels of ONE volume; in == out allowed); labels int64.
 * ---------------------------------------------------------------------------------------------------------- */
/* preprocess_ct, utils/dataloader.py:111-117: clip to [window_min, window_max] (reference: -160, 240), scale to [0,1] */
int mi3d_preprocess_ct(const float* in, float* out, int64_t n, float window_min, float window_max, void* stream);
/* preprocess_mri, utils/dataloader.py:128-144: z-score with the population std (+1e-8), clip to the
 * np.percentile([p_low, p_high]) values (reference: 1, 99; linear interpolation between exact order statistics),
 * (x - low) / (high - low + 1e-8).  workspace: mi3d_preprocess_mri_workspace_bytes(), 16-byte aligned. */
size_t mi3d_preprocess_mri_workspace_bytes(void);
int mi3d_preprocess_mri(const float* in, float* out, int64_t n, float p_low, float p_high, void* workspace, void* stream);
/* label remaps, utils/dataloader.py:162-181.  kind 0: identity (ts / btcv), 1: AMOS {0:0,1:1,2:3,3:3,6:2, else 0},
 * 2: CHAOS ranges {[55,70]:2, [110,135]:3, [175,200]:3, [240,255]:1, else 0} */
int mi3d_remap_labels(const int64_t* in, int64_t* out, int64_t n, int kind, void* stream);

/* Resampling of ONE decoded scan to the training grid: scipy.ndimage.zoom(..., mode='nearest', prefilter=False) as the
 * reference's offline scripts call it (scripts/resampling/amos_ct_resample.py:56-70,93-97; the same four calls in
 * chaos_resample.py:53,63,83,87 and resample_totalseg_ras_mri.py:57,65,92,94).  in: (D, H, W), out: (Do, Ho, Wo), both
 * contiguous, in != out.  The per-axis tables are built by the caller on the host in float64 (resample.py axis_table)
 * and passed as device pointers, one row per OUTPUT index of the axis; rows_* must equal the output sides. */
/* bytes of the float (D, H, W) stage-1 volume of a two-stage chain (amos_ct_resample.py:60 -> :70), rounded up to 256 */
size_t mi3d_zoom3_workspace_bytes(int D, int H, int W);
/* order=3 (amos_ct_resample.py:60,70).  Table row, 48 bytes, tables 16-byte aligned:
 *   { int32_t idx[4]; double w[4]; }   input indices of the taps floor(c)-1 .. floor(c)+2, each clamped to [0, n_in-1]
 *                                      (mode='nearest'), and their cubic B-spline weights (no prefilter).
 * out = float32(sum over the 4x4x4 taps of in * w_d * w_h * w_w), summed in float64.  ct_window != 0 also applies
 * mi3d_preprocess_ct(window_min, window_max) to the rounded value (the step the script leaves commented out at :74). */
int mi3d_zoom3_cubic(const float* in, float* out, int D, int H, int W, int Do, int Ho, int Wo, const void* table_d, int rows_d,
                     const void* table_h, int rows_h, const void* table_w, int rows_w, int ct_window, float window_min,
                     float window_max, void* stream);
/* order=0 (amos_ct_resample.py:93,97): out[d][h][w] = in[index_d[d]][index_h[h]][index_w[w]].  Two order-0 zooms compose
 * into one call with index = index1[index2] per axis, so the intermediate label volume need not exist. */
int mi3d_zoom3_nearest_i64(const int64_t* in, int64_t* out, int D, int H, int W, int Do, int Ho, int Wo, const int32_t* index_d,
                           int rows_d, const int32_t* index_h, int rows_h, const int32_t* index_w, int rows_w, void* stream);

/* The same scan AS STORED: what the scripts do before the first zoom (reorient_to_ras, amos_ct_resample.py:29-36 = io_orientation
 * -> ornt_transform -> apply_orientation, a host flip + transpose of the whole volume) folded into the reads.  The source is any
 * dense 3-D array (a permutation of a contiguous one) of the dtype below; D, H, W are its sides in RAS order and stride_d/h/w the
 * element strides of those axes in the stored array (orientation.py axis_map).  Nothing is copied on the host.  The entry points
 * check that the strides are positive; that (D - 1) * stride_d + (H - 1) * stride_h + (W - 1) * stride_w lies inside the buffer is the
 * caller's guarantee (resample.py admits dense tensors only, orientation.check_dense). */
enum { MI3D_SRC_U8 = 0, MI3D_SRC_I16 = 1, MI3D_SRC_F32 = 2, MI3D_SRC_I64 = 3 };
/* apply_orientation (amos_ct_resample.py:33): out (D, H, W) contiguous, float32 (out_i64 = 0; from uint8, int16, float32: the
 * .astype(np.float32) of :47) or int64 (out_i64 = 1; from uint8, int16, int64), out[d][h][w] = in[d' * stride_d + h' * stride_h +
 * w' * stride_w] with i' = n - 1 - i on the axes whose flip_mask bit is set (1: D, 2: H, 4: W).  A stored-fastest W is a streamed
 * copy with 16-byte stores; a stored-fastest D or H goes through 32 x 32 LDS tiles, read and written coalesced. */
int mi3d_reorient3(const void* in, int src_dtype, void* out, int out_i64, int D, int H, int W, int64_t stride_d, int64_t stride_h,
                   int64_t stride_w, int flip_mask, void* stream);
/* mi3d_zoom3_cubic of the reoriented scan without making it (amos_ct_resample.py:33 + :60).  Tables as there, built in RAS order;
 * for a flipped axis the caller replaces every tap index i by n - 1 - i AFTER the clamp (weights unchanged).  Same taps, same
 * float64 sums in the same order: bit-identical to mi3d_zoom3_cubic on mi3d_reorient3's float32 output.  Source: uint8, int16 or
 * float32.  A float32 source with the strides of a contiguous (D, H, W) volume runs the kernel mi3d_zoom3_cubic runs; likewise an
 * int64 source of mi3d_zoom3_nearest_src and mi3d_zoom3_nearest_i64. */
int mi3d_zoom3_cubic_src(const void* in, int src_dtype, int64_t stride_d, int64_t stride_h, int64_t stride_w, float* out, int D,
                         int H, int W, int Do, int Ho, int Wo, const void* table_d, int rows_d, const void* table_h, int rows_h,
                         const void* table_w, int rows_w, int ct_window, float window_min, float window_max, void* stream);
/* mi3d_zoom3_nearest_i64 of the reoriented label (chaos_resample.py:40-44 + :83,87; amos_ct_resample.py:93,97), index tables
 * remapped for flips in the same way.  Source: uint8, int16 or int64; out: int64. */
int mi3d_zoom3_nearest_src(const void* in, int src_dtype, int64_t stride_d, int64_t stride_h, int64_t stride_w, int64_t* out, int D,
                           int H, int W, int Do, int Ho, int Wo, const int32_t* index_d, int rows_d, const int32_t* index_h,
                           int rows_h, const int32_t* index_w, int rows_w, void* stream);
/* The TotalSegmentator mask merge (resample_totalseg_ras_mri.py:77-96: per organ reorient, two order-0 zooms,
 * label_combined[label_resized > 0] = value) as ONE gather: out = 0, then for k = 0 .. n-1: if (mask_k[source voxel] > 0) out =
 * value_k, so later entries win as in the script's loop; n = 0 gives zeros (the script's "file not found" branch for every organ).
 * All masks share the shape, the strides, the dtype (uint8 or float32) and the composed index tables. */
#define MI3D_MAX_MASKS 8
typedef struct {
    const void* mask[MI3D_MAX_MASKS];
    int64_t value[MI3D_MAX_MASKS];
    int32_t n;
} mi3d_mask_list;
int mi3d_merge_masks3(const mi3d_mask_list* masks, int src_dtype, int64_t stride_d, int64_t stride_h, int64_t stride_w, int64_t* out,
                      int D, int H, int W, int Do, int Ho, int Wo, const int32_t* index_d, int rows_d, const int32_t* index_h,
                      int rows_h, const int32_t* index_w, int rows_w, void* stream);
/* The way back: a uint8 label map on the training grid (Dg, Hg, Wg, contiguous) put onto the scan as stored.  The reference has no
 * inverse, so it is defined here: RAS label = scipy.ndimage.zoom(grid, ras_shape / grid_shape, order=0, mode='nearest',
 * prefilter=False), ONE zoom (the intermediate shape of the inbound chain carries no information for an order-0 gather), then the
 * inverse of reorient_to_ras.  out is the stored uint8 tensor seen in RAS order: sides D, H, W and element strides as for
 * mi3d_zoom3_nearest_src's source, here on the destination; index_* hold one grid index per RAS index of the axis (resample.py
 * axis_table(n_grid, n, 0), D / H / W entries), built in RAS order and, for a flipped axis, read backwards: entry i is the table's
 * entry n - 1 - i.  out[d*stride_d + h*stride_h + w*stride_w] = grid[index_d[d]][index_h[h]][index_w[w]].  The output is written
 * in the stored tensor's memory order for every orientation, 16 bytes per store where the row is aligned.  grid != out. */
int mi3d_restore_labels3(const uint8_t* grid, int Dg, int Hg, int Wg, uint8_t* out, int D, int H, int W, int64_t stride_d,
                         int64_t stride_h, int64_t stride_w, const int32_t* index_d, const int32_t* index_h, const int32_t* index_w,
                         void* stream);
/* The soft way back: the float32 vote volume (C, Dg, Hg, Wg, contiguous; mi3d_head_votes with MI3D_VOTES_KEEP) zoomed linearly onto
 * the scan as stored and the argmax taken THERE, in one gather: scipy.ndimage.zoom(votes[k], ras_shape / grid_shape, order=1,
 * mode='nearest', prefilter=False) per class, restated so that the bits are fixed.  Per axis, for RAS index i of n onto a grid of
 * n_grid: z = (n_grid - 1) / (n - 1) (1.0 for n = 1), c = i * z in float64, f = floor(c), t = c - f; table row, 24 bytes:
 *   { int32_t idx[2]; double w[2]; }   taps clip(f, 0, n_grid - 1) and clip(f + 1, 0, n_grid - 1); weights 1.0 - t and t
 * (resample.py axis_table(n_grid, n, 1), D / H / W rows; built in RAS order and, for a flipped axis, read backwards as index_* of
 * mi3d_restore_labels3).  The value of class k at (d, h, w) is the nested interpolation, W innermost, then H, then D, in float64,
 * every product and every sum rounded on its own (no fused multiply-add):
 *   r(a, b) = p[k][d_a][h_b][w_0] * ww0 + p[k][d_a][h_b][w_1] * ww1          a, b in {0, 1}
 *   s(a)    = r(a, 0) * wh0 + r(a, 1) * wh1
 *   v_k     = s(0) * wd0 + s(1) * wd1
 * out (uint8) = the first maximum of v_0 .. v_{C-1} (strict `>` scan from class 0, the rule of mi3d_head_votes); confidence (float,
 * may be NULL) = (float)v_label, the one rounding to float32.  Both are the stored tensor seen in RAS order (sides D, H, W, element
 * strides as for mi3d_restore_labels3) and are written in its memory order for every orientation: the lanes of a wave run along the
 * destination axis that is the grid's W, the only contiguous axis of the votes (consecutive bytes per lane where that is the stored-
 * fastest axis, a 16-byte piece of its own row per lane, cut at aligned addresses, where it is not).  The order of operations
 * does not depend on the layout, so a float64 numpy model of the lines above gives the same bits, ties included.  Finite votes are
 * the contract (a NaN never wins a comparison).  C in [2, 8]; sides and strides as for mi3d_restore_labels3; out and confidence
 * must differ from votes and from each other.  Every argument is checked before anything is launched. */
typedef struct {
    int32_t idx[2];
    double w[2];
} mi3d_lerp_row;
int mi3d_restore_votes3(const float* votes, int C, int Dg, int Hg, int Wg, uint8_t* out, float* confidence, int D, int H, int W,
                        int64_t stride_d, int64_t stride_h, int64_t stride_w, const mi3d_lerp_row* rows_d, const mi3d_lerp_row* rows_h,
                        const mi3d_lerp_row* rows_w, void* stream);

/* The preview figure of the reference's test loop (visualize_prediction, test_model.py:66-193, called at :299-305 on whole host
 * copies of the image, the label and the prediction) and the slider of visualize_nifti.py:29-52, computed where the volumes are.
 * Every volume is a dense 3-D array of sides D, H, W (the reference's axes 0, 1, 2) seen through element strides, as the source
 * of mi3d_zoom3_nearest_src: a contiguous training-grid tensor and a scan as stored go through the same code.  Labels are uint8
 * or int64, images float32 or int16 (an int16 voxel counts as the float32 of it).  The image must be finite: the minimum and
 * maximum of a slice with a NaN or an Inf are not defined here.  All entries allocate nothing, do not synchronise and return a
 * negative value for null pointers, sides outside [1, 65535], non-positive strides and unknown dtype / mode codes.
 *
 * mi3d_preview_workspace_bytes: enough for the counts (D + H + W int64), three int32 indices (16 bytes) and 2 keys for every
 * slice of the longest axis; the caller lays the pieces out, ZEROES counts and keys before the calls below, and may hand counts
 * and indices to its user.  0 (and an error) for bad sides. */
size_t mi3d_preview_workspace_bytes(int D, int H, int W);
/* find_best_slice's np.sum(label_volume > 0, axis=...) (test_model.py:77-82) for all three axes in ONE read of the label:
 * counts[i] += #{label > 0 in slice i of axis 0}, counts[D + i] of axis 1, counts[D + H + i] of axis 2; counts zeroed by the
 * caller.  A label >= 4 counts, a negative one does not.  The volume is walked in memory order whichever axis is stored fastest:
 * register columns per lane along it, shuffle sums along the next, then LDS and 64-bit integer atomics; integer sums in any
 * order are the same sum, so the result is exact and the same bits every run.  16-byte loads where the rows are 16-byte aligned
 * and the fastest side is a multiple of 16 (uint8) or 2 (int64); one element per lane otherwise. */
int mi3d_foreground_profiles(const void* label, int label_dtype, int D, int H, int W, int64_t stride_d, int64_t stride_h,
                             int64_t stride_w, int64_t* counts, void* stream);
/* best[a] = np.argmax(counts of axis a), the FIRST maximum, or n_a // 2 where that maximum is 0 (test_model.py:85-89), for
 * a = 0, 1, 2; counts as mi3d_foreground_profiles leaves them.  The indices stay on the device for the two entries below. */
int mi3d_best_slices(const int64_t* counts, int D, int H, int W, int32_t* best, void* stream);
/* Which slices an entry covers.  STACK: every slice of `axis`, slot i = slice i.  ONE: one slice of `axis`, slot 0; its index is
 * read from index[0] on the device when index != NULL, else it is k (checked).  THREE: the slice index[a] of every axis a, slot
 * a (`axis` and k unused).  An index read from device memory is clamped to the axis. */
enum { MI3D_PREVIEW_STACK = 0, MI3D_PREVIEW_ONE = 1, MI3D_PREVIEW_THREE = 2 };
/* overlay.min() and overlay.max() (test_model.py:110) of each covered slice, as two uint32 keys per slot that start from ZERO
 * (the caller's): keys[2 s] = max over the slice of key(v), keys[2 s + 1] = max of ~key(v), with key(v) = bits ^ 0xffffffff for a
 * negative float and bits | 0x80000000 otherwise (the float order as an unsigned order; never 0 for a finite v).  Unsigned
 * atomic maxima: any order gives the same pair.  -0.0 orders below +0.0 here; which of the two numpy returns is not defined. */
int mi3d_slice_minmax(const void* image, int image_dtype, int D, int H, int W, int64_t stride_d, int64_t stride_h, int64_t stride_w,
                      int axis, int mode, const int32_t* index, int k, uint32_t* keys, void* stream);
/* create_overlay (test_model.py:103-125, the same function as visualize_nifti.py:29-52) per output pixel, in IEEE double with
 * every operation rounded on its own: g = ((double)v - min) / (max - min) from the slice's keys, rgb = (g, g, g), replaced by
 * (1, 0, 0) for label 1, (1, 0.65, 0) for label 2, (0, 0.5, 0) for label 3; any other label keeps the grey; a flat slice gives
 * 0 / 0 = NaN wherever no colour replaces it, as numpy does.  The slice of axis 0 / 1 / 2 is the 2-D array over axes (1, 2) /
 * (0, 2) / (0, 1), sides (A, B); rot90 != 0 writes np.rot90 of it, out[i][j] = slice[j][B - 1 - i], (B, A) pixels.
 * out_dtype: F64 the reference's own bits, F32 one rounding of them, U8 (255 * value).astype(np.uint8): truncation, NaN -> 0.
 *   STACK, ONE   outs[0] = (n_axis, R, C, 3) or (R, C, 3); pred must be NULL.  16-byte stores where C is a multiple of 2 (F64),
 *                4 (F32) or 16 (U8) pixels and outs[0] is 16-byte aligned.  A stack whose image is stored fastest along the slice
 *                axis or along R is read with lanes along that axis and turned through LDS tiles; the bits do not depend on it.
 *   THREE        the 3 x 3 figure of test_model.py:127-179 in one launch, rot90 required: outs[3 v + 0 / 1 / 2] = float32 (R, C)
 *                raw slice, overlay of `label`, overlay of `pred`, for v = 0, 1, 2 = axial (axis 2), sagittal (axis 0), coronal
 *                (axis 1).  label and pred may differ in dtype and strides.
 * *_strides: three element strides each, HOST arrays read before the call returns.  outs: a HOST array of device pointers.
 * keys: what mi3d_slice_minmax left for the same axis / mode / index. */
enum { MI3D_OVERLAY_F64 = 0, MI3D_OVERLAY_F32 = 1, MI3D_OVERLAY_U8 = 2 };
int mi3d_overlay_render(const void* image, int image_dtype, const int64_t* image_strides, const void* label, int label_dtype,
                        const int64_t* label_strides, const void* pred, int pred_dtype, const int64_t* pred_strides, int D, int H, int W,
                        int axis, int mode, const int32_t* index, int k, int rot90, const uint32_t* keys, int out_dtype,
                        void* const* outs, void* stream);

/* Connected components of a label map, the largest of them per class, and the cleaned map: what follows a prediction on the host
 * today (scipy.ndimage.label(labels == c, scipy.ndimage.generate_binary_structure(3, connectivity)) per class, np.bincount of the
 * ids, np.isin of the kept ones).  The reference writes its predictions out uncleaned (test_model.py:299-309), so scipy.ndimage.label
 * is the contract.  labels: N samples of sides D, H, W seen through element strides (any dense layout per sample), uint8 or int64.
 *   component   two voxels of one sample with the same SELECTED value (a subset of 1..255; 0, and int64 values outside 0..255, never)
 *               joined by a path of neighbours of that value; connectivity 1, 2, 3 = 6, 18, 26 neighbours.  Components never
 *               cross samples; unselected voxels belong to none.
 *   root        the C-order index d * H * W + h * W + w (logical axes, within the sample) of the component's first voxel: the
 *               labelling is canonical, independent of launch order, tile size and strides.
 *   ranking     within one (sample, class): size descending, then root ascending.
 * Only integer atomics are used: the same bits every run.  Nothing allocates or synchronises.  status_out: one int32 the entry
 * zeroes first; a kernel whose parent-following loop reaches its bound (it cannot, a chain has fewer than D * H * W links) ORs
 * a MI3D_COMPONENTS_STATUS_* bit into it and leaves, so every kernel terminates; the outputs mean nothing unless it is 0.
 * workspace: mi3d_components_workspace_bytes bytes (13 per voxel, rounded up), 256-byte aligned; 0 (and an error) for N outside
 * [1, 65535], a side < 1 or D * H * W >= 2^31. */
#define MI3D_COMPONENTS_TILE 8            /* a workgroup labels a tile of 8 x 8 x 64 voxels (d, h, w) before the tiles are joined */
#define MI3D_COMPONENTS_MAX_CLASSES 8
#define MI3D_COMPONENTS_MAX_KEEP 8
enum { MI3D_COMPONENTS_STATUS_TILE = 1, MI3D_COMPONENTS_STATUS_SEAM = 2, MI3D_COMPONENTS_STATUS_FLATTEN = 4 };
size_t mi3d_components_workspace_bytes(int N, int D, int H, int W);
/* roots_out (N, D, H, W) int32, contiguous: the root of every voxel's component, -1 where the voxel's value is not selected; the
 * np.unique(ids, return_index=True) of scipy's labelling of every selected class, at every voxel.  class_select: a HOST array of
 * 256 bytes read before the call returns, non-zero at the selected values; class_select[0] must be 0. */
int mi3d_component_roots(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d,
                         int64_t stride_h, int64_t stride_w, int connectivity, const uint8_t* class_select, int32_t* roots_out,
                         int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream);
/* labels_out (dtype and strides of labels; may be labels itself): a voxel of listed class j keeps its value iff its component is
 * kept, else it becomes fill (0..255); every other voxel is copied.  A component of class j is kept iff its rank is below
 * keep_k[j] (1..8) and its size is at least min_size (>= 1).  class_values / keep_k: HOST arrays of n_classes (1..8) distinct
 * values in 1..255 and their counts.  stats_out: (N, n_classes, 3 + 2 * 8) int64, one row per listed class:
 *   [0] n_components  [1] voxels_before  [2] voxels_kept  [3..10] sizes of the kept components in rank order, 0 where there are
 *   fewer  [11..18] their roots, -1 where there are fewer. */
int mi3d_keep_components(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d,
                         int64_t stride_h, int64_t stride_w, int connectivity, int n_classes, const int32_t* class_values,
                         const int32_t* keep_k, int64_t min_size, int fill, void* labels_out, int64_t* stats_out, int32_t* status_out,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Fill the enclosed holes of a label map by their enclosing class: the step after mi3d_keep_components (which turns a wrong-class
 * island inside an organ into such a hole).  Integers only, the same bits on every run.  labels as above; S =
 * scipy.ndimage.generate_binary_structure(3, connectivity).
 *   background component   a component of labels == 0 (an int64 value exactly 0) of one sample under S.
 *   ring                   the positions that are not in the component but are S-neighbours of one of its voxels, positions outside
 *                          the volume included.
 *   enclosed               no ring position lies outside the volume: none of the component's voxels lies on a face of the sample.
 *   filled with v          enclosed, every ring voxel carries the same value v, v is a listed class (1..255), and the component has
 *                          at most max_size voxels (max_size = 0: no limit).  Its voxels become v.
 * Every other voxel is copied: open components, enclosed ones whose ring carries two or more values (MIXED), and ones whose single
 * ring value is unlisted or an int64 value outside 0..255 (SKIPPED, as is a component above max_size).  All int64 values outside
 * 0..255 count as ONE ring value, "other": a ring of 300 and -5 alone is skipped, not mixed; the map is the same either way.
 * The host route this replaces: ids, n = scipy.ndimage.label(labels == 0, S); per component, on a copy padded by one voxel,
 * ring = binary_dilation(comp, S) & ~comp and np.unique of the padded map on the ring; on a map with the single class c the result is
 * scipy.ndimage.binary_fill_holes(labels == c, S) * c.  monai.transforms.FillHoles states the same idea (enclosed background, one
 * enclosing label, applied_labels); this contract is not pinned against MONAI.
 * labels_out: dtype and strides of labels; may be labels itself.  class_values: a HOST array of n_classes (1..8) distinct values in
 * 1..255.  stats_out: (N, n_classes, 2) int64, per listed class [0] holes filled [1] voxels filled.  summary_out: (N, 4) int64,
 * [0] enclosed components [1] filled [2] mixed [3] skipped; [0] = [1] + [2] + [3].  status_out: as above.  workspace:
 * mi3d_fill_holes_workspace_bytes bytes (23 per voxel, rounded up), 256-byte aligned; the domain of mi3d_components_workspace_bytes.
 * Every argument is checked before the first launch. */
size_t mi3d_fill_holes_workspace_bytes(int N, int D, int H, int W);
int mi3d_fill_holes(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d, int64_t stride_h,
                    int64_t stride_w, int connectivity, int n_classes, const int32_t* class_values, int64_t max_size, void* labels_out,
                    int64_t* stats_out, int64_t* summary_out, int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream);

/* Surface distances between two label maps: the exact Euclidean distance transform and, from it, the Hausdorff distance, its
 * percentile (HD95), the average symmetric surface distance (ASSD) and the surface Dice (NSD) per (sample, class): what a user does
 * on the host today with scipy.ndimage.binary_erosion and scipy.ndimage.distance_transform_edt per class and direction.  The
 * reference computes no surface metric, so scipy (the conventions of monai.metrics and medpy) is the contract.  Maps: N samples of
 * sides D, H, W seen through element strides (any dense layout per sample), uint8 or int64.  spacing: 3 HOST doubles (sd, sh, sw),
 * mm per voxel along d, h, w, positive and finite, read before the call returns.
 *   surface    S(M) = M & ~scipy.ndimage.binary_erosion(M, scipy.ndimage.generate_binary_structure(3, connectivity)), border_value 0:
 *              a voxel of M with a neighbour (connectivity 1, 2, 3 = 6, 18, 26 neighbours) outside M or outside the volume.
 *   g3         the squared distance to a set F, in IEEE double, every operation rounded on its own, defined separably:
 *                g1[d,h,w] = min over w' with F[d,h,w'] of fl((sw (w - w'))^2), +inf if the row has none
 *                g2[d,h,w] = min over h' of fl(g1[d,h',w] + fl((sh (h - h'))^2))
 *                g3[d,h,w] = min over d' of fl(g2[d',h,w] + fl((sd (d - d'))^2))
 *              the minimum of these expressions themselves; +inf everywhere for an empty F.  sqrt(g3) is
 *              scipy.ndimage.distance_transform_edt(~F, sampling=spacing): bit for bit where every term is exact in double (spacings
 *              such as (1, 1, 1), (2.5, 0.75, 0.75), (3, 1, 1.5)), within rounding elsewhere (scipy adds the terms in another order).
 * The same bits on every run (integer atomics; the float sum through fixed slots in a fixed order).  Nothing allocates or
 * synchronises; no loop is unbounded, so there is no status word.  workspace: mi3d_surface_workspace_bytes bytes (34 per voxel plus
 * the partial sums, rounded up), 256-byte aligned, for every entry below; 0 (and an error) for N outside [1, 65535], a side < 1,
 * D * H * W >= 2^31 or n_classes outside [1, MI3D_COMPONENTS_MAX_CLASSES]. */
#define MI3D_SURFACE_MAX_TOLERANCES 4
#define MI3D_SURFACE_COUNT_COLUMNS (2 + 2 * MI3D_SURFACE_MAX_TOLERANCES)
#define MI3D_SURFACE_TABLE_COLUMNS 8
size_t mi3d_surface_workspace_bytes(int N, int D, int H, int W, int n_classes);
/* dist2_out (N, D, H, W) float64, contiguous: g3 to F = the non-zero voxels of mask, at every voxel;
 * numpy.sqrt(dist2_out) replaces scipy.ndimage.distance_transform_edt(mask == 0, sampling=spacing).  The workspace of
 * mi3d_surface_workspace_bytes(N, D, H, W, 1). */
int mi3d_distance_transform(const void* mask, int mask_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d, int64_t stride_h,
                            int64_t stride_w, const double* spacing, double* dist2_out, void* workspace, size_t workspace_bytes,
                            void* stream);
/* surface_out (N, D, H, W) uint8, contiguous: 1 on S(labels == class_value), else 0; replaces
 * M & ~scipy.ndimage.binary_erosion(M, scipy.ndimage.generate_binary_structure(3, connectivity)) of M = (labels == class_value).
 * Any int32 class_value; a value a uint8 map cannot hold has an empty surface. */
int mi3d_surface_mask(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d, int64_t stride_h,
                      int64_t stride_w, int connectivity, int class_value, uint8_t* surface_out, void* stream);
/* Per (sample, listed class c), with P = S(pred == c), G = S(target == c), direction 0 the distances A = {sqrt(g3 to G)[p] : p in P}
 * and direction 1 B = {sqrt(g3 to P)[g] : g in G}; replaces, per class and direction, distance_transform_edt(~G, sampling=spacing)[P].
 * class_values: a HOST array of n_classes (1..8) distinct int32 values.  q in [0, 1]: the quantile of the order statistics
 * (percentile / 100); with n values they are those of rank lo = floor((n - 1) q) and hi = ceil((n - 1) q) in ascending order
 * (numpy.percentile's linear method interpolates between them).  tol_mm: a HOST array of n_tol (0..4) finite tolerances >= 0 in mm.
 * counts_out (N, n_classes, 10) int64: [0] |P|  [1] |G|  [2 + 4 dir + t] how many of the direction have g3 <= fl(tol_mm[t]^2), 0 for
 *   t >= n_tol.
 * table_out (N, n_classes, 8) float64, per direction dir four columns from 4 dir: [0] max g3  [1] g3 of rank lo  [2] g3 of rank hi
 *   [3] the sum of sqrt(g3).  Squared where it can be: the host's correctly rounded sqrt then makes the Hausdorff distance and the
 *   order statistics exact.  For a direction without voxels the three g3 entries are +inf and the sum is 0; where only the other
 *   surface is empty they and the sum are +inf. */
int mi3d_surface_distances(const void* pred, int pred_dtype, int64_t pred_stride_n, int64_t pred_stride_d, int64_t pred_stride_h,
                           int64_t pred_stride_w, const void* target, int target_dtype, int64_t target_stride_n, int64_t target_stride_d,
                           int64_t target_stride_h, int64_t target_stride_w, int N, int D, int H, int W, int connectivity, int n_classes,
                           const int32_t* class_values, const double* spacing, double q, int n_tol, const double* tol_mm,
                           int64_t* counts_out, double* table_out, void* workspace, size_t workspace_bytes, void* stream);
/* Signed distance maps of a target, what the boundary loss (mi3d_boundary_loss) multiplies the probabilities with; replaces the two
 * scipy.ndimage.distance_transform_edt calls per class and sample of Kervadec's one_hot2dist.  labels: as above (N samples through
 * element strides, uint8 or int64).  class_values: a HOST array of n_classes (1..8) distinct int32 values; N * n_classes <= 65535.
 * inner_offset: a HOST double >= 0.  Per sample and listed class c, with M = (labels == c):
 *   a = sqrt(g3(x, M))       the distance of x to the nearest voxel of the class            (double, correctly rounded)
 *   b = sqrt(g3(x, ~M))      the distance of x to the nearest voxel outside the class
 *   phi[x] = (float)a                            x outside M
 *   phi[x] = (float)(0 - (b - inner_offset))     x inside M      (a zero is +0)
 *   phi[x] = 0                                   wherever the distance it needs is +inf: an absent class and a class that fills its
 *                                                sample both give an all-zero map (scipy measures to a phantom voxel there)
 * one rounding of the double to float32.  Off those two cases this is one_hot2dist with `sampling`,
 * edt(~M) * ~M - (edt(M) - 1) * M, when inner_offset = 1; at another spacing the smallest of the three spacings is the largest
 * offset that keeps phi <= 0 inside the class.  phi_out: float32, contiguous (N, n_classes, D, H, W).  One sweep of the w and h
 * passes over N * n_classes * 2 jobs; the last pass takes the d pass of the one direction a voxel needs.  The same bits on every run
 * and for every dense layout of the same map; nothing allocates or synchronises; every argument is checked before the first launch.
 * workspace: mi3d_signed_distance_workspace_bytes bytes (34 per voxel and map, rounded up), 256-byte aligned; 0 (and an error)
 * outside the domain above. */
size_t mi3d_signed_distance_workspace_bytes(int N, int D, int H, int W, int n_classes);
int mi3d_signed_distance_maps(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d,
                              int64_t stride_h, int64_t stride_w, int n_classes, const int32_t* class_values, const double* spacing,
                              double inner_offset, float* phi_out, void* workspace, size_t workspace_bytes, void* stream);

/* Spatial augmentation of ONE (C, D, H, W) sample: random_flip (np.flip over axes 1, 2, 3, utils/dataloader.py:207-213) and
 * random_rotate (scipy.ndimage.rotate(reshape=False, mode='nearest') in one plane, order=1 image / order=0 label, :215-221)
 * with the random decisions already drawn by the host (spatial.py), as one gather pass.  img: float32, lab: int64, both
 * contiguous (C, D, H, W); either pair may be NULL; in != out.  (ax0, ax1), 1 <= ax0 < ax1 <= 3, is the plane; matrix (2x2,
 * row-major) and offset (2) are HOST doubles, read before the call returns.  Per output voxel with plane indices (o0, o1) and
 * plane sides (n0, n1), in IEEE double, every operation rounded on its own (no FMA):
 *   cc_i = (o0*M[i][0] + o1*M[i][1]) + off[i], clamped to [0, n_i - 1]
 *   label  source index floor(cc_i + 0.5) per plane axis, value copied
 *   image  f_i = floor(cc_i), t_i = cc_i - f_i, upper neighbour min(f_i + 1, n_i - 1); weights (1-t0)(1-t1), (1-t0)t1, t0(1-t1),
 *          t0 t1; sum of weight * value in the order (f0,f1), (f0,f1+1), (f0+1,f1), (f0+1,f1+1); one rounding to float32
 * Every plane parallel to the two axes and every channel uses the same coordinates.  flip_mask bit k reverses the SOURCE index
 * on axis k+1 (n - 1 - i) after the mapping, so the call equals rotate(flip(x)) bit for bit.  matrix = identity and offset = 0
 * is a pure flip: a copy with reversed indices whose output is bitwise the gather's for finite values (the gather turns -0.0
 * into +0.0 and 0 * Inf into NaN; the copy keeps both).  Allocates nothing, does not synchronise.  Negative return: bad axes,
 * null or aliased in/out, non-positive sizes, more than 2^31 - 1 voxels, flip_mask outside 0..7. */
int mi3d_plane_affine(const float* img_in, float* img_out, const int64_t* lab_in, int64_t* lab_out, int C, int D, int H, int W,
                      int ax0, int ax1, const double* matrix, const double* offset, int flip_mask, void* stream);

/* Affine + elastic spatial augmentation of ONE sample: the MONAI RandAffined / Rand3DElasticd block that combined_transform() lists
 * and leaves commented out (utils/dataloader.py:227-248), as one smoothed random displacement field and one gather that reads image
 * and label through the same coordinates (spatial.py draws the parameters).
 *
 * mi3d_elastic_field writes the float32 field u (3, D, H, W); component a displaces along axis a of (D, H, W).  V = D*H*W, idx the
 * C-order voxel index:
 *   noise   r = mix64a(mix64a(seed) ^ (uint64)(a*V + idx)), k = r >> 40, noise = (float)((int)k - 2^23) * 2^-23: an exact dyadic in
 *           [-1, 1), never stored
 *   taps    a HOST table of 2*radius + 1 doubles, taps[j + radius] = g[j], read before the call returns; radius <=
 *           MI3D_ELASTIC_MAX_RADIUS.  (MONAI's GaussianFilter(sigma, truncated=3.0, approx="erf") table: spatial.gaussian_taps)
 *   smooth  three separable passes in the order W, H, D, zeros beyond the volume: out[i] = sum over j of g[j] * (double)src[i + j]
 *           (scipy.ndimage.correlate1d(mode='constant', cval=0)), a float64 sum in ascending j, every product and sum rounded on its
 *           own (no FMA), taps beyond the volume skipped; each pass rounds once to float32
 * workspace: mi3d_elastic_workspace_bytes(D, H, W), 16-byte aligned, not the field.  Negative return: null pointers, non-positive
 * sizes, more than 2^31 - 1 field values, radius outside 0..MI3D_ELASTIC_MAX_RADIUS, workspace too small.
 *
 * mi3d_warp3 gathers img_out (C, Do, Ho, Wo) float32 and lab_out (C, Do, Ho, Wo) int64 from img_in / lab_in (C, D, H, W), all
 * contiguous; either pair may be NULL; in != out.  matrix (3x3, row-major) and translate (3) are HOST doubles, read before the call
 * returns; field is NULL or a device (3, Do, Ho, Wo) float32 field on the OUTPUT grid.  Per output voxel o, with n = (D, H, W) and
 * no = (Do, Ho, Wo), in IEEE double, every operation rounded on its own (no FMA), in this order:
 *   c_a = (double)o_a - (no_a - 1)/2
 *   p_a = c_a + magnitude * (double)u_a[o]                  (field NULL: p_a = c_a)
 *   s_a = ((M[a][0]*p_0 + M[a][1]*p_1) + M[a][2]*p_2) + ((n_a - 1)/2 + t_a)
 * M maps output coordinates to sampling coordinates (a pull), both voxel-centred about the middle of their grid.
 *   outside  any s_a that is not 0 <= s_a <= n_a - 1 (so a NaN coordinate is outside), decided first; then every s_a is clamped to
 *            [0, n_a - 1], a NaN to 0
 *   image    f_a = floor(s_a), t_a = s_a - f_a, upper tap min(f_a + 1, n_a - 1); the W level lo*(1 - t) + hi*t on the four (d, h) rows,
 *            then H, then D, in double; one rounding to float32   (scipy.ndimage.map_coordinates(order=1))
 *   label    the voxel floor(s_a + 0.5) per axis, value copied         (order=0)
 *   padding  MI3D_PAD_BORDER: as above (scipy mode='nearest'); MI3D_PAD_ZEROS: 0 where outside, as above elsewhere (mode='constant',
 *            cval=0); one mode each for image and label
 * Every channel uses the same coordinates.  No index outside the input is formed: a NaN coordinate reads voxel 0 under
 * MI3D_PAD_BORDER and gives 0 under MI3D_PAD_ZEROS.  Allocates nothing,
 * does not synchronise.  Negative return: null matrix / translate, a pair with only one of in / out, aliased in / out, non-positive
 * sizes, more than 2^31 - 1 voxels in a volume, an unknown padding mode. */
#define MI3D_ELASTIC_MAX_RADIUS 32      /* covers sigma <= 10.5 of the truncated=3.0 table */
#define MI3D_PAD_BORDER 0
#define MI3D_PAD_ZEROS 1
size_t mi3d_elastic_workspace_bytes(int D, int H, int W);
int mi3d_elastic_field(float* field, int D, int H, int W, uint64_t seed, const double* taps, int radius, void* workspace,
                       size_t workspace_bytes, void* stream);
int mi3d_warp3(const float* img_in, float* img_out, const int64_t* lab_in, int64_t* lab_out, int C, int D, int H, int W, int Do, int Ho,
               int Wo, const double* matrix, const double* translate, const float* field, double magnitude, int image_padding,
               int label_padding, void* stream);
/* mi3d_warp3 with the window placed on a start that lives on the device.  start: NULL, or three DEVICE int32 (a row of
 * mi3d_patch_pick's starts_out), the input voxel under the window's first voxel; read by the kernel, never by the host.  With start
 * the last line of the contract above becomes
 *   s_a = ((M[a][0]*p_0 + M[a][1]*p_1) + M[a][2]*p_2) + (((double)start_a + (no_a - 1)/2) + t_a)
 * so the window's middle sits at start + (no - 1)/2 instead of at the input's middle; any int32 is a valid start (the coordinates
 * are clamped as above).  With the identity matrix, no field and t = 0, s_a = o_a + start_a exactly: the call then equals
 * mi3d_patch_crop for a start inside the volume and finite inputs without -0.0.  start == NULL is mi3d_warp3, bit for bit. */
int mi3d_warp3_at(const float* img_in, float* img_out, const int64_t* lab_in, int64_t* lab_out, int C, int D, int H, int W, int Do,
                  int Ho, int Wo, const double* matrix, const double* translate, const float* field, double magnitude,
                  int image_padding, int label_padding, const int32_t* start, void* stream);

/* Foreground-balanced patch sampling: where MONAI's RandCropByPosNegLabeld / RandCropByLabelClassesd put their windows, found on the
 * device from random words the host drew without knowing any count (spatial.py draws them), and the windows cut in one launch.
 * labels: N samples of sides D, H, W seen through element strides (any dense layout per sample), uint8 or int64, the view of
 * mi3d_keep_components.  A voxel's index is d*H*W + h*W + w over the logical axes; V = D*H*W.
 *   group_of   a HOST table of 256 bytes read before the call returns: group_of[v] is the group 0..MI3D_COMPONENTS_MAX_CLASSES-1 of
 *              label value v, or 255 for "in no group".  G = 1 + the largest group named.  An int64 value outside 0..255 is in no
 *              group; it is tested as it is, never narrowed to a byte first.  (PosNeg: group_of[0] = 0, group_of[v > 0] = 1; per
 *              class: group_of[v] = v.)
 *   mulhi64    mulhi64(a, b) = floor(a * b / 2^64) of two unsigned 64-bit words (__umul64hi)
 * Integer arithmetic only (integer atomics of sums): the same bits on every run.  Nothing allocates or synchronises.
 * workspace: mi3d_patch_workspace_bytes bytes, 256-byte aligned: int32 [N][8][ceil(V / MI3D_PATCH_BLOCK)], the voxels of every group
 * in every block of MI3D_PATCH_BLOCK consecutive voxel indices of a sample; 0 (and an error) for N outside [1, 65535], a side < 1 or
 * V >= 2^31. */
#define MI3D_PATCH_BLOCK 4096
size_t mi3d_patch_workspace_bytes(int N, int D, int H, int W);
/* One pass over labels writes the workspace and counts_out (N, G) int64 (8-byte aligned, device): the voxels of each group per
 * sample.  Rows along a unit W stride are read in 16-byte loads; any other layout is read strided, one element per load. */
int mi3d_patch_count(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d, int64_t stride_h,
                     int64_t stride_w, const uint8_t* group_of, int64_t* counts_out, void* workspace, size_t workspace_bytes,
                     void* stream);
/* K draws (1..65535) as three HOST arrays read before the call returns: sample[k] in [0, N), group[k] in [0, G), rnd[k] any 64-bit
 * word; labels, group_of and workspace those of the preceding mi3d_patch_count.  For draw k, with c = the voxels of group[k] in
 * sample[k]:
 *   c > 0    r = mulhi64(rnd[k], c); the voxel is the r-th voxel (from 0) of that group in ascending index; picked_out[k] = group[k]
 *   c == 0   the voxel is mulhi64(rnd[k], V), whatever its value; picked_out[k] = -1
 *   start    with (c_d, c_h, c_w) the voxel's coordinates: start_a = clamp(c_a - size_a / 2, 0, n_a - size_a), integer division
 *            (MONAI's correct_crop_centers + SpatialCrop, stated here)
 * size: three HOST ints, 1 <= size_a <= n_a (a larger window is an argument error).  Outputs on the device: starts_out (K, 3),
 * voxel_out (K), picked_out (K), all int32.  One workgroup per draw; 256 draws per launch ride in the kernel's arguments. */
int mi3d_patch_pick(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d, int64_t stride_h,
                    int64_t stride_w, const uint8_t* group_of, int K, const int32_t* sample, const int32_t* group, const uint64_t* rnd,
                    const int32_t* size, int32_t* starts_out, int32_t* voxel_out, int32_t* picked_out, const void* workspace,
                    size_t workspace_bytes, void* stream);
/* K windows of ONE sample in one launch: img_out (K, C, Do, Ho, Wo) float32 and lab_out (K, C, Do, Ho, Wo) int64 from img_in float32
 * and lab_in int64, both (C, D, H, W) contiguous; either pair may be NULL; in != out.  starts: (K, 3) int32 in DEVICE memory, read by
 * the kernel; each start is clamped to [0, n_a - no_a] where it is used, so no index outside the input is formed whatever it holds.
 *   out[k][c][od][oh][ow] = in[c][start_d + od][start_h + oh][start_w + ow]
 * A copy: every bit pattern is kept (NaN payloads, -0.0, Inf).  Negative return: a pair with only one of in / out, aliased in / out,
 * K outside [1, 65535], non-positive sizes, more than 2^31 - 1 input voxels, a window larger than the volume. */
int mi3d_patch_crop(const float* img_in, float* img_out, const int64_t* lab_in, int64_t* lab_out, int K, int C, int D, int H, int W, int Do,
                    int Ho, int Wo, const int32_t* starts, void* stream);

/* Training-set augmentation, combined_transform() (utils/dataloader.py:223-262, used at train_unet.py:361): the
 * arithmetic of MONAI's RandBiasField -> RandGaussianNoise -> RandAdjustContrast -> RandHistogramShift ->
 * RandCoarseDropout on one (C, D, H, W) float volume, with the random parameters already drawn by the host
 * (augment.py draws them from numpy RandomState streams laid out like MONAI's Compose).  A transform whose do_* flag
 * (n_holes for the last) is 0 is skipped, as when MONAI's prob draw fails.
 *   bias      x * exp(field), field = Legendre series (degree <= 3; coefficient order i, j, k with i + j + k <= degree
 *             over the three spatial axes) on linspace(-1, 1, dim) float32 coordinates, evaluated in float64
 *   noise     x + noise[i] (noise != NULL: host-drawn tensor, same shape) or x + N(noise_mean, noise_std) from the
 *             library's counter-based generator seeded with noise_seed (same distribution, different stream)
 *   contrast  ((x - min) / (max - min + 1e-7)) ** gamma * (max - min) + min, min / max over the whole volume
 *   hist      piecewise-linear map through n_cp control points ref_cp -> flt_cp (both on [0, 1], scaled to [min, max])
 *   holes     n_holes boxes [hole_lo, hole_lo + hole_size) over all channels set to fill_value */
#define MI3D_AUG_MAX_COEFF 20
#define MI3D_AUG_MAX_CP 16
#define MI3D_AUG_MAX_HOLES 8
typedef struct mi3d_aug_params {
    int32_t do_bias, bias_degree;
    double bias_coeff[MI3D_AUG_MAX_COEFF];
    int32_t do_noise;
    float noise_mean, noise_std;
    uint64_t noise_seed;
    int32_t do_contrast;
    float gamma;
    int32_t do_hist, n_cp;
    float ref_cp[MI3D_AUG_MAX_CP], flt_cp[MI3D_AUG_MAX_CP];
    int32_t n_holes;
    int32_t hole_size[3];
    int32_t hole_lo[MI3D_AUG_MAX_HOLES][3];
    float fill_value;
} mi3d_aug_params;
size_t mi3d_augment_workspace_bytes(void);
/* in == out allowed.  workspace: mi3d_augment_workspace_bytes(), 16-byte aligned. */
int mi3d_augment(const float* in, float* out, const float* noise, int C, int D, int H, int W, const mi3d_aug_params* params,
                 void* workspace, size_t workspace_bytes, void* stream);
/* the label half of RandCoarseDropoutd: the same boxes set to `fill` in an int64 (C, D, H, W) label volume, in place */
int mi3d_fill_boxes_i64(int64_t* label, int C, int D, int H, int W, int n_holes, const int32_t* hole_lo,
                        const int32_t* hole_size, int64_t fill, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Per-operator entry points (channels-last activations; used by the parity tests and by stand-alone modules).
 * x/y: `dtype` tensors [N][D][H][W][C] with channel stride xcs/ycs (elements).
 * ---------------------------------------------------------------------------------------------------------- */
/* nn.Conv3d(k=3,p=1) unet.py:11,15.  w (Cout,Cin,3,3,3) float.  workspace: mi3d_conv3_workspace_bytes */
size_t mi3d_conv3_workspace_bytes(int Cin, int Cout, int N, int D, int H, int W);
int mi3d_conv3_forward(int in_dtype, int out_dtype, const void* x, int xcs, int Cin, const float* w, const float* bias,
                       void* y, int ycs, int Cout, int N, int D, int H, int W, void* workspace, size_t workspace_bytes,
                       void* stream);
/* dx may be NULL (first layer); dW (Cout,Cin,3,3,3), db (Cout) float */
int mi3d_conv3_backward(int x_dtype, int dy_dtype, const void* x, int xcs, int Cin, const float* w, const void* dy,
                        int dycs, int Cout, void* dx, int dxcs, float* dW, float* db, int accumulate, int N, int D,
                        int H, int W, void* workspace, size_t workspace_bytes, void* stream);
/* One half of a DoubleConv block as the training forward of the whole-network plan runs it: Conv3d(k=3,p=1) -> train-mode
 * BatchNorm3d statistics -> ReLU + Dropout3d apply (-> MaxPool3d(2,2)), with the plan's own route decisions (the plan and this
 * entry call ONE function).  in_dtype = dtype, or MI3D_F32 for the one-channel image of the first layer; y [M][Cout] is the conv
 * output BatchNorm reads, z the activated tensor, pooled NULL or MaxPool3d(2,2)(z) on even volumes.  route_out (may be NULL)
 * reports what was launched:
 *   conv    0 direct fp32-FMA, 1 first-layer MFMA, 2 persistent MFMA, 3 MFMA with the 16-wide tile, 4 MFMA with the 8-wide tile
 *   ksplit  split-K factor of the conv launch (1 = none);  ticket  1 = the split-K launch finished itself
 *   stats   0 a statistics pass over y, 1 partial rows finished by the apply pass, 2 partial rows + a finalize launch,
 *           3 split-K partials finished by the statistics pass
 *   rows    partial rows handed on (0 = none);  rows_offset  byte offset in the workspace of those rows ([rows][2][Cout] float)
 * The entry clears the split-K ticket counters in its weight-pack launch as the plan does; MI3D_CONV3_BN_KEEP_TICKETS in flags
 * skips that (the previous call on this workspace left them at zero). */
typedef struct mi3d_conv3_bn_route { int32_t conv, ksplit, ticket, stats, rows, rows_offset; } mi3d_conv3_bn_route;
enum { MI3D_CONV3_BN_KEEP_TICKETS = 1 };
size_t mi3d_conv3_bn_workspace_bytes(int in_dtype, int dtype, int Cin, int Cout, int N, int D, int H, int W);
int mi3d_conv3_bn_forward(int in_dtype, int dtype, const void* x, int xcs, int Cin, const float* w, const float* bias,
                          const float* gamma, const float* beta, float* running_mean, float* running_var,
                          int64_t* num_batches_tracked, float momentum, float eps, const float* drop, void* y, void* z, int zcs,
                          void* pooled, int pcs, float* stat, int flags, mi3d_conv3_bn_route* route_out, int Cout, int N, int D,
                          int H, int W, void* workspace, size_t workspace_bytes, void* stream);
/* One half of a DoubleConv block as the inference forward of the whole-network plan (mi3d_unet_infer) runs it: eval-mode
 * BatchNorm3d folded into the conv, ReLU in the conv's epilogue, z = relu(conv(x, w * scale) + fbias) with
 *   scale = gamma / sqrt(running_var + eps),  fbias = (bias - running_mean) * scale + beta       (bias NULL = 0)
 * through the plan's own launches in the plan's order (the fold, the weight pack carrying the scale, then the ONE function the
 * plan calls per layer).  in_dtype = dtype, or MI3D_F32 for the one-channel image of the first layer; z has channel stride zcs
 * (the concat buffer's 2 * Cout, say).  x_split, x_delta: planar halves of x as in mi3d_conv3_bn_backward (0, 0 = one plane; only
 * the persistent kernels take them).  fold_out (may be NULL): device float[2 * Cout] that receives scale, then fbias.  route_out
 * (may be NULL): conv = the codes of mi3d_conv3_bn_route, ksplit = split-K factor of the launch (1 = none; the scratch is handed
 * over only to an output with 16-byte aligned rows). */
typedef struct mi3d_conv3_infer_route { int32_t conv, ksplit; } mi3d_conv3_infer_route;
size_t mi3d_conv3_infer_workspace_bytes(int in_dtype, int dtype, int Cin, int Cout, int N, int D, int H, int W);
int mi3d_conv3_infer_forward(int in_dtype, int dtype, const void* x, int xcs, int x_split, int64_t x_delta, int Cin,
                             const float* w, const float* bias, const float* gamma, const float* beta,
                             const float* running_mean, const float* running_var, float eps, void* z, int zcs, float* fold_out,
                             mi3d_conv3_infer_route* route_out, int Cout, int N, int D, int H, int W, void* workspace,
                             size_t workspace_bytes, void* stream);
/* One half of a DoubleConv block as the training backward of the whole-network plan runs it: BatchNorm3d + ReLU + Dropout3d
 * backward (dz -> dy, dgamma, dbeta), then the conv's weight / bias gradient and input gradient, with the plan's own per-layer
 * decisions (the plan and this entry call ONE function) on a workspace of its own.  x is the layer's input, y / stat / drop what
 * the forward saved, dz the gradient of the activated output, dy [M][Cout] the buffer the conv's output gradient is written to.
 *   stat == NULL          no BatchNorm: dz is the conv's dy (what mi3d_conv3_backward means); y, drop, dy, dgamma, dbeta unused
 *   dz_partials, dz_ks    dz arrives as fp32 split-K partials [dz_ks][M][Cout]; the reduction sums and rounds them and WRITES dz
 *   x_split, x_delta      planar halves of x: 16-channel block b >= x_split lies x_delta elements further (0, 0 = one plane);
 *   dx_split, dx_delta    the same for dx.  Only the full-resolution (persistent) kernels and the weight gradient honour them
 *   riders[2]             NULL, or up to two pending sums (nblocks > 0) carried in this call's BatchNorm-backward reduction
 *   pending_out           with MI3D_CONV3_BN_BWD_LEAVE_PENDING: the layer's slab sum is NOT launched but returned here
 * flags
 *   MI3D_CONV3_BN_BWD_ALLOW_PARTIALS  a split-K dx may stay as fp32 partials [dx_ks][M][Cin] in the workspace at dx_offset (dx is
 *                                     then not written); whoever reads them finishes them
 *   MI3D_CONV3_BN_BWD_DEFER           the deferred layer's route, run in order on the given stream: the input gradient alone, then
 *                                     the stand-alone weight gradient cut into the slabs of the layer's fused launch
 *   MI3D_CONV3_BN_BWD_LEAVE_PENDING   see pending_out
 * route_out (may be NULL) reports what was launched:
 *   bn           0 none, 1 reduction + finalize + apply, 2 reduction + apply (the apply pass finishes the rows in its prologue)
 *   riders       pending sums carried by the reduction (0, 1, 2);  dz_ks  split factor of the dz partials consumed (0 = stored dz)
 *   conv         0 direct fp32-FMA kernels, 1 first-layer weight gradient only, 2 fused persistent, 3 fused with the 16-wide tile,
 *                4 fused with the 8-wide tile, 5 stand-alone pair (weight gradient, then input gradient), 6 deferred pair
 *   dgrad_ks     split-K factor of the input gradient (1 = none, 0 = no input gradient);  dx_ks  split factor of a dx LEFT as
 *                partials (0 = dx written);  dx_offset  byte offset of those partials in the workspace
 *   slabs, slab_layout, slab_ew   weight-gradient slabs summed, the sum's layout (0 element order, 1 MFMA order, 2 MFMA order
 *                through an LDS transpose) and elements per block (0 for layout 2); all 0 for the direct kernels
 *   pending      1 = the sum was left in pending_out */
typedef struct mi3d_pending_sum { int64_t opaque[9]; } mi3d_pending_sum;      /* a slab sum waiting for a launch; plain data */
typedef struct mi3d_conv3_bn_bwd_route {
    int32_t bn, riders, dz_ks, conv, dgrad_ks, dx_ks, dx_offset, slabs, slab_layout, slab_ew, pending;
} mi3d_conv3_bn_bwd_route;
enum { MI3D_CONV3_BN_BWD_ALLOW_PARTIALS = 1, MI3D_CONV3_BN_BWD_DEFER = 2, MI3D_CONV3_BN_BWD_LEAVE_PENDING = 4 };
size_t mi3d_conv3_bn_bwd_workspace_bytes(int in_dtype, int dtype, int Cin, int Cout, int N, int D, int H, int W);
int mi3d_conv3_bn_backward(int in_dtype, int dtype, const void* x, int xcs, int x_split, int64_t x_delta, int Cin, const float* w,
                           const void* y, const float* stat, const float* drop, void* dz, int dzcs, const float* dz_partials,
                           int dz_ks, void* dy, void* dx, int dxcs, int dx_split, int64_t dx_delta, float* dW, float* db,
                           float* dgamma, float* dbeta, int accumulate, const mi3d_pending_sum* riders, mi3d_pending_sum* pending_out,
                           int flags, mi3d_conv3_bn_bwd_route* route_out, int Cout, int N, int D, int H, int W, void* workspace,
                           size_t workspace_bytes, void* stream);
/* launches a pending sum on its own (what the plan does with the last one of a call) */
int mi3d_pending_sum_launch(const mi3d_pending_sum* job, void* stream);
/* BatchNorm3d(train) + ReLU + Dropout3d fused; stat: device float[4*C] saved for backward */
size_t mi3d_bn_workspace_bytes(int C);
int mi3d_bn_relu_drop_forward(int dtype, const void* y, int ycs, int C, int64_t M, int64_t V, const float* gamma,
                              const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                              float momentum, float eps, int training, const float* drop, void* z, int zcs, float* stat,
                              void* workspace, void* stream);
int mi3d_bn_relu_drop_backward(int dtype, const void* dz, int dzcs, const void* y, int ycs, int C, int64_t M, int64_t V,
                               const float* stat, const float* drop, void* dy, int dycs, float* dgamma, float* dbeta,
                               int accumulate, void* workspace, void* stream);
/* the second half of an encoder block as the training step runs it (unet.py:16-18 then :71): train-mode BatchNorm3d + ReLU +
 * Dropout3d writing z AND pooled = MaxPool3d(2,2)(z) in one pass.  Even D, H, W; pooled [N][D/2][H/2][W/2][C], stride pcs */
int mi3d_bn_relu_drop_pool_forward(int dtype, const void* y, int ycs, int C, int N, int D, int H, int W, const float* gamma,
                                   const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                   float momentum, float eps, const float* drop, void* z, int zcs, void* pooled, int pcs,
                                   float* stat, void* workspace, void* stream);
int mi3d_maxpool2_forward(int dtype, const void* z, int zcs, int C, int N, int D, int H, int W, void* p, int pcs,
                          void* stream);
int mi3d_maxpool2_backward(int dtype, const void* dp, int dpcs, const void* z, int zcs, const void* dskip, int dskipcs,
                           void* dz, int dzcs, int C, int N, int D, int H, int W, void* stream);
/* the same with dp not yet written: it is still the ks fp32 split-K partials [ks][M/8][C] of the conv that produces it */
int mi3d_maxpool2_backward_partials(int dtype, const float* dp_partials, int ks, const void* z, int zcs, const void* dskip,
                                    int dskipcs, void* dz, int dzcs, int C, int N, int D, int H, int W, void* stream);
/* ConvTranspose3d(k2,s2) unet.py:56-58.  w (Cin,Cout,2,2,2) float; geometry = INPUT volume */
size_t mi3d_upconv2_workspace_bytes(int Cin, int Cout, int N, int D, int H, int W);
int mi3d_upconv2_forward(int dtype, const void* x, int xcs, int Cin, const float* w, const float* bias, void* y, int ycs,
                         int Cout, int N, int D, int H, int W, void* workspace, size_t workspace_bytes, void* stream);
int mi3d_upconv2_backward(int dtype, const void* x, int xcs, int Cin, const float* w, const void* gy, int gycs, int Cout,
                          void* dx, int dxcs, float* dW, float* db, int accumulate, int N, int D, int H, int W,
                          void* workspace, size_t workspace_bytes, void* stream);
/* One decoder up step as the whole-network plan runs it (the plan and these entries call ONE function pair): ConvTranspose3d(k2,s2)
 * of x (N,D,H,W,Cin) into the up half of a concat buffer, given as a pointer `up` and a channel stride `ucs` (interleaved halves:
 * cat + Cout with ucs = 2 Cout; planar halves: ucs = Cout), whose geometry is (Do,Ho,Wo).  Where (Do,Ho,Wo) is not (2D,2H,2W) the
 * transposed conv writes a temporary in the workspace and F.interpolate(mode="nearest") resizes it into the half (unet.py:81-83).
 * mi3d_up_backward is the adjoint: gup is the gradient of that half; dx, dW, db may each be NULL.
 * flags
 *   MI3D_UP_BWD_LEAVE_PENDING      the MFMA route's slab sum is NOT launched but returned in pending_out (launch it with
 *                                  mi3d_pending_sum_launch or hand it to mi3d_conv3_bn_backward as a rider)
 *   MI3D_UP_BWD_SECOND_WORKSPACE   the slabs go to the second slab region of the workspace, as in the plan while the decoder conv's
 *                                  sum waits in the first (the plan's carry)
 * route_out (may be NULL) reports what was launched; fields that do not apply are 0:
 *   forward    kind 0 direct fp32-FMA / 1 MFMA;  gy  grid size over output-channel blocks;  tap_split  1 = the 8 taps are spread over
 *              workgroups;  wide  1 = 16-byte stores of x-neighbour pairs;  strided  1 = some workgroup takes more than one round of
 *              voxel groups;  resized  1 = temporary + nearest resize
 *   backward   kind 0 direct / 1 fused launch / 2 stand-alone pair / 3 dx only / 4 weights only;  ksplit  1 = K-split input
 *              gradient;  persistent  1 = the input-gradient workgroups take more than one round;  slabs, slab_ew  weight-gradient
 *              slabs summed and elements per block of the sum;  wgrad_blocks, dgrad_blocks  workgroups of each kind;
 *              pending  1 = the sum was left in pending_out;  resized  1 = the resize adjoint ran first
 * workspace: mi3d_up_workspace_bytes, 256-byte aligned; mi3d_up_workspace_region(..., which, &bytes) returns the byte offset of
 * region which = 0 packed weights, 1 temporary, 2 first slab region, 3 second slab region. */
typedef struct mi3d_up_route {
    int32_t kind, gy, tap_split, wide, strided, resized, ksplit, persistent, slabs, slab_ew, wgrad_blocks, dgrad_blocks, pending;
} mi3d_up_route;
enum { MI3D_UP_BWD_LEAVE_PENDING = 1, MI3D_UP_BWD_SECOND_WORKSPACE = 2 };
size_t mi3d_up_workspace_bytes(int dtype, int Cin, int Cout, int N, int D, int H, int W);
size_t mi3d_up_workspace_region(int dtype, int Cin, int Cout, int N, int D, int H, int W, int which, size_t* bytes_out);
int mi3d_up_forward(int dtype, const void* x, int xcs, int Cin, const float* w, const float* bias, void* up, int ucs, int Cout,
                    int N, int D, int H, int W, int Do, int Ho, int Wo, mi3d_up_route* route_out, void* workspace,
                    size_t workspace_bytes, void* stream);
int mi3d_up_backward(int dtype, const void* x, int xcs, int Cin, const float* w, const void* gup, int gucs, int Cout, void* dx,
                     int dxcs, float* dW, float* db, int accumulate, int N, int D, int H, int W, int Do, int Ho, int Wo, int flags,
                     mi3d_pending_sum* pending_out, mi3d_up_route* route_out, void* workspace, size_t workspace_bytes, void* stream);
/* F.interpolate(x, size=(Do,Ho,Wo), mode="nearest") on channels-last tensors, any in / out sides >= 1, and its adjoint (gx[src] =
 * the sum, ascending in (d,h,w), of gy over every destination voxel that reads src; deterministic) */
int mi3d_nearest_resize_forward(int dtype, const void* x, int xcs, int C, int N, int Di, int Hi, int Wi, void* y, int ycs, int Do,
                                int Ho, int Wo, void* stream);
int mi3d_nearest_resize_backward(int dtype, const void* gy, int gycs, int C, int N, int Do, int Ho, int Wo, void* gx, int gxcs,
                                 int Di, int Hi, int Wi, void* stream);
/* final nn.Conv3d(C0, n_classes, 1) unet.py:62,87.  z: channels-last `dtype` [N][V][Cin] (stride zcs); w (Cout,Cin,1,1,1) float;
 * logits / dlogits: NCDHW float (the API layout).  backward: dz (channels-last, stride dzcs), dW (Cout,Cin), db (Cout) float;
 * workspace: mi3d_conv1_workspace_bytes.  The bf16 path runs the MFMA kernels of the training step. */
size_t mi3d_conv1_workspace_bytes(int Cin, int Cout);
int mi3d_conv1_forward(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, float* logits, int Cout,
                       int N, int64_t V, void* stream);
int mi3d_conv1_backward(int dtype, const void* z, int zcs, int Cin, const float* w, const float* dlogits, int Cout, void* dz,
                        int dzcs, float* dW, float* db, int accumulate, int N, int64_t V, void* workspace,
                        size_t workspace_bytes, void* stream);
/* layout helpers: NCDHW float <-> channels-last `dtype` */
int mi3d_ncdhw_to_ndhwc(int dtype, const float* src, void* dst, int dcs, int C, int N, int64_t V, void* stream);
int mi3d_ndhwc_to_ncdhw(int dtype, const void* src, int scs, float* dst, int C, int N, int64_t V, void* stream);

/* hipGraph capture helpers (launch-bound step loops): capture everything launched on `stream` between begin/end */
int mi3d_graph_begin(void* stream);
int mi3d_graph_end(void* stream, void** graph_exec_out);
int mi3d_graph_launch(void* graph_exec, void* stream);
int mi3d_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* MI3D_H */
