// ops.h — internal launcher API (C++), one function per kernel family.  Every launcher
//   * takes raw device pointers + explicit channel strides (see common.h for the layout),
//   * launches on the stream it is given and never synchronises, allocates or frees,
//   * returns 0, a negative argument error, or a positive hipError_t.
// The extern "C" boundary (include/mi3d.h, api.hip) and the whole-network plan (plan.hip) sit on top.
#pragma once
#include "common.h"
#include "slab_sum.h"

struct Geo {
    int N, D, H, W;
    int64_t V() const { return (int64_t)D * H * W; }
    int64_t M() const { return (int64_t)N * D * H * W; }
};

// ---- 3x3x3 convolution, direct (any channel count, any dtype; fp32 FMA) -------------- conv3_direct.hip
// Reference: nn.Conv3d(k=3,p=1) models/unet.py:11,15.  Weights arrive in torch layout (Cout,Cin,3,3,3) fp32.
size_t conv3_direct_pack_floats(int Cin, int Cout);          // size of ONE packed operand (fwd or dgrad)
int conv3_direct_pack(const float* w, int Cin, int Cout, float* wp_fwd, float* wp_dgrad, hipStream_t s,
                      const float* scale = nullptr);     // scale: per-output-channel factor of the forward operand
// y[v,co] = bias[co] + sum_{tap,ci} x[v+tap,ci] * wp ;  dgrad = same call with wp_dgrad, (Cin,Cout) swapped, bias NULL
int conv3_direct_fwd(int in_dtype, int out_dtype, const void* x, int xcs, int Cin, const float* wp,
                     const float* bias, void* y, int ycs, int Cout, Geo g, hipStream_t s, int relu = 0);
// dW[co,ci,tap] (+)= sum_v dy[v,co] x[v+tap,ci] ; db[co] (+)= sum_v dy[v,co].  Deterministic slab reduction.
size_t conv3_direct_wgrad_ws_floats(int Cin, int Cout, Geo g);
int conv3_direct_wgrad(int x_dtype, int dy_dtype, const void* x, int xcs, int Cin, const void* dy, int dycs,
                       int Cout, Geo g, float* dW, float* db, int accumulate, float* ws, size_t ws_floats,
                       hipStream_t s);

// ---- 3x3x3 convolution, MFMA implicit GEMM (bf16, Cin,Cout % 16 == 0) ------------------ conv3_mfma.hip
bool conv3_mfma_supported(int Cin, int Cout, int xcs, int ycs);
size_t conv3_mfma_pack_elems(int Cin, int Cout);             // bf16 elements of ONE packed operand
int conv3_mfma_pack(const float* w, int Cin, int Cout, void* wp_fwd, void* wp_dgrad, Geo g, hipStream_t s);
// All weight packs of a network in ONE launch (every kernel node of the step graph costs ~4.5 us of dispatch floor):
// jobs are appended on the host, the kernel finds its job from the block index.
// scale (conv3 only, may be NULL): per-output-channel factor folded into the FORWARD image (inference: BatchNorm scale)
struct PackJob { const float* w; void* a; void* b; int Cin, Cout, kind, mode_f, mode_d, blk0; const float* scale; };   // kind 0 conv3, 1 upconv
constexpr int MAX_PACK_JOBS = 32;
struct PackJobs { int n, nblocks; PackJob j[MAX_PACK_JOBS]; int* zero = nullptr; int nzero = 0; };      // zero: ints block 0 clears (split-K ticket counters)
int pack_all_add_conv3(PackJobs& J, const float* w, int Cin, int Cout, void* wp_fwd, void* wp_dgrad, Geo g,
                       const float* scale = nullptr);
int pack_all_add_upconv(PackJobs& J, const float* w, int Cin, int Cout, void* wp);
int pack_all_launch(const PackJobs& J, hipStream_t s);
int conv3_mfma_stat_blocks(int Cin, int Cout, Geo g);                           // partials written when `part` != NULL
// dgrad = same call with the dgrad pack and (Cin,Cout) swapped, bias NULL, part NULL
size_t conv3_mfma_splitk_floats(int Cin, int Cout, Geo g);    // K-split scratch for deep (small-M) layers, 0 = none
bool conv3_mfma_fuses_stats(int Cin, int Cout, Geo g);        // false -> caller runs bn_train_stats afterwards
// A tensor whose channels live in TWO planes of the same stride ("planar halves" of a skip/up concat buffer):
// 16-channel block b >= split is found `delta` elements further than the single-plane address would say.
// Default = ordinary single-plane tensor.  Only the persistent full-resolution kernels and wgrad honour it.
struct Halves { int split = 1 << 30; int64_t delta = 0; bool on() const { return delta != 0; } };
inline Halves halves_at(int split, int64_t delta) {      // delta == 0: the single-plane default, whatever split says
    Halves h;
    if (delta) { h.split = split; h.delta = delta; }
    return h;
}
bool conv3_mfma_halves_ok(int Cin, int Cout, Geo g);          // forward (Cin,Cout) launch can take Halves x / y
// The split-K forward launch of this layer can finish itself: the LAST of the ks workgroups of an (output tile, channel group) to
// arrive (one atomic ticket per workgroup on a counter only those ks workgroups touch) sums the ks fp32 partials in k order, adds
// the bias, stores bf16 y and writes the tile's BatchNorm partial row -- the bn_stats_splitk launch of the layer disappears and
// the consumer finishes <= 108 tile rows instead of 128 block rows.  Same bits in y as the separate finishing pass.
bool conv3_mfma_ticket_ok(int Cin, int Cout, Geo g);
constexpr int CONV3_TK_COUNTERS = 4096;         // ints of counter space a plan reserves
// what conv3_mfma_fwd launched (filled in at the branch it took): kind 2 = persistent, 3 = 16-wide tile, 4 = 8-wide tile (the
// codes of mi3d_conv3_bn_route::conv); ks = split-K factor of the launch
struct Conv3Launch { int kind = 0, ks = 1; };
int conv3_mfma_fwd(const void* x, int xcs, int Cin, const void* wp, const float* bias, void* y, int ycs, int Cout,
                   Geo g, float* part, float* skws, hipStream_t s, Halves xh = Halves(), Halves yh = Halves(),
                   int* ks_deferred = nullptr, int relu = 0, int split_target = 0, float* tk_rows = nullptr,
                   int* tk_count = nullptr, Conv3Launch* launched = nullptr);
// split_target > 0: split-K workgroup target of this launch (0 = the forward default; a larger one is clamped to it, the planned
// split-K scratch).  The input-gradient convs of the backward use CONV3_BWD_SPLITK_TARGET in the fused launch AND when they run
// stand-alone, so both routes produce the same bits
constexpr int CONV3_BWD_SPLITK_TARGET = 128;
// relu != 0: y = max(0, conv + bias) -- the inference path, where BatchNorm is folded into (weights, bias)
// ks_deferred != NULL: a split-K launch leaves its fp32 partials in skws ([ks][M][Cout]) WITHOUT the finishing pass and
// reports ks there (0 = y was written as usual); the caller finishes (bn_train_stats_splitk, fused with the statistics)

size_t conv3_mfma_wgrad_ws_floats(int Cin, int Cout, Geo g);
int conv3_mfma_wgrad(const void* x, int xcs, int Cin, const void* dy, int dycs, int Cout, Geo g, float* dW, float* db,
                     int accumulate, float* ws, size_t ws_floats, hipStream_t s, Halves xh = Halves(), SlabJob* pend = nullptr,
                     int wg_target = 0);
// wg_target > 0: workgroup target of the launch (0 = two per CU).  conv3_mfma_bwd_wg_target = the target the layer's FUSED
// backward launch uses for its weight-gradient half (0: the layer has no fused launch): a stand-alone weight gradient launched
// with it cuts the tiles into the same slabs, i.e. sums in the same order and produces the same bits as the fused route
int conv3_mfma_bwd_wg_target(int Cin, int Cout, int xcs, int dycs, int dxcs, Geo g);
int conv3_mfma_wgrad_slabs(int Cin, int Cout, Geo g, int wg_target);      // slabs conv3_mfma_wgrad / the fused launches write
int conv3_mfma_bwd_ksplit(int Cin, int Cout, Geo g);      // split-K factor of the layer's input-gradient conv when it has the scratch
bool conv3_mfma_big_geo(Geo g);      // 16-wide tiles (levels 0-1 of a 96^3 net) vs the 8-wide deep-level tiling
// pend != NULL (here and below): the final slab sum is NOT launched; its job is returned for the caller to attach to
// the next kernel on the chain (bn_bwd) or to run with slab_job_launch

// deep levels: weight gradient and input-gradient conv of one layer in ONE launch (independent, latency-bound each)
bool conv3_mfma_bwd_fused_ok(int Cin, int Cout, int xcs, int dycs, int dxcs, Geo g);
int conv3_mfma_bwd_fused(const void* x, int xcs, int Cin, const void* dy, int dycs, int Cout, const void* wp_dgrad, void* dx,
                         int dxcs, Geo g, float* dW, float* db, int accumulate, float* wgws, size_t wgws_floats, float* skws,
                         hipStream_t s, SlabJob* pend = nullptr, int* ks_deferred = nullptr);
// ks_deferred != NULL: a split-K input gradient is LEFT as fp32 partials in skws ([ks][M][Cin], *ks_deferred = ks, dx not
// written) for bn_bwd(..., skp, ks) of the layer below to finish inside its reduction; 0 = dx was written as usual
bool conv3_mfma_bwd_fused_persist_ok(int Cin, int Cout, int xcs, int dycs, Geo g);
int conv3_mfma_bwd_fused_persist(const void* x, int xcs, int Cin, const void* dy, int dycs, int Cout, const void* wp_dgrad, void* dx,
                                 int dxcs, Geo g, float* dW, float* db, int accumulate, float* wgws, size_t wgws_floats,
                                 hipStream_t s, Halves xh = Halves(), Halves dxh = Halves(), SlabJob* pend = nullptr);
// first layer (Cin = 1, fp32 input) forward on the matrix cores (K = taps); optional BN partial sums like conv3_mfma_fwd
int conv3_c1_fwd_stat_blocks(Geo g);
int conv3_c1_fwd_mfma(const float* x, const float* w, const float* bias, void* y, int ycs, int Cout, Geo g, float* part,
                      hipStream_t s, const float* wscale = nullptr, int relu = 0);
int conv3_mfma_wgrad_c1(const float* x, const void* dy, int dycs, int Cout, Geo g, float* dW, float* db, int accumulate,
                        float* ws, size_t ws_floats, hipStream_t s, SlabJob* pend = nullptr);

// ---- BatchNorm3d + ReLU + Dropout3d ---------------------------------------------------------- bn.hip
// Reference: nn.BatchNorm3d / nn.ReLU(inplace) / nn.Dropout3d  models/unet.py:12-14,16-18.
// stat buffer layout: float[4][C] = {mean, invstd, a = gamma*invstd, b = beta - mean*a}
size_t bn_ws_floats(int C);
// small_rows != NULL and the tensor is small (deep levels): NO finalize launch -- *small_rows = number of partial rows left
// in ws (<= 128) and the caller hands them to bn_apply_relu_drop (BnSmall), which finishes them in its prologue;
// otherwise *small_rows = 0 and stat / the running statistics are final on return as before
int bn_train_stats(int dtype, const void* y, int ycs, int C, int64_t M, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                   float eps, float* stat, float* ws, hipStream_t s, int* small_rows = nullptr);
bool bn_small_ok(int C, int64_t M, int rows);       // a producer's `rows` partial rows can take the consumer-prologue route
// round 4: the `rows` partial rows of a conv epilogue can be handed to bn_apply_relu_drop(_pool) as a BnSmall (no finalize launch):
// <= 128 rows by the thin kernels' prologue, up to 1024 rows by the wide (1024-thread) kernels; needs C a power of two, 8..256,
// 16-byte aligned channels-last rows, and for the pooled pass the two-threads-per-window shape
bool bn_rows_route_ok(int C, int64_t M, int rows);
struct BnSmall {
    const float* part; int nrows;
    const float* gamma; const float* beta; float* running_mean; float* running_var; int64_t* num_batches_tracked;
    float momentum, eps;
    int64_t M = 0;      // elements per channel: filled in by the launcher, which hands the kernels its own copy
};
// same finalize, fed by conv-epilogue partials part[nblk][2][C]
int bn_train_finalize(const float* part, int nblk, int C, int64_t M, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                      float eps, float* stat, hipStream_t s);
int bn_eval_stats(int C, const float* gamma, const float* beta, const float* running_mean,
                  const float* running_var, float eps, float* stat, hipStream_t s);
// Inference: eval-mode BatchNorm folded into the preceding conv, for ALL layers of a network in ONE launch:
//   scale[c] = gamma/sqrt(running_var + eps)   (multiplied into the filter at pack time)
//   fbias[c] = (conv_bias - running_mean)*scale + beta
struct BnFoldJob { const float* gamma; const float* beta; const float* rm; const float* rv; const float* conv_bias;
                   float* scale; float* fbias; int C; };
constexpr int MAX_FOLD_JOBS = 2 * (2 * 6 + 1);
struct BnFoldJobs { int n; float eps; BnFoldJob j[MAX_FOLD_JOBS]; };
int bn_fold_all(const BnFoldJobs& J, hipStream_t s);
// DEFERRED running-statistics update: a training forward called with momentum < 0 does not touch running_mean / running_var /
// num_batches_tracked; `running_mean` then points at double[2C] where the finalize step publishes (batch mean, unbiased batch
// variance) exactly as it computed them.  bn_deferred_apply performs, later and in the order the caller chooses, the very
// update the forward would have made -- same doubles, same expression, bit-identical buffers.  (Two forwards of one model
// on two streams, train_dann.py:268-272: their updates of the shared buffers must stay in source-then-target order.)
struct BnDeferJob { float* rm; float* rv; int64_t* nbt; const double* side; int C; };
struct BnDeferJobs { int n; float momentum; BnDeferJob j[MAX_FOLD_JOBS]; };
int bn_deferred_apply(const BnDeferJobs& J, hipStream_t s);
// z = drop[n,c] * relu(a*y + b)      (drop == NULL -> 1)
// small != NULL: batch statistics from small->part (prologue); stat[4][C] is then WRITTEN (kept for backward) and the
// running statistics / num_batches_tracked are updated here
int bn_apply_relu_drop(int dtype, const void* y, int ycs, int C, int64_t M, int64_t V, float* stat,
                       const float* drop, void* z, int zcs, hipStream_t s, const BnSmall* small = nullptr);
// the same pass fused with MaxPool3d(2,2): writes z AND pooled = max over each 2x2x2 window of z (even D, H, W only)
int bn_apply_relu_drop_pool(int dtype, const void* y, int ycs, int C, Geo g, float* stat, const float* drop, void* z, int zcs,
                            void* pooled, int pcs, hipStream_t s, const BnSmall* small = nullptr);
// dy = gamma*invstd*(dyh - mean(dyh) - xhat*mean(dyh*xhat)), dyh = dz*drop*[a*y+b > 0]; dgamma, dbeta (+)=
int bn_bwd(int dtype, const void* dz, int dzcs, const void* y, int ycs, int C, int64_t M, int64_t V,
           const float* stat, const float* drop, void* dy, int dycs, float* dgamma, float* dbeta,
           int accumulate, float* ws, hipStream_t s, const SlabJob* extra = nullptr, const float* skp = nullptr, int ks = 0,
           const SlabJob* extra2 = nullptr);
// skp != NULL: dz is still the ks fp32 split-K partials [ks][M][C] of the conv that produced it; the reduction sums and
// rounds them and WRITES dz (the split-K finishing launch of that conv is skipped by the caller)
// extra: a pending slab sum that rides in the reduction kernel's launch (extra blocks)
int slab_job_launch(const SlabJob& q, hipStream_t s);

// split-K conv finish (y = bf16(bias + sum_k skp[k][M][C])) fused with the batch statistics of the stored values
int bn_train_stats_splitk(const float* skp, int ks, const float* bias, void* y, int ycs, int C, int64_t M, const float* gamma,
                          const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                          float momentum, float eps, float* stat, float* ws, hipStream_t s, int* small_rows = nullptr);

// ---- one half of a DoubleConv block, forward: conv -> statistics -> apply (-> pool) ------------------ plan.hip
// The ONE copy of the forward's route decisions (ticket, fused statistics, who finishes the partial rows, the split-K hand-over):
// block_forward of the whole-network plan and the per-operator entry mi3d_conv3_bn_forward both call it.
struct mi3d_conv3_bn_route;            // include/mi3d.h: what was launched, for the per-operator tests
// route class of a conv layer whose activations have dtype dt (build_plan and mi3d_conv3_bn_forward): mfma = bf16 implicit GEMM,
// c1 = first layer on the matrix cores (one input channel, read as fp32), neither = direct fp32 FMA
inline void conv3_layer_class(int dt, int Cin, int Cout, bool& mfma, bool& c1) {
    mfma = dt == MI3D_BF16 && conv3_mfma_supported(Cin, Cout, 16, 16);
    c1 = dt == MI3D_BF16 && Cin == 1 && Cout % 16 == 0;
}
struct ConvBnHalf {
    int Cin, Cout; Geo g;
    int dt;                            // dtype of y / out / pooled
    bool mfma, c1;                     // bf16 implicit GEMM / first layer on the matrix cores / neither: direct fp32 FMA
    const void* in; int ics, idt; Halves ih;
    const float* w; const float* bias; const float* gamma; const float* beta;      // w: torch layout (c1 and direct read it)
    void* wpf; void* wpd;              // mfma: the packed forward image (read); direct: both images are packed here
    void* y; float* stat;
    float* rm; float* rv; int64_t* nbt; float mom, eps;
    int training;                      // 0: running statistics
    bool tk_zeroed;                    // the split-K ticket counters at tkcount are zero
    bool beside;                       // another forward runs beside this one (thin consumers only)
    float* statpart; float* skws; int* tkcount; float* bnws;
    const float* drop;                 // this layer's [N][Cout] scales or NULL
    void* out; int ocs; void* pooled; int pcs;
};
int conv3_bn_half_forward(const ConvBnHalf& a, hipStream_t s, mi3d_conv3_bn_route* route = nullptr);

// ---- one half of a DoubleConv block, inference: conv with BatchNorm folded in, ReLU in the epilogue ------------------ plan.hip
// The ONE copy of the inference forward's per-layer decisions (which kernel, whether the split-K scratch is handed over, the
// direct pack with the scale): block_infer of the whole-network plan and the per-operator entry mi3d_conv3_infer_forward both
// call it.  scale / fbias: what bn_fold_all left (ops.h BnFoldJob); an MFMA layer's packed image already carries the scale.
struct mi3d_conv3_infer_route;         // include/mi3d.h: what was launched, for the per-operator tests
struct ConvBnHalfInfer {
    int Cin, Cout; Geo g;
    int dt;                            // dtype of out
    bool mfma, c1;                     // the layer's route class (conv3_layer_class)
    const void* in; int ics, idt; Halves ih;
    const float* w;                    // torch layout (c1 and direct read it)
    void* wpf;                         // mfma: the packed forward image, scale folded in (read); direct: packed here
    const float* scale; const float* fbias;
    void* out; int ocs;
    float* skws;                       // split-K scratch (conv3_mfma_splitk_floats); handed on only to 16-byte aligned output rows
};
int conv3_bn_half_infer(const ConvBnHalfInfer& a, hipStream_t s, mi3d_conv3_infer_route* route = nullptr);

// ---- one half of a DoubleConv block, backward: BatchNorm backward -> weight gradient + input gradient ---------------- plan.hip
// The weight-gradient slab sums that wait for a launch to ride in.  A launcher that is handed a slot leaves its final slab sum
// there instead of launching it (nblocks > 0: a sum waits).  The rule, once:
//   * a launch that writes the first slab workspace (wgws) takes `first`: older sums read their workspaces before it, with
//     launches of their own;
//   * the transposed conv's backward may take `carry` instead while the decoder conv's sum waits: it writes the SECOND
//     workspace (wgws2) and both sums stay;
//   * the next BatchNorm-backward reduction carries up to two (`riders`, then `rode` behind that launch);
//   * an exchange mark is recorded behind the launch that carried its segment's sums (`rode`), or behind a flush when the
//     segment launched no BatchNorm backward / the call ends (`finish`).
struct Pending {
    SlabJob pend, pend2;
    hipEvent_t mark = nullptr;      // exchange mark waiting for the launch that completes its segment's gradients
    static bool waits(const SlabJob& j) { return j.nblocks > 0; }
    int flush(hipStream_t s) {
        int rc = 0;
        if (waits(pend)) { rc = slab_job_launch(pend, s); pend.nblocks = 0; }
        if (waits(pend2)) { int r2 = slab_job_launch(pend2, s); pend2.nblocks = 0; if (!rc) rc = r2; }
        return rc;
    }
    SlabJob* first(hipStream_t s) {      // where the launcher leaves its own slab sum instead of launching it
        flush(s);
        pend = SlabJob();
        return &pend;
    }
    SlabJob* carry() {      // NULL: nothing to carry across, or the second slot is taken
        if (!waits(pend) || waits(pend2)) return nullptr;
        pend2 = SlabJob();
        return &pend2;
    }
    void riders(const SlabJob*& extra, const SlabJob*& extra2) const {
        extra = waits(pend) ? &pend : (waits(pend2) ? &pend2 : nullptr);
        extra2 = (waits(pend) && waits(pend2)) ? &pend2 : nullptr;
    }
    int rode(hipStream_t s) {            // the sums `riders` handed out are in a launch on s
        pend.nblocks = pend2.nblocks = 0;
        if (mark) { MI3D_HIP(hipEventRecord(mark, s)); mark = nullptr; }
        return 0;
    }
    int finish(hipStream_t s) {
        MI3D_TRY(flush(s));
        return rode(s);
    }
    // two marks on one launch cannot happen (one event per segment); an older mark still waiting means the segment in
    // between launched no BatchNorm backward: complete it now
    int set_mark(hipEvent_t ev, hipStream_t s) {
        if (mark) MI3D_TRY(finish(s));
        mark = ev;
        return 0;
    }
};

// The ONE copy of the backward's per-layer decisions (who carries the pending slab sums, deferred input gradient alone / fused
// persistent / fused / stand-alone pair, where `first` is taken, a split-K dx left as partials): block_backward of the
// whole-network plan and the per-operator entries mi3d_conv3_bn_backward / mi3d_conv3_backward both call it.
struct mi3d_conv3_bn_bwd_route;        // include/mi3d.h: what was launched, for the per-operator tests
struct ConvBnHalfBwd {
    int Cin, Cout; Geo g;
    int dt;                            // dtype of y / dz / dy / dx
    bool mfma, c1;                     // the layer's route class (conv3_layer_class)
    const void* in; int ics, idt; Halves ih;      // the layer's input
    const void* wpd;                   // packed input-gradient image (mfma: bf16 MFMA image, otherwise the direct kernels' floats)
    const void* y; const float* stat; const float* drop;      // saved by the forward; stat NULL: no BatchNorm, dz IS the conv's dy
    const void* dz; int dzcs;          // gradient of the activated output; with dz_skp the reduction WRITES it (bf16 of the sums)
    const float* dz_skp; int dz_ks;    // dz still as split-K partials [ks][M][Cout] fp32 (NULL / 0: dz is stored)
    void* dy; int dycs;                // gradient of the conv output (written; unused without BatchNorm)
    void* dx; int dxcs; Halves dxh;    // input gradient or NULL
    float* dW; float* db; float* dgamma; float* dbeta; int accumulate;
    float* bnws; float* wgws; size_t wgws_floats; float* skws;      // scratch: BatchNorm rows, weight-gradient slabs, split-K partials
    bool allow_partials;               // a split-K dx may stay as fp32 partials [ks][M][Cin] in skws (*dx_ks says so)
    bool deferred;                     // deferred route: the input gradient alone; the caller launches conv3_deferred_wgrad later
    int (*after_bn)(void*); void* after_bn_arg;      // called behind the BatchNorm backward's launches (the plan's fork points) or NULL
};
// dx_ks (may be NULL): split factor of a dx left as partials (0 = dx was written)
int conv3_bn_half_backward(const ConvBnHalfBwd& a, Pending& pending, hipStream_t s, int* dx_ks = nullptr,
                           mi3d_conv3_bn_bwd_route* route = nullptr);
// The weight gradient of a layer on the deferred route: the stand-alone kernel cut into the slabs of the layer's fused launch
// (conv3_mfma_bwd_wg_target; dxcs = 0: the layer has no input gradient), so both routes produce the same bits
int conv3_deferred_wgrad(const void* in, int ics, int Cin, Halves ih, const void* dy, int dycs, int Cout, Geo g, int dxcs, float* dW,
                         float* db, int accumulate, float* ws, size_t ws_floats, hipStream_t s);

// ---- MaxPool3d(2,2) ------------------------------------------------------------------------ pool.hip
// Reference: models/unet.py:40,71.  g = INPUT geometry; odd sides floor like nn.MaxPool3d (last slice in no window).
int maxpool2_fwd(int dtype, const void* z, int zcs, int C, Geo g, void* p, int pcs, hipStream_t s);
// dz = dskip (or 0) + route(dp) to the first max in (d,h,w) scan order
int maxpool2_bwd(int dtype, const void* dp, int dpcs, const void* z, int zcs, const void* dskip, int dskipcs,
                 void* dz, int dzcs, int C, Geo g, hipStream_t s, const float* skp = nullptr, int ks = 0);
// skp / ks: dp has not been written -- it is still the ks fp32 split-K partials [ks][M/8][C] of the conv that produces it

// F.interpolate(x, size=...) nearest, models/unet.py:81-83 (volume sides not divisible by 2^levels).  gi = input
// geometry, go = output geometry; backward is the gather-form adjoint (deterministic)
int nearest_resize_fwd(int dtype, const void* x, int xcs, int C, Geo gi, void* y, int ycs, Geo go, hipStream_t s);
int nearest_resize_bwd(int dtype, const void* gy, int gycs, int C, Geo go, void* gx, int gxcs, Geo gi, hipStream_t s);

// ---- ConvTranspose3d(k=2,s=2) ------------------------------------------------------------ upconv.hip
// Reference: models/unet.py:56-58,79.  Weight torch layout (Cin,Cout,2,2,2).  g = INPUT geometry.
// what a forward / backward launcher of the transposed conv launched (filled in at the branch it took; the fields of
// mi3d_up_route, include/mi3d.h)
struct UpLaunch { int kind = 0, gy = 1, tap_split = 0, wide = 0, strided = 0; };
struct UpBwdLaunch { int kind = 0, ksplit = 0, persistent = 0, slabs = 0, slab_ew = 0, wgrad_blocks = 0, dgrad_blocks = 0; };
size_t upconv2_pack_floats(int Cin, int Cout);
int upconv2_pack(const float* w, int Cin, int Cout, float* wp_fwd, float* wp_bwd, hipStream_t s);
int upconv2_fwd(int dtype, const void* x, int xcs, int Cin, const float* wp_fwd, const float* bias, void* y,
                int ycs, int Cout, Geo g, hipStream_t s, UpLaunch* launched = nullptr);
size_t upconv2_bwd_ws_floats(int Cin, int Cout, Geo g);
int upconv2_bwd(int dtype, const void* x, int xcs, int Cin, const void* gy, int gycs, int Cout,
                const float* wp_bwd, void* dx, int dxcs, float* dW, float* db, int accumulate, float* ws,
                size_t ws_floats, Geo g, hipStream_t s, UpBwdLaunch* launched = nullptr);

// MFMA versions (bf16, Cin % 32 == 0, Cout % 16 == 0)                                   upconv_mfma.hip
bool upconv2_mfma_supported(int Cin, int Cout, int xcs, int ycs);
size_t upconv2_mfma_pack_elems(int Cin, int Cout);           // bf16 elements (fwd + bwd images)
int upconv2_mfma_pack(const float* w, int Cin, int Cout, void* wp, hipStream_t s);
int upconv2_mfma_fwd(const void* x, int xcs, int Cin, const void* wp, const float* bias, void* y, int ycs, int Cout,
                     Geo g, hipStream_t s, UpLaunch* launched = nullptr);
size_t upconv2_mfma_bwd_ws_floats(int Cin, int Cout, Geo g);
int upconv2_mfma_bwd(const void* x, int xcs, int Cin, const void* gy, int gycs, int Cout, const void* wp, void* dx,
                     int dxcs, float* dW, float* db, int accumulate, float* ws, size_t ws_floats, Geo g, hipStream_t s, SlabJob* pend = nullptr,
                     UpBwdLaunch* launched = nullptr);

// ---- one decoder up step: transposed conv into the up half of a concat buffer (-> nearest resize), and its adjoint ---- plan.hip
// The ONE copy of the up step's decisions (temporary + resize where the output geometry is not 2x the input, MFMA or direct
// launcher, which pending slot and which slab workspace the backward takes): up_forward / the decoder segments of the
// whole-network plan and the per-operator entries mi3d_up_forward / mi3d_up_backward / mi3d_upconv2_* all call it.
struct mi3d_up_route;                  // include/mi3d.h: what was launched, for the per-operator tests
struct UpHalf {
    int Cin, Cout; Geo g;              // g: INPUT geometry
    int dt; bool mfma;                 // bf16 MFMA kernels / the direct fp32-FMA kernels
    const void* in; int ics;
    const float* w; const float* bias; // w: torch layout (the direct route packs it here, in front of its launch)
    void* wp; float* wpb;              // mfma: the packed image (read); direct: forward image / backward image (written)
    void* up; int ucs; Geo go;         // the up half of the concat buffer, its channel stride and geometry
    void* tmp;                         // [2D][2H][2W][Cout] temporary, needed where go is not (2D, 2H, 2W)
};
int up_half_forward(const UpHalf& a, hipStream_t s, mi3d_up_route* route = nullptr);
struct UpHalfBwd {
    int Cin, Cout; Geo g;              // g: INPUT geometry of the transposed conv
    int dt; bool mfma;
    const void* in; int ics;
    const void* wp; const float* wpb;  // mfma: the packed image; direct: the backward image
    const void* gup; int gucs; Geo go; // gradient of the up half of the concat buffer
    void* tmp;                         // [2D][2H][2W][Cout] temporary of the resize adjoint
    void* dx; int dxcs;                // input gradient or NULL
    float* dW; float* db; int accumulate;
    float* wgws; float* wgws2; size_t wgws_floats;      // first / second slab workspace (wgws2 NULL: no carry)
    bool leave;                        // the MFMA route leaves its slab sum in `pending` (the plan) instead of launching it
};
int up_half_backward(const UpHalfBwd& a, Pending& pending, hipStream_t s, mi3d_up_route* route = nullptr);

// ---- final 1x1x1 conv, losses, metrics ------------------------------------------------ head_loss.hip
// Reference: nn.Conv3d(16,4,1) models/unet.py:62,87 ; utils/metrics.py:14-40,65-129,137-190.
int conv1_fwd(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, float* logits,
              int Cout, int N, int64_t V, hipStream_t s);
size_t conv1_bwd_ws_floats(int Cin, int Cout);
int conv1_bwd(int dtype, const void* z, int zcs, int Cin, const float* w, const float* dlogits, int Cout,
              void* dz, int dzcs, float* dW, float* db, int accumulate, float* ws, int N, int64_t V,
              hipStream_t s, SlabJob* pend = nullptr);

struct LossCfg {
    float w_ce;       // weight of mean cross-entropy
    int region_kind;  // 0 none, 1 soft-Dice (combined_loss), 2 Tversky
    float w_reg;      // weight of mean_{c>=1} region term
    float alpha, beta, eps;
    float w_kd;       // weight of T^2 * mean_{n,c,v} KL(teacher || student)   (0 = no distillation)
    float temp;
    int mask = 0;     // the *_masked entries: voxels labelled `ignore` are left out of CE, the region sums and the metric counts
    int ignore = 0;   // (contract: include/mi3d.h, "Ignore value"); mask = 0 is the unmasked kernels, bit for bit
};
// cfg with the ignore value of a *_masked entry; false: the value does not fit int32 (the entry answers MI3D_EINVAL)
inline bool loss_cfg_ignore(LossCfg& k, int64_t ignore_index) {
    if (ignore_index < INT32_MIN || ignore_index > INT32_MAX) return false;
    k.mask = 1;
    k.ignore = (int)ignore_index;
    return true;
}
enum { MI3D_MAX_CLASSES = 8 };
size_t seg_loss_ws_bytes(int C);
// loss_out: device float[1]; coef: device float[2*MI3D_MAX_CLASSES + 4] consumed by seg_loss_bwd
int seg_loss_fwd(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int64_t V,
                 LossCfg cfg, float* loss_out, float* coef, void* ws, hipStream_t s,
                 int D = 0, float* metrics_out = nullptr, void* metrics_ws = nullptr);
int seg_loss_bwd(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int64_t V,
                 LossCfg cfg, const float* coef, const float* grad_out, float* dlogits, hipStream_t s);
// head + loss of the training step in one pass each way (logits / dlogits never written); `*_ok` says whether the shape has
// the fused kernels (bf16, Cin % 16 == 0, <= 4 classes; backward: Cin == 16); teacher: (N,C,V) float logits, needed iff cfg.w_kd != 0
bool head_loss_ok(int dtype, const void* z, int zcs, int Cin, int C, LossCfg cfg);
bool head_loss_bwd_ok(int dtype, const void* z, int zcs, int Cin, int C, LossCfg cfg, const void* dz, int dzcs);
int head_loss_fwd(const void* z, int zcs, int Cin, const float* w, const float* bias, const int64_t* labels, const float* teacher,
                  int N, int C, int64_t V, LossCfg cfg, float* loss_out, float* coef, void* ws, hipStream_t s, int D, float* metrics_out,
                  void* metrics_ws, float* logits_opt);
int head_loss_bwd(const void* z, int zcs, int Cin, const float* w, const float* bias, const int64_t* labels, const float* teacher, int C,
                  LossCfg cfg, const float* coef, const float* grad_out, void* dz, int dzcs, float* dW, float* db, int accumulate,
                  float* ws, int N, int64_t V, hipStream_t s, SlabJob* pend = nullptr);
// pseudo-labels of a prediction for the masked loss (pseudo_labels.hip; contract: include/mi3d.h mi3d_pseudo_labels);
// thresholds: C host floats, table: device int64 (N, C + 1)
int pseudo_labels(const uint8_t* labels, const float* conf, int N, int64_t V, int C, const float* thresholds, int64_t ignore_index,
                  int64_t* target, int64_t* table, hipStream_t s);
size_t seg_metrics_ws_bytes(int C);
// out: device float[3] = {iou, dice, acc}; Q1 loop bound = first spatial dim D (utils/metrics.py:74,101)
int seg_metrics(const float* logits, const int64_t* labels, int N, int C, int D, int64_t V, float* out, void* ws,
                hipStream_t s, int64_t* counts_out = nullptr);
// head + argmax in one pass (inference: the logits are never written): labels[n][v] = first maximum of conv1_fwd's logits of that
// voxel, uint8; with target (N,V) int64 also counts (N, 3*Cout + 1) int64 per sample, in seg_metrics' counts_out order.
// ws: head_labels_ws_bytes(N, Cout), needed only with a target
size_t head_labels_ws_bytes(int N, int Cout);
int head_labels(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, int Cout, int N, int64_t V,
                uint8_t* labels, const int64_t* target, int64_t* counts, void* ws, hipStream_t s);
// one view of a flip / model ensemble: votes (N,Cout,D,H,W) float += softmax of that head at the voxel mirrored by `flip`; the
// last view ends in the argmax of the total (contract: include/mi3d.h mi3d_head_votes).  ws: head_labels_ws_bytes(N, Cout)
int head_votes(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, int Cout, int N, int D, int H, int W,
               int flip, int view, int views, int flags, float* votes, uint8_t* labels, float* confidence, const int64_t* target,
               int64_t* counts, void* ws, hipStream_t s);
// sliding-window inference: N window samples (d, h, wd) of that head, each weighted by the tables' product and added into
// acc (Cout,D,H,W) at its origin, in sample order; then the finishing pass over acc (contract: include/mi3d.h
// mi3d_head_votes_window, mi3d_votes_finish).  flips (N) and origins (N x 3) are host arrays.  ws: head_labels_ws_bytes(1, Cout)
int head_votes_window(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, int Cout, int N, int d, int h, int wd,
                      const int* flips, const float* gd, const float* gh, const float* gw, const int* origins, float* acc, int D, int H,
                      int W, hipStream_t s);
int votes_finish(float* acc, int Cout, int D, int H, int W, const float* nd, const float* nh, const float* nw, int views, int flags,
                 uint8_t* labels, float* confidence, const int64_t* target, int64_t* counts, void* ws, hipStream_t s);

// ---- spatial augmentation: flip + in-plane rotation of one (C, D, H, W) sample ------------- spatial.hip
// Reference: random_flip / random_rotate, utils/dataloader.py:207-221.  Contract and arithmetic: include/mi3d.h mi3d_plane_affine.
int plane_affine(const float* img_in, float* img_out, const int64_t* lab_in, int64_t* lab_out, int C, int D, int H, int W, int ax0,
                 int ax1, const double* matrix, const double* offset, int flip_mask, hipStream_t s);

// ---- spatial augmentation: 3-D affine + elastic warp of one (C, D, H, W) sample ---------------- warp.hip
// Reference: the commented-out RandAffined / Rand3DElasticd block, utils/dataloader.py:227-248.  Contract and arithmetic:
// include/mi3d.h mi3d_elastic_field / mi3d_warp3 / mi3d_warp3_at.  taps, matrix, translate: HOST arrays; start: NULL or three DEVICE ints.
size_t elastic_ws_bytes(int D, int H, int W);
int elastic_field(float* field, int D, int H, int W, uint64_t seed, const double* taps, int radius, void* ws, size_t ws_bytes,
                  hipStream_t s);
int warp3(const float* img_in, float* img_out, const int64_t* lab_in, int64_t* lab_out, int C, int D, int H, int W, int Do, int Ho,
          int Wo, const double* matrix, const double* translate, const float* field, double magnitude, int image_padding,
          int label_padding, const int32_t* start, hipStream_t s);

// ---- misc ---------------------------------------------------------------------------------- misc.hip
int ncdhw_to_ndhwc(int dtype, const float* src, void* dst, int dcs, int C, int N, int64_t V, hipStream_t s);
int ndhwc_to_ncdhw(int dtype, const void* src, int scs, float* dst, int C, int N, int64_t V, hipStream_t s);
// torch.mean(x, dim=[2,3,4]) models/unet_dann.py:79 ; backward adds scale*g[n,c]/V to every voxel
int gap_fwd(int dtype, const void* z, int zcs, int C, int N, int64_t V, float* out, hipStream_t s);
int gap_bwd(int dtype, const float* g, float scale, void* dz, int dzcs, int C, int N, int64_t V,
            int accumulate, hipStream_t s);
// nn.Linear (+ optional ReLU and dropout scale) train_dann.py:38-46 ; fp32, small M
int linear_fwd(const float* x, const float* w, const float* b, float* y, int M, int K, int Nout, int relu,
               const float* drop, hipStream_t s);
int linear_bwd(const float* x, const float* w, const float* y, const float* gy, int M, int K, int Nout,
               int relu, const float* drop, float* gx, float* gw, float* gb, int accumulate, float gx_scale,
               float* ws, hipStream_t s);
int softmax_ce_rows(const float* logits, const int64_t* labels, int M, int C, float* loss, float* dlogits,
                    float scale, hipStream_t s);
// fused flat AdamW (torch.optim.AdamW semantics, train_unet.py:378); step_dev: device int64 step counter (incremented)
int adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2,
               float eps, float wd, float grad_scale, int64_t* step_dev, hipStream_t s, int increment = 1);
// Dropout3d channel masks: out[i] = (u_i >= p) ? 1/(1-p) : 0, counter-based RNG; state_dev = {seed, counter}
int dropout_scales(float* out, int64_t n, float p, uint64_t* state_dev, hipStream_t s);
int fill_f32(float* p, int64_t n, float v, hipStream_t s);
int occupy_cus(int wgs, int usec, float* buf, int64_t n, hipStream_t s);     // collective stand-in (bench.py --emulate-comm)
int scale_f32(const float* x, float* y, int64_t n, float a, const float* a_dev, hipStream_t s);   // y = a * (*a_dev|1) * x
int scale_add_f32(float* dst, const float* src, int64_t n, float a, float b, hipStream_t s);  // dst = a*dst + b*src
