// api.hip — extern "C" wrappers (include/mi3d.h) around the per-operator launchers, losses, DANN head,
// optimizer and hipGraph helpers.  The whole-network entry points live in plan.hip.
#include "../../include/mi3d.h"
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "ops.h"
#include "scratch.h"

static_assert(MI3D_LOSS_COEF_FLOATS >= 2 * MI3D_MAX_CLASSES + 4, "coef buffer too small");

// ---- route switches (common.h): one struct, filled from the environment once, changed only through the ABI
namespace {
struct RouteEntry { const char* name; int Mi3dRoutes::*field; };
const RouteEntry ROUTE_TABLE[] = {
#define MI3D_ROUTE_ENTRY(name, dflt) {#name, &Mi3dRoutes::name},
    MI3D_ROUTE_LIST(MI3D_ROUTE_ENTRY)
#undef MI3D_ROUTE_ENTRY
};
constexpr int N_ROUTES = sizeof(ROUTE_TABLE) / sizeof(ROUTE_TABLE[0]);
Mi3dRoutes load_routes() {
    Mi3dRoutes r;
    for (int i = 0; i < N_ROUTES; i++) {
        char env[64] = "MI3D_";
        size_t n = 5;
        for (const char* c = ROUTE_TABLE[i].name; *c && n + 1 < sizeof(env); c++) env[n++] = (*c >= 'a' && *c <= 'z') ? *c - 32 : *c;
        env[n] = 0;
        const char* v = getenv(env);
        if (!v) continue;
        char* end = nullptr;
        long k = strtol(v, &end, 10);
        r.*(ROUTE_TABLE[i].field) = (end != v) ? (int)k : 1;
    }
    return r;
}
Mi3dRoutes& routes_mut() {
    static Mi3dRoutes r = load_routes();      // thread-safe one-time initialisation
    return r;
}
}  // namespace
const Mi3dRoutes& mi3d_routes() { return routes_mut(); }

static inline LossCfg to_cfg(const mi3d_loss_cfg* c) {
    LossCfg k;
    k.w_ce = c->w_ce; k.region_kind = c->region_kind; k.w_reg = c->w_reg; k.alpha = c->alpha; k.beta = c->beta;
    k.eps = c->eps; k.w_kd = c->w_kd; k.temp = c->temperature > 0.f ? c->temperature : 1.f;
    return k;
}
// the loss configuration of a *_masked entry (ops.h loss_cfg_ignore)
#define MI3D_MASKED_CFG(k, cfg, ignore_index, what) \
    LossCfg k = to_cfg(cfg);                        \
    MI3D_CHECK_ARG(loss_cfg_ignore(k, ignore_index), what ": ignore_index %lld does not fit int32", (long long)(ignore_index))

static inline bool use_mfma(int in_dtype, int out_dtype, int Cin, int Cout, int xcs, int ycs) {
    return in_dtype == MI3D_BF16 && out_dtype == MI3D_BF16 && conv3_mfma_supported(Cin, Cout, xcs, ycs);
}

extern "C" {

size_t mi3d_seg_loss_workspace_bytes(int C) { return seg_loss_ws_bytes(C); }
int mi3d_seg_loss_forward(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int64_t V,
                          const mi3d_loss_cfg* cfg, float* loss_out, float* coef, void* workspace, void* stream) {
    MI3D_CHECK_ARG(logits && labels && cfg && loss_out && coef && workspace, "mi3d_seg_loss_forward: null pointer");
    return seg_loss_fwd(logits, labels, teacher, N, C, V, to_cfg(cfg), loss_out, coef, workspace, (hipStream_t)stream);
}
int mi3d_seg_loss_metrics_forward(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int D,
                                  int64_t V, const mi3d_loss_cfg* cfg, float* loss_out, float* coef, float* metrics_out,
                                  void* loss_workspace, void* metrics_workspace, void* stream) {
    MI3D_CHECK_ARG(logits && labels && cfg && loss_out && coef && metrics_out && loss_workspace && metrics_workspace,
                   "mi3d_seg_loss_metrics_forward: null pointer");
    return seg_loss_fwd(logits, labels, teacher, N, C, V, to_cfg(cfg), loss_out, coef, loss_workspace, (hipStream_t)stream, D,
                        metrics_out, metrics_workspace);
}
int mi3d_seg_loss_backward(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int64_t V,
                           const mi3d_loss_cfg* cfg, const float* coef, const float* grad_out, float* dlogits,
                           void* stream) {
    MI3D_CHECK_ARG(logits && labels && cfg && coef && dlogits, "mi3d_seg_loss_backward: null pointer");
    return seg_loss_bwd(logits, labels, teacher, N, C, V, to_cfg(cfg), coef, grad_out, dlogits, (hipStream_t)stream);
}
// the masked siblings: the same launchers, the ignore value in the internal configuration (MASK = true instantiations)
int mi3d_seg_loss_forward_masked(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int64_t V,
                                 const mi3d_loss_cfg* cfg, int64_t ignore_index, float* loss_out, float* coef, void* workspace,
                                 void* stream) {
    MI3D_CHECK_ARG(logits && labels && cfg && loss_out && coef && workspace, "mi3d_seg_loss_forward_masked: null pointer");
    MI3D_MASKED_CFG(k, cfg, ignore_index, "mi3d_seg_loss_forward_masked");
    return seg_loss_fwd(logits, labels, teacher, N, C, V, k, loss_out, coef, workspace, (hipStream_t)stream);
}
int mi3d_seg_loss_metrics_forward_masked(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int D,
                                         int64_t V, const mi3d_loss_cfg* cfg, int64_t ignore_index, float* loss_out, float* coef,
                                         float* metrics_out, void* loss_workspace, void* metrics_workspace, void* stream) {
    MI3D_CHECK_ARG(logits && labels && cfg && loss_out && coef && metrics_out && loss_workspace && metrics_workspace,
                   "mi3d_seg_loss_metrics_forward_masked: null pointer");
    MI3D_MASKED_CFG(k, cfg, ignore_index, "mi3d_seg_loss_metrics_forward_masked");
    return seg_loss_fwd(logits, labels, teacher, N, C, V, k, loss_out, coef, loss_workspace, (hipStream_t)stream, D, metrics_out,
                        metrics_workspace);
}
int mi3d_seg_loss_backward_masked(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int64_t V,
                                  const mi3d_loss_cfg* cfg, int64_t ignore_index, const float* coef, const float* grad_out,
                                  float* dlogits, void* stream) {
    MI3D_CHECK_ARG(logits && labels && cfg && coef && dlogits, "mi3d_seg_loss_backward_masked: null pointer");
    MI3D_MASKED_CFG(k, cfg, ignore_index, "mi3d_seg_loss_backward_masked");
    return seg_loss_bwd(logits, labels, teacher, N, C, V, k, coef, grad_out, dlogits, (hipStream_t)stream);
}
int mi3d_pseudo_labels(const uint8_t* labels, const float* confidence, int N, int64_t V, int C, const float* thresholds,
                       int64_t ignore_index, int64_t* target, int64_t* table, void* stream) {
    MI3D_CHECK_ARG(labels && confidence && thresholds && target && table, "mi3d_pseudo_labels: null pointer");
    return pseudo_labels(labels, confidence, N, V, C, thresholds, ignore_index, target, table, (hipStream_t)stream);
}
size_t mi3d_seg_metrics_workspace_bytes(int C) { return seg_metrics_ws_bytes(C); }
int mi3d_seg_metrics(const float* logits, const int64_t* labels, int N, int C, int D, int64_t V, float* out,
                     void* workspace, void* stream) {
    MI3D_CHECK_ARG(logits && labels && out && workspace, "mi3d_seg_metrics: null pointer");
    return seg_metrics(logits, labels, N, C, D, V, out, workspace, (hipStream_t)stream);
}
int mi3d_seg_class_counts(const float* logits, const int64_t* labels, int N, int C, int64_t V, int64_t* counts,
                          void* workspace, void* stream) {
    MI3D_CHECK_ARG(logits && labels && counts && workspace, "mi3d_seg_class_counts: null pointer");
    return seg_metrics(logits, labels, N, C, 0, V, nullptr, workspace, (hipStream_t)stream, counts);
}
size_t mi3d_head_labels_workspace_bytes(int N, int Cout) { return head_labels_ws_bytes(N, Cout); }
int mi3d_head_labels(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, int Cout, int N, int64_t V,
                     uint8_t* labels_out, const int64_t* target, int64_t* counts, void* workspace, void* stream) {
    MI3D_CHECK_ARG(z && w && labels_out, "mi3d_head_labels: null pointer");
    MI3D_CHECK_ARG(dtype == MI3D_F32 || dtype == MI3D_BF16, "mi3d_head_labels: bad dtype %d", dtype);
    return head_labels(dtype, z, zcs, Cin, w, bias, Cout, N, V, labels_out, target, counts, workspace, (hipStream_t)stream);
}
size_t mi3d_head_votes_workspace_bytes(int N, int Cout) { return head_labels_ws_bytes(N, Cout); }
int mi3d_head_votes(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, int Cout, int N, int D, int H, int W,
                    int flip, int view, int views, int flags, float* votes, uint8_t* labels_out, float* confidence,
                    const int64_t* target, int64_t* counts, void* workspace, void* stream) {
    MI3D_CHECK_ARG(z && w, "mi3d_head_votes: null pointer");
    MI3D_CHECK_ARG(dtype == MI3D_F32 || dtype == MI3D_BF16, "mi3d_head_votes: bad dtype %d", dtype);
    return head_votes(dtype, z, zcs, Cin, w, bias, Cout, N, D, H, W, flip, view, views, flags, votes, labels_out, confidence, target,
                      counts, workspace, (hipStream_t)stream);
}
int mi3d_head_votes_window(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, int Cout, int N, int d, int h,
                           int wd, const int* flips, const float* g_d, const float* g_h, const float* g_w, const int* origins, float* acc,
                           int D, int H, int W, void* stream) {
    MI3D_CHECK_ARG(z && w, "mi3d_head_votes_window: null pointer");
    MI3D_CHECK_ARG(dtype == MI3D_F32 || dtype == MI3D_BF16, "mi3d_head_votes_window: bad dtype %d", dtype);
    return head_votes_window(dtype, z, zcs, Cin, w, bias, Cout, N, d, h, wd, flips, g_d, g_h, g_w, origins, acc, D, H, W,
                             (hipStream_t)stream);
}
int mi3d_votes_finish(float* acc, int Cout, int D, int H, int W, const float* n_d, const float* n_h, const float* n_w,
                      int views_per_window, int flags, uint8_t* labels_out, float* confidence, const int64_t* target, int64_t* counts,
                      void* workspace, void* stream) {
    return votes_finish(acc, Cout, D, H, W, n_d, n_h, n_w, views_per_window, flags, labels_out, confidence, target, counts, workspace,
                        (hipStream_t)stream);
}

int mi3d_linear_forward(const float* x, const float* w, const float* b, float* y, int M, int K, int Nout, int relu,
                        const float* drop, void* stream) {
    MI3D_CHECK_ARG(x && w && y && M > 0 && K > 0 && Nout > 0, "mi3d_linear_forward: bad arguments");
    return linear_fwd(x, w, b, y, M, K, Nout, relu, drop, (hipStream_t)stream);
}
int mi3d_linear_backward(const float* x, const float* w, const float* y, const float* gy, int M, int K, int Nout,
                         int relu, const float* drop, float* gx, float* gw, float* gb, int accumulate, float gx_scale,
                         float* workspace, void* stream) {
    MI3D_CHECK_ARG(x && w && y && gy && workspace, "mi3d_linear_backward: null pointer");
    MI3D_CHECK_ARG(M > 0 && K > 0 && Nout > 0, "mi3d_linear_backward: M=%d K=%d Nout=%d must be positive", M, K, Nout);
    return linear_bwd(x, w, y, gy, M, K, Nout, relu, drop, gx, gw, gb, accumulate, gx_scale, workspace, (hipStream_t)stream);
}
int mi3d_softmax_ce_rows(const float* logits, const int64_t* labels, int M, int C, float* loss, float* dlogits,
                         float scale, void* stream) {
    MI3D_CHECK_ARG(logits && labels, "mi3d_softmax_ce_rows: null pointer");
    MI3D_CHECK_ARG(M > 0 && C > 0, "mi3d_softmax_ce_rows: M=%d C=%d must be positive", M, C);
    return softmax_ce_rows(logits, labels, M, C, loss, dlogits, scale, (hipStream_t)stream);
}

int mi3d_scale(const float* x, float* y, int64_t n, float alpha, const float* alpha_dev, void* stream) {
    MI3D_CHECK_ARG(x && y && n >= 0, "mi3d_scale: bad arguments");
    return scale_f32(x, y, n, alpha, alpha_dev, (hipStream_t)stream);
}

int mi3d_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, float grad_scale, int64_t* step_dev, void* stream) {
    MI3D_CHECK_ARG(p && g && m && v && step_dev && n >= 0, "mi3d_adamw_step: bad arguments");
    return adamw_step(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, grad_scale, step_dev, (hipStream_t)stream);
}
int mi3d_adamw_apply(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, float grad_scale, int64_t* step_dev, int increment, void* stream) {
    MI3D_CHECK_ARG(step_dev && (n == 0 || (p && g && m && v)) && n >= 0, "mi3d_adamw_apply: bad arguments");
    return adamw_step(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, grad_scale, step_dev, (hipStream_t)stream, increment);
}
int mi3d_debug_occupy_cus(int workgroups, int microseconds, float* buf, int64_t n, void* stream) {
    return occupy_cus(workgroups, microseconds, buf, n, (hipStream_t)stream);
}
int mi3d_dropout_scales(float* out, int64_t n, float p, uint64_t* state_dev, void* stream) {
    MI3D_CHECK_ARG(out && state_dev && n >= 0 && p >= 0.f && p <= 1.f, "mi3d_dropout_scales: bad arguments");
    return dropout_scales(out, n, p, state_dev, (hipStream_t)stream);
}

// ---- per-operator entry points ------------------------------------------------------------------
}  // extern "C"

// What the per-operator conv entries share: argument checks, the single-job pack launch, and the three workspace layouts: the areas
// one layer touches in the plan's workspace, in the plan's order, in a workspace of its own, sized by the layer's ConvScratch (scratch.h)
namespace {
// x_halves / ocs: the input arrives as planar halves (16-channel blocks) / channel stride of the entry's output-side tensor
int conv_entry_check(const char* fn, int in_dtype, int dtype, int Cin, int Cout, int xcs, bool x_halves, int ocs, Geo g) {
    MI3D_CHECK_ARG((dtype == MI3D_F32 || dtype == MI3D_BF16) && (in_dtype == dtype || (in_dtype == MI3D_F32 && Cin == 1 && xcs == 1)),
                   "%s: bad dtypes %d -> %d", fn, in_dtype, dtype);
    MI3D_CHECK_ARG(Cin >= 1 && Cout >= 1 && Cout <= 256 && xcs >= (x_halves ? 16 : Cin) && ocs >= Cout && g.N >= 1 && g.D >= 1 && g.H >= 1 && g.W >= 1,
                   "%s: bad shape", fn);
    return 0;
}
int workspace_check(const char* fn, const void* workspace, size_t have, size_t need) {
    MI3D_CHECK_ARG(have >= need, "%s: workspace too small: %zu < %zu", fn, have, need);
    MI3D_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
    return 0;
}
inline bool geo_ok(int Cin, int Cout, int N, int D, int H, int W) { return Cin >= 1 && Cout >= 1 && N >= 1 && D >= 1 && H >= 1 && W >= 1; }
// the plan's pack launch with one job.  scale: BatchNorm scale folded into the forward image; zero: ticket counters block 0 clears
int pack_one_conv3(const float* w, int Cin, int Cout, void* wpf, void* wpd, Geo g, hipStream_t s, const float* scale = nullptr, int* zero = nullptr) {
    PackJobs J;
    J.n = 0; J.nblocks = 0;
    if (zero) { J.zero = zero; J.nzero = CONV3_TK_COUNTERS; }
    MI3D_TRY(pack_all_add_conv3(J, w, Cin, Cout, wpf, wpd, g, scale));
    return pack_all_launch(J, s);
}

struct ConvBnWs { size_t statpart, tkcount, bnws, wpf, wpd, skws, total; };       // mi3d_conv3_bn_forward
ConvBnWs conv_bn_ws(const ConvScratch& S, int Cout) {
    ConvBnWs L; Arena A;
    L.statpart = A.take((size_t)S.stat_rows * 2 * Cout * sizeof(float));
    L.tkcount = A.take((size_t)CONV3_TK_COUNTERS * sizeof(int));
    L.bnws = A.take(bn_ws_floats(Cout) * sizeof(float));
    L.wpf = A.take(S.wpf_bytes);
    L.wpd = A.take(S.wpd_bytes);
    L.skws = A.take(S.splitk_fwd_floats * sizeof(float) + 16);
    L.total = A.off;
    return L;
}
struct ConvInferWs { size_t fold, wpf, wpd, skws, total; };                       // mi3d_conv3_infer_forward
ConvInferWs conv_infer_ws(const ConvScratch& S, int Cout) {
    ConvInferWs L; Arena A;
    L.fold = A.take((size_t)2 * Cout * sizeof(float));      // scale, then the folded bias: the plan's stat[0..2C) of an inference call
    L.wpf = A.take(S.wpf_bytes);
    L.wpd = A.take(S.mfma ? S.wpd_bytes : 0);               // the pack launch writes both images; the direct pack only the forward one
    L.skws = A.take(S.splitk_fwd_floats * sizeof(float) + 16);
    L.total = A.off;
    return L;
}
// mi3d_conv3_bn_backward / mi3d_conv3_backward.  S: the kernels the call runs -- the layer's class, or the direct description where
// mi3d_conv3_backward routes a class-MFMA layer down because of the caller's strides
struct ConvBnBwdWs { size_t wpf, wpd, bnws, wgws, wgws_floats, skws, total; };
ConvBnBwdWs conv_bn_bwd_ws(const ConvScratch& S, int Cin, int Cout, Geo g) {
    ConvBnBwdWs L; Arena A;
    L.wpf = A.take(S.wpf_bytes);
    L.wpd = A.take(S.wpd_bytes);
    L.bnws = A.take(bn_ws_floats(Cout) * sizeof(float));
    // a class that runs on the matrix cores may still land on the direct weight gradient at the call: room for the larger of the two.
    // A one-channel layer has always reserved the first-layer kernel's slabs whatever its dtype: dx_offset and the size query keep that
    const ConvScratch Dk = conv3_scratch_direct(Cin, Cout, g), F = conv3_scratch(MI3D_BF16, Cin, Cout, g);
    L.wgws_floats = std::max({S.wgrad_floats, Dk.wgrad_floats, F.c1 ? F.wgrad_floats : (size_t)0});
    L.wgws = A.take(L.wgws_floats * sizeof(float));
    L.skws = A.take(S.splitk_bwd_floats * sizeof(float) + 16);      // the input gradient's split-K partials
    L.total = A.off;
    return L;
}
static_assert(sizeof(mi3d_pending_sum) == sizeof(SlabJob) && alignof(mi3d_pending_sum) == alignof(SlabJob), "mi3d_pending_sum holds a SlabJob");

struct ConvBwdCall {
    int in_dtype, dtype; const void* x; int xcs; Halves xh; int Cin; const float* w; const void* y; const float* stat; const float* drop;
    void* dz; int dzcs; const float* dz_partials; int dz_ks; void* dy; void* dx; int dxcs; Halves dxh; float* dW; float* db;
    float* dgamma; float* dbeta; int accumulate; const mi3d_pending_sum* riders; mi3d_pending_sum* pending_out; int flags;
    mi3d_conv3_bn_bwd_route* route_out; int Cout; Geo g; bool mfma, c1; char* ws;
};
// the plan's pack launch, then conv3_bn_half_backward with a Pending of the caller's riders; the layer's own sum is handed out or launched
int conv_bn_bwd_run(const ConvBwdCall& k, const ConvBnBwdWs& L, hipStream_t s) {
    if (k.mfma) MI3D_TRY(pack_one_conv3(k.w, k.Cin, k.Cout, k.ws + L.wpf, k.ws + L.wpd, k.g, s));
    else if (k.dx) MI3D_TRY(conv3_direct_pack(k.w, k.Cin, k.Cout, (float*)(k.ws + L.wpf), (float*)(k.ws + L.wpd), s));
    Pending pending;
    if (k.riders) {
        memcpy(&pending.pend, &k.riders[0], sizeof(SlabJob));
        memcpy(&pending.pend2, &k.riders[1], sizeof(SlabJob));
        if (!Pending::waits(pending.pend) && Pending::waits(pending.pend2)) { pending.pend = pending.pend2; pending.pend2 = SlabJob(); }
    }
    const bool defer = (k.flags & MI3D_CONV3_BN_BWD_DEFER) != 0, leave = (k.flags & MI3D_CONV3_BN_BWD_LEAVE_PENDING) != 0;
    ConvBnHalfBwd a{k.Cin, k.Cout, k.g, k.dtype, k.mfma, k.c1, k.x, k.xcs, k.in_dtype, k.xh, k.ws + L.wpd, k.y, k.stat, k.drop,
                    k.dz, k.dzcs, k.dz_partials, k.dz_ks, k.dy, k.Cout, k.dx, k.dxcs, k.dxh, k.dW, k.db, k.dgamma, k.dbeta, k.accumulate,
                    (float*)(k.ws + L.bnws), (float*)(k.ws + L.wgws), L.wgws_floats, (float*)(k.ws + L.skws),
                    (k.flags & MI3D_CONV3_BN_BWD_ALLOW_PARTIALS) != 0, defer, nullptr, nullptr};
    MI3D_TRY(conv3_bn_half_backward(a, pending, s, nullptr, k.route_out));
    if (defer)      // what drain_aux of the plan launches on the aux stream, here in order on s
        MI3D_TRY(conv3_deferred_wgrad(k.x, k.xcs, k.Cin, k.xh, k.stat ? k.dy : k.dz, k.stat ? k.Cout : k.dzcs, k.Cout, k.g, k.dx ? k.dxcs : 0,
                                      k.dW, k.db, k.accumulate, (float*)(k.ws + L.wgws), L.wgws_floats, s));
    if (k.pending_out) memset(k.pending_out, 0, sizeof(*k.pending_out));
    if (leave && Pending::waits(pending.pend)) {
        memcpy(k.pending_out, &pending.pend, sizeof(SlabJob));
        pending.pend.nblocks = 0;
    }
    const bool left = leave && k.pending_out && ((const SlabJob*)k.pending_out)->nblocks > 0;
    MI3D_TRY(pending.flush(s));
    if (k.route_out) {
        k.route_out->pending = left ? 1 : 0;
        k.route_out->dx_offset = (int32_t)L.skws;
    }
    return 0;
}
}  // namespace

extern "C" {

size_t mi3d_conv3_workspace_bytes(int Cin, int Cout, int N, int D, int H, int W) {
    // no dtype argument: room for the layer's bf16 class and for the direct kernels, whichever the call runs.  The forward: the two
    // direct images (the MFMA ones are smaller) in front of a slab region
    const Geo g{N, D, H, W};
    const ConvScratch S = conv3_scratch(MI3D_BF16, Cin, Cout, g), Dk = conv3_scratch_direct(Cin, Cout, g);
    const size_t fwd = Dk.wpf_bytes + Dk.wpd_bytes + (std::max(S.wgrad_floats, Dk.wgrad_floats) + 64) * sizeof(float);
    // the backward's areas (mi3d_conv3_backward aligns the workspace itself: + 256)
    const size_t bwd = std::max(conv_bn_bwd_ws(S, Cin, Cout, g).total, conv_bn_bwd_ws(Dk, Cin, Cout, g).total);
    return std::max(fwd, bwd) + 256;
}
int mi3d_conv3_forward(int in_dtype, int out_dtype, const void* x, int xcs, int Cin, const float* w, const float* bias,
                       void* y, int ycs, int Cout, int N, int D, int H, int W, void* workspace, size_t workspace_bytes,
                       void* stream) {
    MI3D_CHECK_ARG(x && w && y && workspace, "mi3d_conv3_forward: null pointer");
    MI3D_CHECK_ARG(workspace_bytes >= mi3d_conv3_workspace_bytes(Cin, Cout, N, D, H, W), "mi3d_conv3_forward: workspace too small");
    float* wpf = (float*)workspace;
    float* wpd = (float*)((char*)workspace + conv3_scratch_direct(Cin, Cout, Geo{N, D, H, W}).wpf_bytes);
    hipStream_t s = (hipStream_t)stream;
    if (use_mfma(in_dtype, out_dtype, Cin, Cout, xcs, ycs)) {       // bf16 implicit GEMM on the matrix cores
        MI3D_TRY(conv3_mfma_pack(w, Cin, Cout, wpf, wpd, Geo{N, D, H, W}, s));
        return conv3_mfma_fwd(x, xcs, Cin, wpf, bias, y, ycs, Cout, Geo{N, D, H, W}, nullptr, nullptr, s);
    }
    MI3D_TRY(conv3_direct_pack(w, Cin, Cout, wpf, wpd, s));
    return conv3_direct_fwd(in_dtype, out_dtype, x, xcs, Cin, wpf, bias, y, ycs, Cout, Geo{N, D, H, W}, s);
}
// The conv half of conv3_bn_half_backward (no BatchNorm, no flags): the kernels the training step runs for this layer.  A layer
// whose strides the MFMA kernels cannot take runs the direct kernels
int mi3d_conv3_backward(int x_dtype, int dy_dtype, const void* x, int xcs, int Cin, const float* w, const void* dy,
                        int dycs, int Cout, void* dx, int dxcs, float* dW, float* db, int accumulate, int N, int D, int H,
                        int W, void* workspace, size_t workspace_bytes, void* stream) {
    MI3D_CHECK_ARG(x && w && dy && workspace, "mi3d_conv3_backward: null pointer");
    MI3D_CHECK_ARG(workspace_bytes >= mi3d_conv3_workspace_bytes(Cin, Cout, N, D, H, W), "mi3d_conv3_backward: workspace too small");
    Geo g{N, D, H, W};
    const ConvScratch S = conv3_scratch(dy_dtype, Cin, Cout, g);
    const bool mfma = S.mfma && x_dtype == MI3D_BF16 && conv3_mfma_supported(Cin, Cout, xcs, dycs) && dycs % 8 == 0 &&
                      (!dx || conv3_mfma_supported(Cout, Cin, dycs, dxcs));
    const bool c1 = S.c1 && x_dtype == MI3D_F32 && xcs == 1 && dycs % 8 == 0 && !dx;
    // strides that rule the MFMA kernels out: the direct kernels' areas (the layout keeps slab room for either weight gradient)
    const ConvBnBwdWs L = conv_bn_bwd_ws(S.mfma && !mfma ? conv3_scratch_direct(Cin, Cout, g) : S, Cin, Cout, g);
    char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    ConvBwdCall k{x_dtype, dy_dtype, x, xcs, Halves(), Cin, w, nullptr, nullptr, nullptr, const_cast<void*>(dy), dycs, nullptr, 0, nullptr,
                  dx, dxcs, Halves(), dW, db, nullptr, nullptr, accumulate, nullptr, nullptr, 0, nullptr, Cout, g, mfma, c1, ws};
    return conv_bn_bwd_run(k, L, (hipStream_t)stream);
}

size_t mi3d_conv3_bn_bwd_workspace_bytes(int in_dtype, int dtype, int Cin, int Cout, int N, int D, int H, int W) {
    const Geo g{N, D, H, W};
    return geo_ok(Cin, Cout, N, D, H, W) ? conv_bn_bwd_ws(conv3_scratch(dtype, Cin, Cout, g), Cin, Cout, g).total : 0;
}
int mi3d_conv3_bn_backward(int in_dtype, int dtype, const void* x, int xcs, int x_split, int64_t x_delta, int Cin, const float* w,
                           const void* y, const float* stat, const float* drop, void* dz, int dzcs, const float* dz_partials,
                           int dz_ks, void* dy, void* dx, int dxcs, int dx_split, int64_t dx_delta, float* dW, float* db,
                           float* dgamma, float* dbeta, int accumulate, const mi3d_pending_sum* riders, mi3d_pending_sum* pending_out,
                           int flags, mi3d_conv3_bn_bwd_route* route_out, int Cout, int N, int D, int H, int W, void* workspace,
                           size_t workspace_bytes, void* stream) {
    const char* fn = "mi3d_conv3_bn_backward";
    MI3D_CHECK_ARG(x && w && dz && workspace, "%s: null pointer", fn);
    MI3D_CHECK_ARG(!stat || (y && dy), "%s: the BatchNorm backward needs y and dy", fn);
    MI3D_CHECK_ARG(stat || (!dz_partials && !riders), "%s: dz partials and riders need the BatchNorm backward", fn);
    const Geo g{N, D, H, W};
    MI3D_TRY(conv_entry_check(fn, in_dtype, dtype, Cin, Cout, xcs, x_delta != 0, dzcs, g));
    MI3D_CHECK_ARG(!dz_partials || dz_ks >= 1, "%s: dz_ks=%d", fn, dz_ks);
    MI3D_CHECK_ARG(!(flags & MI3D_CONV3_BN_BWD_LEAVE_PENDING) || pending_out, "%s: LEAVE_PENDING needs pending_out", fn);
    MI3D_CHECK_ARG(!(flags & MI3D_CONV3_BN_BWD_DEFER) || !(flags & MI3D_CONV3_BN_BWD_LEAVE_PENDING), "%s: DEFER launches its own sum", fn);
    const ConvScratch S = conv3_scratch(dtype, Cin, Cout, g);
    MI3D_CHECK_ARG(!S.mfma || (xcs % 8 == 0 && dzcs % 8 == 0 && (!dx || dxcs % 4 == 0)), "%s: channel strides %d / %d / %d", fn, xcs, dzcs, dxcs);
    MI3D_CHECK_ARG(!S.c1 || (in_dtype == MI3D_F32 && !dx), "%s: the first-layer kernel reads an fp32 image and has no input gradient", fn);
    MI3D_CHECK_ARG(!dx || dxcs >= (dx_delta ? 16 : Cin), "%s: dx stride %d", fn, dxcs);
    MI3D_CHECK_ARG(!(flags & MI3D_CONV3_BN_BWD_DEFER) || (S.mfma && (dW || db)), "%s: only MFMA layers with a weight gradient defer it", fn);
    MI3D_CHECK_ARG((!x_delta && !dx_delta) || (S.mfma && conv3_mfma_halves_ok(Cout, Cin, g)),
                   "%s: planar halves need the full-resolution kernels", fn);
    const ConvBnBwdWs L = conv_bn_bwd_ws(S, Cin, Cout, g);
    MI3D_TRY(workspace_check(fn, workspace, workspace_bytes, L.total));
    ConvBwdCall k{in_dtype, dtype, x, xcs, halves_at(x_split, x_delta), Cin, w, y, stat, drop, dz, dzcs, dz_partials, dz_ks, dy, dx, dxcs,
                  halves_at(dx_split, dx_delta), dW, db, dgamma, dbeta, accumulate, riders, pending_out, flags, route_out, Cout, g, S.mfma, S.c1,
                  (char*)workspace};
    return conv_bn_bwd_run(k, L, (hipStream_t)stream);
}
int mi3d_pending_sum_launch(const mi3d_pending_sum* job, void* stream) {
    MI3D_CHECK_ARG(job, "mi3d_pending_sum_launch: null job");
    SlabJob q;
    memcpy(&q, job, sizeof(q));
    return slab_job_launch(q, (hipStream_t)stream);
}

size_t mi3d_conv3_bn_workspace_bytes(int in_dtype, int dtype, int Cin, int Cout, int N, int D, int H, int W) {
    return geo_ok(Cin, Cout, N, D, H, W) ? conv_bn_ws(conv3_scratch(dtype, Cin, Cout, Geo{N, D, H, W}), Cout).total : 0;
}
int mi3d_conv3_bn_forward(int in_dtype, int dtype, const void* x, int xcs, int Cin, const float* w, const float* bias,
                          const float* gamma, const float* beta, float* running_mean, float* running_var,
                          int64_t* num_batches_tracked, float momentum, float eps, const float* drop, void* y, void* z, int zcs,
                          void* pooled, int pcs, float* stat, int flags, mi3d_conv3_bn_route* route_out, int Cout, int N, int D,
                          int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi3d_conv3_bn_forward";
    MI3D_CHECK_ARG(x && w && bias && gamma && beta && y && z && stat && workspace, "%s: null pointer", fn);
    const Geo g{N, D, H, W};
    MI3D_TRY(conv_entry_check(fn, in_dtype, dtype, Cin, Cout, xcs, false, zcs, g));
    MI3D_CHECK_ARG(!pooled || (D % 2 == 0 && H % 2 == 0 && W % 2 == 0 && pcs >= Cout && (int64_t)N * D * H * W * Cout < (1ll << 31)),
                   "%s: pooled needs even sides and fewer than 2^31 elements", fn);
    const ConvScratch S = conv3_scratch(dtype, Cin, Cout, g);      // the route class as build_plan assigns it
    const ConvBnWs L = conv_bn_ws(S, Cout);
    MI3D_CHECK_ARG(!S.mfma || xcs % 8 == 0, "%s: input channel stride %d", fn, xcs);
    MI3D_CHECK_ARG(!S.c1 || in_dtype == MI3D_F32, "%s: the first-layer kernel reads an fp32 image", fn);
    MI3D_TRY(workspace_check(fn, workspace, workspace_bytes, L.total));
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    if (S.mfma)      // the plan's pack launch: the weight images, and block 0 clears the ticket counters
        MI3D_TRY(pack_one_conv3(w, Cin, Cout, ws + L.wpf, ws + L.wpd, g, s, nullptr,
                                (flags & MI3D_CONV3_BN_KEEP_TICKETS) ? nullptr : (int*)(ws + L.tkcount)));
    ConvBnHalf a{Cin, Cout, g, dtype, S.mfma, S.c1, x, xcs, in_dtype, Halves(), w, bias, gamma, beta, ws + L.wpf, ws + L.wpd,
                 y, stat, running_mean, running_var, num_batches_tracked, momentum, eps, 1, /*tk_zeroed*/ S.mfma, false,
                 (float*)(ws + L.statpart), (float*)(ws + L.skws), (int*)(ws + L.tkcount), (float*)(ws + L.bnws),
                 drop, z, zcs, pooled, pcs};
    MI3D_TRY(conv3_bn_half_forward(a, s, route_out));
    if (route_out) route_out->rows_offset = (int32_t)(route_out->stats == 1 || route_out->stats == 2 ? L.statpart : L.bnws);
    return 0;
}

size_t mi3d_conv3_infer_workspace_bytes(int in_dtype, int dtype, int Cin, int Cout, int N, int D, int H, int W) {
    return geo_ok(Cin, Cout, N, D, H, W) ? conv_infer_ws(conv3_scratch(dtype, Cin, Cout, Geo{N, D, H, W}), Cout).total : 0;
}
int mi3d_conv3_infer_forward(int in_dtype, int dtype, const void* x, int xcs, int x_split, int64_t x_delta, int Cin,
                             const float* w, const float* bias, const float* gamma, const float* beta,
                             const float* running_mean, const float* running_var, float eps, void* z, int zcs, float* fold_out,
                             mi3d_conv3_infer_route* route_out, int Cout, int N, int D, int H, int W, void* workspace,
                             size_t workspace_bytes, void* stream) {
    const char* fn = "mi3d_conv3_infer_forward";
    MI3D_CHECK_ARG(x && w && gamma && beta && running_mean && running_var && z && workspace, "%s: null pointer", fn);
    const Geo g{N, D, H, W};
    MI3D_TRY(conv_entry_check(fn, in_dtype, dtype, Cin, Cout, xcs, x_delta != 0, zcs, g));
    const ConvScratch S = conv3_scratch(dtype, Cin, Cout, g);
    const ConvInferWs L = conv_infer_ws(S, Cout);
    MI3D_CHECK_ARG(!S.mfma || (xcs % 8 == 0 && zcs % 4 == 0 && ((uintptr_t)x % 16) == 0), "%s: channel strides %d / %d", fn, xcs, zcs);
    MI3D_CHECK_ARG(!S.c1 || (in_dtype == MI3D_F32 && zcs % 4 == 0), "%s: the first-layer kernel reads an fp32 image", fn);
    MI3D_CHECK_ARG(!(S.mfma || S.c1) || ((uintptr_t)z % 8) == 0, "%s: misaligned output", fn);
    MI3D_CHECK_ARG(!S.mfma || ((uintptr_t)w % 16) == 0, "%s: the weight tensor must be 16-byte aligned", fn);
    MI3D_CHECK_ARG(!x_delta || (S.mfma && conv3_mfma_halves_ok(Cin, Cout, g)), "%s: planar halves need the full-resolution kernels", fn);
    MI3D_TRY(workspace_check(fn, workspace, workspace_bytes, L.total));
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    float* scale = (float*)(ws + L.fold);
    BnFoldJobs F;      // launch 1 of mi3d_unet_infer with one job
    F.n = 1; F.eps = eps;
    F.j[0] = BnFoldJob{gamma, beta, running_mean, running_var, bias, scale, scale + Cout, Cout};
    MI3D_TRY(bn_fold_all(F, s));
    if (S.mfma)      // launch 2: the weight images, BatchNorm scale multiplied into the forward one
        MI3D_TRY(pack_one_conv3(w, Cin, Cout, ws + L.wpf, ws + L.wpd, g, s, scale));
    ConvBnHalfInfer a{Cin, Cout, g, dtype, S.mfma, S.c1, x, xcs, in_dtype, halves_at(x_split, x_delta), w, ws + L.wpf, scale, scale + Cout, z, zcs,
                      (float*)(ws + L.skws)};
    MI3D_TRY(conv3_bn_half_infer(a, s, route_out));
    if (fold_out) MI3D_HIP(hipMemcpyAsync(fold_out, scale, (size_t)2 * Cout * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

size_t mi3d_bn_workspace_bytes(int C) { return bn_ws_floats(C) * sizeof(float); }
int mi3d_bn_relu_drop_forward(int dtype, const void* y, int ycs, int C, int64_t M, int64_t V, const float* gamma,
                              const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                              float momentum, float eps, int training, const float* drop, void* z, int zcs, float* stat,
                              void* workspace, void* stream) {
    MI3D_CHECK_ARG(y && gamma && beta && z && stat && workspace, "mi3d_bn_relu_drop_forward: null pointer");
    hipStream_t s = (hipStream_t)stream;
    int small_rows = 0;
    if (training)
        MI3D_TRY(bn_train_stats(dtype, y, ycs, C, M, gamma, beta, running_mean, running_var, num_batches_tracked, momentum,
                                eps, stat, (float*)workspace, s, &small_rows));
    else {
        MI3D_CHECK_ARG(running_mean && running_var, "eval-mode BN needs running statistics");
        MI3D_TRY(bn_eval_stats(C, gamma, beta, running_mean, running_var, eps, stat, s));
    }
    BnSmall sm{(const float*)workspace, small_rows, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps};
    return bn_apply_relu_drop(dtype, y, ycs, C, M, V, stat, drop, z, zcs, s, small_rows > 0 ? &sm : nullptr);
}
int mi3d_bn_relu_drop_backward(int dtype, const void* dz, int dzcs, const void* y, int ycs, int C, int64_t M, int64_t V,
                               const float* stat, const float* drop, void* dy, int dycs, float* dgamma, float* dbeta,
                               int accumulate, void* workspace, void* stream) {
    MI3D_CHECK_ARG(dz && y && stat && dy && workspace, "mi3d_bn_relu_drop_backward: null pointer");
    return bn_bwd(dtype, dz, dzcs, y, ycs, C, M, V, stat, drop, dy, dycs, dgamma, dbeta, accumulate, (float*)workspace,
                  (hipStream_t)stream);
}
int mi3d_bn_relu_drop_pool_forward(int dtype, const void* y, int ycs, int C, int N, int D, int H, int W, const float* gamma,
                                   const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                   float momentum, float eps, const float* drop, void* z, int zcs, void* pooled, int pcs,
                                   float* stat, void* workspace, void* stream) {
    MI3D_CHECK_ARG(y && gamma && beta && z && pooled && stat && workspace, "mi3d_bn_relu_drop_pool_forward: null pointer");
    hipStream_t s = (hipStream_t)stream;
    Geo g{N, D, H, W};
    int small_rows = 0;
    MI3D_TRY(bn_train_stats(dtype, y, ycs, C, g.M(), gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps,
                            stat, (float*)workspace, s, &small_rows));
    BnSmall sm{(const float*)workspace, small_rows, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps};
    return bn_apply_relu_drop_pool(dtype, y, ycs, C, g, stat, drop, z, zcs, pooled, pcs, s, small_rows > 0 ? &sm : nullptr);
}
size_t mi3d_conv1_workspace_bytes(int Cin, int Cout) { return conv1_bwd_ws_floats(Cin, Cout) * sizeof(float); }
int mi3d_conv1_forward(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, float* logits, int Cout,
                       int N, int64_t V, void* stream) {
    MI3D_CHECK_ARG(z && w && logits, "mi3d_conv1_forward: null pointer");
    MI3D_CHECK_ARG(dtype == MI3D_F32 || dtype == MI3D_BF16, "mi3d_conv1_forward: bad dtype %d", dtype);
    return conv1_fwd(dtype, z, zcs, Cin, w, bias, logits, Cout, N, V, (hipStream_t)stream);
}
int mi3d_head_loss_supported(int dtype, int Cin, int C, const mi3d_loss_cfg* cfg) {
    return cfg && head_loss_bwd_ok(dtype, nullptr, Cin, Cin, C, to_cfg(cfg), nullptr, Cin) ? 1 : 0;
}
int mi3d_head_loss_forward(const void* z, int zcs, int Cin, const float* w, const float* bias, const int64_t* labels,
                           const float* teacher, int N, int C, int D, int64_t V, const mi3d_loss_cfg* cfg, float* loss_out, float* coef,
                           float* metrics_out, void* loss_workspace, void* metrics_workspace, float* logits_opt, void* stream) {
    MI3D_CHECK_ARG(z && w && labels && cfg && loss_out && coef && loss_workspace, "mi3d_head_loss_forward: null pointer");
    return head_loss_fwd(z, zcs, Cin, w, bias, labels, teacher, N, C, V, to_cfg(cfg), loss_out, coef, loss_workspace, (hipStream_t)stream,
                         D, metrics_out, metrics_workspace, logits_opt);
}
int mi3d_head_loss_backward(const void* z, int zcs, int Cin, const float* w, const float* bias, const int64_t* labels,
                            const float* teacher, int N, int C, int64_t V, const mi3d_loss_cfg* cfg, const float* coef,
                            const float* grad_scale, void* dz, int dzcs, float* dW, float* db, int accumulate, void* workspace,
                            size_t workspace_bytes, void* stream) {
    MI3D_CHECK_ARG(z && w && labels && cfg && coef && dz && workspace, "mi3d_head_loss_backward: null pointer");
    MI3D_CHECK_ARG(workspace_bytes >= mi3d_conv1_workspace_bytes(Cin, C), "mi3d_head_loss_backward: workspace too small");
    return head_loss_bwd(z, zcs, Cin, w, bias, labels, teacher, C, to_cfg(cfg), coef, grad_scale, dz, dzcs, dW, db, accumulate,
                         (float*)workspace, N, V, (hipStream_t)stream);
}
int mi3d_head_loss_forward_masked(const void* z, int zcs, int Cin, const float* w, const float* bias, const int64_t* labels,
                                  const float* teacher, int N, int C, int D, int64_t V, const mi3d_loss_cfg* cfg, int64_t ignore_index,
                                  float* loss_out, float* coef, float* metrics_out, void* loss_workspace, void* metrics_workspace,
                                  float* logits_opt, void* stream) {
    MI3D_CHECK_ARG(z && w && labels && cfg && loss_out && coef && loss_workspace, "mi3d_head_loss_forward_masked: null pointer");
    MI3D_MASKED_CFG(k, cfg, ignore_index, "mi3d_head_loss_forward_masked");
    return head_loss_fwd(z, zcs, Cin, w, bias, labels, teacher, N, C, V, k, loss_out, coef, loss_workspace, (hipStream_t)stream, D,
                         metrics_out, metrics_workspace, logits_opt);
}
int mi3d_head_loss_backward_masked(const void* z, int zcs, int Cin, const float* w, const float* bias, const int64_t* labels,
                                   const float* teacher, int N, int C, int64_t V, const mi3d_loss_cfg* cfg, int64_t ignore_index,
                                   const float* coef, const float* grad_scale, void* dz, int dzcs, float* dW, float* db, int accumulate,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    MI3D_CHECK_ARG(z && w && labels && cfg && coef && dz && workspace, "mi3d_head_loss_backward_masked: null pointer");
    MI3D_CHECK_ARG(workspace_bytes >= mi3d_conv1_workspace_bytes(Cin, C), "mi3d_head_loss_backward_masked: workspace too small");
    MI3D_MASKED_CFG(k, cfg, ignore_index, "mi3d_head_loss_backward_masked");
    return head_loss_bwd(z, zcs, Cin, w, bias, labels, teacher, C, k, coef, grad_scale, dz, dzcs, dW, db, accumulate, (float*)workspace, N,
                         V, (hipStream_t)stream);
}
int mi3d_conv1_backward(int dtype, const void* z, int zcs, int Cin, const float* w, const float* dlogits, int Cout, void* dz,
                        int dzcs, float* dW, float* db, int accumulate, int N, int64_t V, void* workspace,
                        size_t workspace_bytes, void* stream) {
    MI3D_CHECK_ARG(z && w && dlogits && dz && workspace, "mi3d_conv1_backward: null pointer");
    MI3D_CHECK_ARG(dtype == MI3D_F32 || dtype == MI3D_BF16, "mi3d_conv1_backward: bad dtype %d", dtype);
    MI3D_CHECK_ARG(workspace_bytes >= mi3d_conv1_workspace_bytes(Cin, Cout), "mi3d_conv1_backward: workspace too small");
    return conv1_bwd(dtype, z, zcs, Cin, w, dlogits, Cout, dz, dzcs, dW, db, accumulate, (float*)workspace, N, V,
                     (hipStream_t)stream);
}
int mi3d_maxpool2_forward(int dtype, const void* z, int zcs, int C, int N, int D, int H, int W, void* p, int pcs,
                          void* stream) {
    MI3D_CHECK_ARG(z && p, "mi3d_maxpool2_forward: null pointer");
    return maxpool2_fwd(dtype, z, zcs, C, Geo{N, D, H, W}, p, pcs, (hipStream_t)stream);
}
int mi3d_maxpool2_backward(int dtype, const void* dp, int dpcs, const void* z, int zcs, const void* dskip, int dskipcs,
                           void* dz, int dzcs, int C, int N, int D, int H, int W, void* stream) {
    MI3D_CHECK_ARG(dp && z && dz, "mi3d_maxpool2_backward: null pointer");
    return maxpool2_bwd(dtype, dp, dpcs, z, zcs, dskip, dskipcs, dz, dzcs, C, Geo{N, D, H, W}, (hipStream_t)stream);
}
int mi3d_maxpool2_backward_partials(int dtype, const float* dp_partials, int ks, const void* z, int zcs, const void* dskip,
                                    int dskipcs, void* dz, int dzcs, int C, int N, int D, int H, int W, void* stream) {
    MI3D_CHECK_ARG(dp_partials && ks >= 1 && z && dz, "mi3d_maxpool2_backward_partials: null pointer or ks < 1");
    // the kernels read dp only without partials; its stride still takes part in the choice of kernel (the plan passes the pooled tensor's C)
    return maxpool2_bwd(dtype, dp_partials, C, z, zcs, dskip, dskipcs, dz, dzcs, C, Geo{N, D, H, W}, (hipStream_t)stream, dp_partials, ks);
}
}  // extern "C"

// mi3d_up_forward / mi3d_up_backward: the route class of a decoder up step and its scratch areas in a workspace of its own
namespace {
struct UpWs { size_t wp, wp_bytes, tmp, tmp_bytes, wgws, wgws2, wg_floats, total; };
// The plan knows a level's route when it lays the level out and reserves the class's images and slabs.  An entry learns its route
// from the caller's strides at the call, and its size queries from less still (mi3d_upconv2_workspace_bytes has no dtype): it
// reserves the direct images, which are never smaller than the MFMA ones, and the larger of the two slab sizes, for either route
UpWs up_ws(int dtype, int Cin, int Cout, Geo g) {
    const UpScratch S = upconv2_scratch(MI3D_BF16, Cin, Cout, g);
    UpWs L; Arena A;
    L.wp_bytes = S.direct_pack_bytes;
    L.wp = A.take(L.wp_bytes);
    L.tmp_bytes = (size_t)g.M() * 8 * Cout * (dtype == MI3D_BF16 ? 2 : 4);
    L.tmp = A.take(L.tmp_bytes);
    L.wg_floats = std::max(S.wgrad_floats, S.direct_wgrad_floats);
    L.wgws = A.take(L.wg_floats * sizeof(float));
    L.wgws2 = A.take(L.wg_floats * sizeof(float));
    L.total = A.off;
    return L;
}
// the route of a call: the MFMA kernels where dtype and the caller's strides allow them
inline bool up_mfma_route(int dtype, int Cin, int Cout, int xcs, int ycs) { return dtype == MI3D_BF16 && upconv2_mfma_supported(Cin, Cout, xcs, ycs); }
// the direct kernels' two weight images inside the packed-weights area
inline float* up_wpb(void* wp, int Cin, int Cout) { return (float*)wp + (size_t)cdiv(Cout, 8) * Cin * 64; }
inline bool up_args_ok(int dtype, int Cin, int Cout, int N, int D, int H, int W, int Do, int Ho, int Wo) {
    return (dtype == MI3D_F32 || dtype == MI3D_BF16) && Cin >= 1 && Cout >= 1 && N >= 1 && D >= 1 && H >= 1 && W >= 1 && Do >= 1 &&
           Ho >= 1 && Wo >= 1;
}
}  // namespace

extern "C" {

size_t mi3d_upconv2_workspace_bytes(int Cin, int Cout, int N, int D, int H, int W) {
    const UpWs L = up_ws(MI3D_F32, Cin, Cout, Geo{N, D, H, W});      // the two areas the wrappers use, back to back
    return L.wp_bytes + L.wg_floats * sizeof(float);
}
// thin wrappers: the up step without a resize, the weight images at the start of the workspace and one slab region behind them
int mi3d_upconv2_forward(int dtype, const void* x, int xcs, int Cin, const float* w, const float* bias, void* y, int ycs,
                         int Cout, int N, int D, int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    MI3D_CHECK_ARG(x && w && y && workspace, "mi3d_upconv2_forward: null pointer");
    MI3D_CHECK_ARG(workspace_bytes >= mi3d_upconv2_workspace_bytes(Cin, Cout, N, D, H, W), "mi3d_upconv2_forward: workspace too small");
    const bool mfma = up_mfma_route(dtype, Cin, Cout, xcs, ycs);
    if (mfma) MI3D_TRY(upconv2_mfma_pack(w, Cin, Cout, workspace, (hipStream_t)stream));
    UpHalf a{Cin, Cout, Geo{N, D, H, W}, dtype, mfma, x, xcs, w, bias, workspace, up_wpb(workspace, Cin, Cout), y, ycs,
             Geo{N, 2 * D, 2 * H, 2 * W}, nullptr};
    return up_half_forward(a, (hipStream_t)stream);
}
int mi3d_upconv2_backward(int dtype, const void* x, int xcs, int Cin, const float* w, const void* gy, int gycs, int Cout,
                          void* dx, int dxcs, float* dW, float* db, int accumulate, int N, int D, int H, int W,
                          void* workspace, size_t workspace_bytes, void* stream) {
    MI3D_CHECK_ARG(x && w && gy && workspace, "mi3d_upconv2_backward: null pointer");
    MI3D_CHECK_ARG(workspace_bytes >= mi3d_upconv2_workspace_bytes(Cin, Cout, N, D, H, W), "mi3d_upconv2_backward: workspace too small");
    const Geo g{N, D, H, W};
    const UpWs L = up_ws(dtype, Cin, Cout, g);
    hipStream_t s = (hipStream_t)stream;
    float* wb = up_wpb(workspace, Cin, Cout);
    const bool mfma = up_mfma_route(dtype, Cin, Cout, xcs, gycs) && (!dx || dxcs % 4 == 0);
    if (mfma) MI3D_TRY(upconv2_mfma_pack(w, Cin, Cout, workspace, s));
    else MI3D_TRY(upconv2_pack(w, Cin, Cout, (float*)workspace, wb, s));
    Pending pending;
    UpHalfBwd a{Cin, Cout, g, dtype, mfma, x, xcs, workspace, wb, gy, gycs, Geo{N, 2 * D, 2 * H, 2 * W}, nullptr, dx, dxcs, dW, db,
                accumulate, (float*)((char*)workspace + L.wp_bytes), nullptr, L.wg_floats, false};
    return up_half_backward(a, pending, s);
}

size_t mi3d_up_workspace_bytes(int dtype, int Cin, int Cout, int N, int D, int H, int W) {
    if (!up_args_ok(dtype, Cin, Cout, N, D, H, W, 1, 1, 1)) return 0;
    return up_ws(dtype, Cin, Cout, Geo{N, D, H, W}).total;
}
size_t mi3d_up_workspace_region(int dtype, int Cin, int Cout, int N, int D, int H, int W, int which, size_t* bytes_out) {
    if (!up_args_ok(dtype, Cin, Cout, N, D, H, W, 1, 1, 1) || which < 0 || which > 3) { if (bytes_out) *bytes_out = 0; return 0; }
    const UpWs L = up_ws(dtype, Cin, Cout, Geo{N, D, H, W});
    const size_t off[4] = {L.wp, L.tmp, L.wgws, L.wgws2}, len[4] = {L.wp_bytes, L.tmp_bytes, L.wg_floats * sizeof(float), L.wg_floats * sizeof(float)};
    if (bytes_out) *bytes_out = len[which];
    return off[which];
}
int mi3d_up_forward(int dtype, const void* x, int xcs, int Cin, const float* w, const float* bias, void* up, int ucs, int Cout,
                    int N, int D, int H, int W, int Do, int Ho, int Wo, mi3d_up_route* route_out, void* workspace,
                    size_t workspace_bytes, void* stream) {
    const char* fn = "mi3d_up_forward";
    MI3D_CHECK_ARG(x && w && up && workspace, "%s: null pointer", fn);
    MI3D_CHECK_ARG(up_args_ok(dtype, Cin, Cout, N, D, H, W, Do, Ho, Wo) && xcs >= Cin && ucs >= Cout, "%s: bad shape or dtype", fn);
    const Geo g{N, D, H, W}, go{N, Do, Ho, Wo};
    const UpWs L = up_ws(dtype, Cin, Cout, g);
    MI3D_TRY(workspace_check(fn, workspace, workspace_bytes, L.total));
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const bool rs = Do != 2 * D || Ho != 2 * H || Wo != 2 * W;
    const bool mfma = up_mfma_route(dtype, Cin, Cout, xcs, rs ? Cout : ucs);
    if (mfma) MI3D_TRY(upconv2_mfma_pack(w, Cin, Cout, ws + L.wp, s));
    UpHalf a{Cin, Cout, g, dtype, mfma, x, xcs, w, bias, ws + L.wp, up_wpb(ws + L.wp, Cin, Cout), up, ucs, go, ws + L.tmp};
    return up_half_forward(a, s, route_out);
}
int mi3d_up_backward(int dtype, const void* x, int xcs, int Cin, const float* w, const void* gup, int gucs, int Cout, void* dx,
                     int dxcs, float* dW, float* db, int accumulate, int N, int D, int H, int W, int Do, int Ho, int Wo, int flags,
                     mi3d_pending_sum* pending_out, mi3d_up_route* route_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi3d_up_backward";
    MI3D_CHECK_ARG(x && w && gup && workspace, "%s: null pointer", fn);
    MI3D_CHECK_ARG(up_args_ok(dtype, Cin, Cout, N, D, H, W, Do, Ho, Wo) && xcs >= Cin && gucs >= Cout && (!dx || dxcs >= Cin),
                   "%s: bad shape or dtype", fn);
    const bool leave = (flags & MI3D_UP_BWD_LEAVE_PENDING) != 0, second = (flags & MI3D_UP_BWD_SECOND_WORKSPACE) != 0;
    MI3D_CHECK_ARG(!leave || pending_out, "%s: LEAVE_PENDING needs pending_out", fn);
    const Geo g{N, D, H, W}, go{N, Do, Ho, Wo};
    const UpWs L = up_ws(dtype, Cin, Cout, g);
    MI3D_TRY(workspace_check(fn, workspace, workspace_bytes, L.total));
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const bool rs = Do != 2 * D || Ho != 2 * H || Wo != 2 * W;
    const bool mfma = up_mfma_route(dtype, Cin, Cout, xcs, rs ? Cout : gucs) && (!dx || dxcs % 4 == 0);
    MI3D_CHECK_ARG(!second || (mfma && !mi3d_routes().no_upbwd_carry), "%s: only the MFMA route with the carry has a second slab workspace", fn);
    float* wb = up_wpb(ws + L.wp, Cin, Cout);
    if (mfma) MI3D_TRY(upconv2_mfma_pack(w, Cin, Cout, ws + L.wp, s));
    else MI3D_TRY(upconv2_pack(w, Cin, Cout, (float*)(ws + L.wp), wb, s));
    // SECOND_WORKSPACE: the plan's situation -- a sum waits in the first slot (it reads the first slab region); the stand-in is never launched
    Pending pending;
    if (second) pending.pend.nblocks = 1;
    UpHalfBwd a{Cin, Cout, g, dtype, mfma, x, xcs, ws + L.wp, wb, gup, gucs, go, ws + L.tmp, dx, dxcs, dW, db, accumulate,
                (float*)(ws + L.wgws), second ? (float*)(ws + L.wgws2) : nullptr, L.wg_floats, leave};
    MI3D_TRY(up_half_backward(a, pending, s, route_out));
    if (second) pending.pend.nblocks = 0;
    if (pending_out) memset(pending_out, 0, sizeof(*pending_out));
    SlabJob& mine = second ? pending.pend2 : pending.pend;
    if (leave && Pending::waits(mine)) { memcpy(pending_out, &mine, sizeof(SlabJob)); mine.nblocks = 0; }
    return pending.flush(s);
}
int mi3d_nearest_resize_forward(int dtype, const void* x, int xcs, int C, int N, int Di, int Hi, int Wi, void* y, int ycs, int Do,
                                int Ho, int Wo, void* stream) {
    MI3D_CHECK_ARG(x && y, "mi3d_nearest_resize_forward: null pointer");
    MI3D_CHECK_ARG(up_args_ok(dtype, C, C, N, Di, Hi, Wi, Do, Ho, Wo) && xcs >= C && ycs >= C, "mi3d_nearest_resize_forward: bad shape or dtype");
    return nearest_resize_fwd(dtype, x, xcs, C, Geo{N, Di, Hi, Wi}, y, ycs, Geo{N, Do, Ho, Wo}, (hipStream_t)stream);
}
int mi3d_nearest_resize_backward(int dtype, const void* gy, int gycs, int C, int N, int Do, int Ho, int Wo, void* gx, int gxcs,
                                 int Di, int Hi, int Wi, void* stream) {
    MI3D_CHECK_ARG(gy && gx, "mi3d_nearest_resize_backward: null pointer");
    MI3D_CHECK_ARG(up_args_ok(dtype, C, C, N, Di, Hi, Wi, Do, Ho, Wo) && gycs >= C && gxcs >= C, "mi3d_nearest_resize_backward: bad shape or dtype");
    return nearest_resize_bwd(dtype, gy, gycs, C, Geo{N, Do, Ho, Wo}, gx, gxcs, Geo{N, Di, Hi, Wi}, (hipStream_t)stream);
}
int mi3d_ncdhw_to_ndhwc(int dtype, const float* src, void* dst, int dcs, int C, int N, int64_t V, void* stream) {
    MI3D_CHECK_ARG(src && dst, "mi3d_ncdhw_to_ndhwc: null pointer");
    return ncdhw_to_ndhwc(dtype, src, dst, dcs, C, N, V, (hipStream_t)stream);
}
int mi3d_ndhwc_to_ncdhw(int dtype, const void* src, int scs, float* dst, int C, int N, int64_t V, void* stream) {
    MI3D_CHECK_ARG(src && dst, "mi3d_ndhwc_to_ncdhw: null pointer");
    return ndhwc_to_ncdhw(dtype, src, scs, dst, C, N, V, (hipStream_t)stream);
}

int mi3d_debug_set_route(const char* name, int value) {
    MI3D_CHECK_ARG(name, "mi3d_debug_set_route: null name");
    for (int i = 0; i < N_ROUTES; i++)
        if (!strcmp(name, ROUTE_TABLE[i].name)) { routes_mut().*(ROUTE_TABLE[i].field) = value; return 0; }
    MI3D_CHECK_ARG(false, "mi3d_debug_set_route: unknown route '%s'", name);
}
int mi3d_debug_get_route(const char* name, int* value_out) {
    MI3D_CHECK_ARG(name && value_out, "mi3d_debug_get_route: null argument");
    for (int i = 0; i < N_ROUTES; i++)
        if (!strcmp(name, ROUTE_TABLE[i].name)) { *value_out = routes_mut().*(ROUTE_TABLE[i].field); return 0; }
    MI3D_CHECK_ARG(false, "mi3d_debug_get_route: unknown route '%s'", name);
}
int mi3d_debug_route_count(void) { return N_ROUTES; }
const char* mi3d_debug_route_name(int i) { return (i >= 0 && i < N_ROUTES) ? ROUTE_TABLE[i].name : nullptr; }

int mi3d_event_create(void** event_out) {
    MI3D_CHECK_ARG(event_out, "mi3d_event_create: null output");
    hipEvent_t e;
    // no system-scope fence on record: by default hipEventRecord writes the caches back for the HOST's benefit, which costs the
    // (measured neutral on this runtime, 2.229 vs 2.237 ms on the exchange path).  These events only order streams of ONE device;
    // the producing kernel's own end-of-kernel release covers that.
    MI3D_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence));
    *event_out = (void*)e;
    return 0;
}
int mi3d_stream_create(int priority_class, void** stream_out) {
    MI3D_CHECK_ARG(stream_out && priority_class >= -1 && priority_class <= 1, "mi3d_stream_create: bad arguments");
    int least = 0, greatest = 0;      // numerically: least = lowest priority (largest value), greatest = highest
    MI3D_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    int prio = priority_class < 0 ? greatest : priority_class > 0 ? least : (least + greatest) / 2;
    hipStream_t s;
    MI3D_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio));
    *stream_out = (void*)s;
    return 0;
}
int mi3d_stream_destroy(void* stream) {
    if (stream) MI3D_HIP(hipStreamDestroy((hipStream_t)stream));
    return 0;
}
int mi3d_timing_event_create(void** event_out) {
    MI3D_CHECK_ARG(event_out, "mi3d_timing_event_create: null output");
    hipEvent_t e;
    MI3D_HIP(hipEventCreate(&e));
    *event_out = (void*)e;
    return 0;
}
int mi3d_event_elapsed_ms(void* start_event, void* stop_event, float* ms_out) {
    MI3D_CHECK_ARG(start_event && stop_event && ms_out, "mi3d_event_elapsed_ms: null argument");
    MI3D_HIP(hipEventSynchronize((hipEvent_t)stop_event));
    MI3D_HIP(hipEventElapsedTime(ms_out, (hipEvent_t)start_event, (hipEvent_t)stop_event));
    return 0;
}
int mi3d_event_destroy(void* event) {
    if (event) MI3D_HIP(hipEventDestroy((hipEvent_t)event));
    return 0;
}

// ---- hipGraph helpers ---------------------------------------------------------------------------
int mi3d_graph_begin(void* stream) {
    MI3D_HIP(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
    return 0;
}
int mi3d_graph_end(void* stream, void** graph_exec_out) {
    MI3D_CHECK_ARG(graph_exec_out, "mi3d_graph_end: null output");
    hipGraph_t graph = nullptr;
    MI3D_HIP(hipStreamEndCapture((hipStream_t)stream, &graph));
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    MI3D_HIP(e);
    *graph_exec_out = (void*)exec;
    return 0;
}
int mi3d_graph_launch(void* graph_exec, void* stream) {
    MI3D_CHECK_ARG(graph_exec, "mi3d_graph_launch: null graph");
    MI3D_HIP(hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream));
    return 0;
}
int mi3d_graph_destroy(void* graph_exec) {
    if (graph_exec) MI3D_HIP(hipGraphExecDestroy((hipGraphExec_t)graph_exec));
    return 0;
}

}  // extern "C"
