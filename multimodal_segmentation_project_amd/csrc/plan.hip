// plan.hip — whole-network execution plan for UNet3D: workspace layout + forward / backward kernel sequences.
// One C call launches the entire forward (or a range of backward segments) on the caller's stream; nothing
// here touches Python, allocates, or synchronises, so a step is hipGraph-capturable end to end.
//
// Reference: models/unet.py:34-90 (UNet3D), models/unet_dann.py:65-98 (GAP branch).
// Data layout in HBM (all inside the caller-owned workspace, channels-last, dtype T):
//   per DoubleConv half : y (raw conv output, kept for BN backward), stat[4][C]
//   per block           : z1 (activated first half)
//   per level l         : cat[l]  [N,V_l,2C_l]  = [ encoder output | upconv output ]   (torch.cat is free)
//                         pool[l] [N,V_l/8,C_l]
//   gradients           : gz[l], gcat[l], gp[l] per level + two max-size scratch tensors
#include "../../include/mi3d.h"
#include <stdlib.h>
#include <algorithm>

#include "ops.h"
#include "scratch.h"

// One half of a DoubleConv block, forward (ops.h ConvBnHalf): conv -> BatchNorm statistics -> apply (-> MaxPool3d).  Every route
// decision of the forward is made here and only here.  a.pooled != NULL (second half of an encoder block on an even volume): the
// apply pass also writes MaxPool3d(2,2) of its output.  route: what was launched.
int conv3_bn_half_forward(const ConvBnHalf& a, hipStream_t s, mi3d_conv3_bn_route* route) {
    const Geo g = a.g;
    const int training = a.training;
    bool fused_stats = false;
    int ksd = 0;
    Conv3Launch ln;
    bool tk = false;
    if (a.mfma) {
        // training: a split-K launch leaves its finishing pass to the statistics kernel (ksd = split factor).  (Deep levels
        // WITHOUT split-K -- conv with fused partial sums -> apply, two launches instead of three -- measured +0.10 ms in
        // round 2: the 8-16-chunk K loops on 32-216 workgroups cost more than the launch they save; that route is gone.)
        // round 4: a split-K launch of a training forward finishes itself behind a per-tile ticket (y, BatchNorm partial rows)
        tk = training && a.tk_zeroed && conv3_mfma_ticket_ok(a.Cin, a.Cout, g);
        MI3D_TRY(conv3_mfma_fwd(a.in, a.ics, a.Cin, a.wpf, a.bias, a.y, a.Cout, a.Cout, g,
                                training ? a.statpart : nullptr, a.skws, s, a.ih, Halves(),
                                training ? &ksd : nullptr, 0, 0, tk ? a.statpart : nullptr,
                                tk ? a.tkcount : nullptr, &ln));
        fused_stats = training && (tk || conv3_mfma_fuses_stats(a.Cin, a.Cout, g));
    } else if (a.c1) {
        // BN partial sums fused like the other convs
        MI3D_TRY(conv3_c1_fwd_mfma((const float*)a.in, a.w, a.bias, a.y, a.Cout, a.Cout, g,
                                   training ? a.statpart : nullptr, s));
        fused_stats = training != 0;
        ln.kind = 1;
    } else {
        MI3D_TRY(conv3_direct_pack(a.w, a.Cin, a.Cout, (float*)a.wpf, (float*)a.wpd, s));
        MI3D_TRY(conv3_direct_fwd(a.idt, a.dt, a.in, a.ics, a.Cin, (const float*)a.wpf, a.bias, a.y, a.Cout,
                                  a.Cout, g, s));
    }
    int small_rows = 0;      // deep levels: the statistics' few partial rows are finished by the apply kernel (no finalize launch)
    const float* rows_at = a.bnws;
    int stats_code = 0, rows = 0;
    if (fused_stats) {
        // round 4: the apply pass finishes the conv epilogue's partial rows itself (bn.hip, wide consumer); the pooled pass only
        // in its two-threads-per-window form
        rows = conv3_scratch(a.dt, a.Cin, a.Cout, g).stat_rows;
        const bool pool_pass = a.pooled != nullptr;
        if (a.dt == MI3D_BF16 && bn_rows_route_ok(a.Cout, g.M(), rows) && !(pool_pass && mi3d_routes().no_pool_pair) &&
            !(a.beside && !bn_small_ok(a.Cout, g.M(), rows))) {
            small_rows = rows;
            rows_at = a.statpart;
            stats_code = 1;
        } else {
            MI3D_TRY(bn_train_finalize(a.statpart, rows, a.Cout, g.M(), a.gamma, a.beta, a.rm, a.rv, a.nbt, a.mom, a.eps, a.stat, s));
            stats_code = 2;
        }
    } else if (training && ksd > 0) {
        MI3D_TRY(bn_train_stats_splitk(a.skws, ksd, a.bias, a.y, a.Cout, a.Cout, g.M(), a.gamma, a.beta, a.rm, a.rv, a.nbt, a.mom,
                                       a.eps, a.stat, a.bnws, s, &small_rows));
        stats_code = 3;
        rows = small_rows;
    } else if (training) {
        MI3D_TRY(bn_train_stats(a.dt, a.y, a.Cout, a.Cout, g.M(), a.gamma, a.beta, a.rm, a.rv, a.nbt, a.mom, a.eps, a.stat,
                                a.bnws, s, &small_rows));
        rows = small_rows;
    } else {
        MI3D_CHECK_ARG(a.rm && a.rv, "eval-mode forward needs running statistics");
        MI3D_TRY(bn_eval_stats(a.Cout, a.gamma, a.beta, a.rm, a.rv, a.eps, a.stat, s));
    }
    BnSmall sm{rows_at, small_rows, a.gamma, a.beta, a.rm, a.rv, a.nbt, a.mom, a.eps};
    const float* drop = training ? a.drop : nullptr;
    if (a.pooled)
        MI3D_TRY(bn_apply_relu_drop_pool(a.dt, a.y, a.Cout, a.Cout, g, a.stat, drop, a.out, a.ocs, a.pooled, a.pcs, s,
                                         small_rows > 0 ? &sm : nullptr));
    else
        MI3D_TRY(bn_apply_relu_drop(a.dt, a.y, a.Cout, a.Cout, g.M(), g.V(), a.stat, drop, a.out, a.ocs, s,
                                    small_rows > 0 ? &sm : nullptr));
    if (route) {
        route->conv = ln.kind;
        route->ksplit = ln.ks;
        route->ticket = tk ? 1 : 0;
        route->stats = stats_code;
        route->rows = rows;
        route->rows_offset = 0;      // relative to a workspace only the caller knows: mi3d_conv3_bn_forward fills it in
    }
    return 0;
}

// One half of a DoubleConv block, inference (ops.h ConvBnHalfInfer): BatchNorm (running statistics) folded into the conv (scale in
// the filter, bias replaced), ReLU in the conv epilogue, output written straight to where the activated tensor lives.  Every
// per-layer decision of the inference forward is made here and only here.  route: what was launched.
int conv3_bn_half_infer(const ConvBnHalfInfer& a, hipStream_t s, mi3d_conv3_infer_route* route) {
    Conv3Launch ln;
    if (a.mfma) {
        // the stand-alone split-K finish stores 16 bytes per thread: no scratch (a single pass) for any other output
        float* skws = (a.ocs % 8 == 0 && ((uintptr_t)a.out % 16) == 0) ? a.skws : nullptr;
        MI3D_TRY(conv3_mfma_fwd(a.in, a.ics, a.Cin, a.wpf, a.fbias, a.out, a.ocs, a.Cout, a.g, nullptr, skws, s, a.ih, Halves(),
                                nullptr, 1, 0, nullptr, nullptr, &ln));
    } else if (a.c1) {
        MI3D_TRY(conv3_c1_fwd_mfma((const float*)a.in, a.w, a.fbias, a.out, a.ocs, a.Cout, a.g, nullptr, s, a.scale, 1));
        ln.kind = 1;
    } else {
        MI3D_TRY(conv3_direct_pack(a.w, a.Cin, a.Cout, (float*)a.wpf, nullptr, s, a.scale));
        MI3D_TRY(conv3_direct_fwd(a.idt, a.dt, a.in, a.ics, a.Cin, (const float*)a.wpf, a.fbias, a.out, a.ocs, a.Cout, a.g, s, 1));
    }
    if (route) {
        route->conv = ln.kind;
        route->ksplit = ln.ks;
    }
    return 0;
}

int conv3_deferred_wgrad(const void* in, int ics, int Cin, Halves ih, const void* dy, int dycs, int Cout, Geo g, int dxcs, float* dW,
                         float* db, int accumulate, float* ws, size_t ws_floats, hipStream_t s) {
    return conv3_mfma_wgrad(in, ics, Cin, dy, dycs, Cout, g, dW, db, accumulate, ws, ws_floats, s, ih, nullptr,
                            conv3_mfma_bwd_wg_target(Cin, Cout, ics, dycs, dxcs > 0 ? dxcs : 8, g));
}

// One half of a DoubleConv block, backward (ops.h ConvBnHalfBwd).  Every per-layer decision of the backward is made here and only
// here, in the order of the data-gradient chain: the pending slab sums ride in the BatchNorm-backward reduction, then ONE of
//   deferred      the input-gradient conv alone (the caller launches conv3_deferred_wgrad elsewhere, later)
//   persistent    weight gradient + input gradient in one launch on the full-resolution bodies
//   fused         the same on the generic tilings (16-wide or 8-wide tile; the 8-wide one may split K)
//   stand-alone   the weight gradient (MFMA, first layer, or direct), then the input-gradient conv
// A launch that writes the slab workspace takes pending.first (older sums are flushed before it).
int conv3_bn_half_backward(const ConvBnHalfBwd& a, Pending& pending, hipStream_t s, int* dx_ks, mi3d_conv3_bn_bwd_route* route) {
    const Geo g = a.g;
    const bool wg = a.dW || a.db;
    if (dx_ks) *dx_ks = 0;
    MI3D_CHECK_ARG(a.stat || !a.dz_skp, "conv3_bn_half_backward: split-K partials of dz need the BatchNorm backward to finish them");
    const void* dyb = a.stat ? a.dy : a.dz;
    const int dycs = a.stat ? a.dycs : a.dzcs;
    void* const dx = a.dx;
    const int dxs = a.dxcs;
    mi3d_conv3_bn_bwd_route r{};
    int dgrad_ks = 1;
    // the layer's input gradient as a launch of its own.  ksd != NULL: a split-K result may stay as partials (see below)
    auto dgrad = [&](int* ksd) {
        if (!a.mfma) return conv3_direct_fwd(a.dt, a.dt, dyb, dycs, a.Cout, (const float*)a.wpd, nullptr, dx, dxs, a.Cin, g, s);
        Conv3Launch ln;
        int rc = conv3_mfma_fwd(dyb, dycs, a.Cout, a.wpd, nullptr, dx, dxs, a.Cin, g, nullptr, (dxs % 8 == 0) ? a.skws : nullptr,
                                s, Halves(), a.dxh, ksd, 0, CONV3_BWD_SPLITK_TARGET, nullptr, nullptr, &ln);
        dgrad_ks = ln.ks;
        return rc;
    };
    // half 1's input gradient feeds straight into half 0's BatchNorm-backward reduction, half 0's into the MaxPool3d backward of
    // the next segment: a split-K result stays as partials and that launch finishes it (one launch less on the chain).  The launch
    // reports its split factor in ksd (0 = dx was written as usual); the caller files it for whoever reads the partials
    int ksd = 0;
    int* const ksp = a.allow_partials && dx && dxs % 8 == 0 && !mi3d_routes().no_defer_tail ? &ksd : nullptr;
    if (a.stat) {
        const SlabJob *extra, *extra2;
        pending.riders(extra, extra2);
        r.riders = (extra ? 1 : 0) + (extra2 ? 1 : 0);
        MI3D_TRY(bn_bwd(a.dt, a.dz, a.dzcs, a.y, a.Cout, a.Cout, g.M(), g.V(), a.stat, a.drop, a.dy, a.dycs, a.dgamma, a.dbeta,
                        a.accumulate, a.bnws, s, extra, a.dz_skp, a.dz_skp ? a.dz_ks : 0, extra2));
        MI3D_TRY(pending.rode(s));
        r.bn = bn_small_ok(a.Cout, g.M(), 1) ? 2 : 1;
        r.dz_ks = a.dz_skp ? a.dz_ks : 0;
    }
    if (a.after_bn) MI3D_TRY(a.after_bn(a.after_bn_arg));
    auto report = [&](int conv) {
        if (dx_ks) *dx_ks = ksd;
        if (!route) return 0;
        r.conv = conv;
        r.dgrad_ks = dx ? dgrad_ks : 0;
        r.dx_ks = ksd;
        const SlabJob& j = pending.pend;
        if (Pending::waits(j)) { r.slabs = j.nslab; r.slab_layout = j.layout; r.slab_ew = j.ew; r.pending = 1; }
        *route = r;
        return 0;
    };
    // a sum that no SlabJob describes (the fused launch's tail kernel, the deferred weight gradient): the same partition and layout rule
    auto report_slabs = [&](int wg_target) {
        const int64_t nW = (int64_t)a.Cout * a.Cin * 27, slab_sz = nW + a.Cout;
        const SlabJob j = slab_job_make((a.dW && slab_sz >= (800 << 10)) ? 2 : 1, nullptr, conv3_mfma_wgrad_slabs(a.Cin, a.Cout, g, wg_target),
                                        slab_sz, nW, a.dW, a.db, a.Cin, a.Cout, a.accumulate);
        r.slabs = j.nslab; r.slab_layout = j.layout; r.slab_ew = j.ew;
    };
    if (a.deferred) {
        // the chain runs the input-gradient conv alone; the weight gradient goes to the aux stream.  Its slab partition is the fused
        // launch's (conv3_deferred_wgrad), the input gradient uses the fused launch's split-K factor and the same K order: both routes
        // produce the same bits
        MI3D_CHECK_ARG(a.mfma && wg, "conv3_bn_half_backward: only MFMA layers with a weight gradient can defer it");
        if (dx) MI3D_TRY(dgrad(ksp));
        report_slabs(conv3_mfma_bwd_wg_target(a.Cin, a.Cout, a.ics, dycs, dx ? dxs : 8, g));
        return report(6);
    }
    if (a.mfma && dx && wg && conv3_mfma_bwd_fused_persist_ok(a.Cin, a.Cout, a.ics, dycs, g)) {
        MI3D_TRY(conv3_mfma_bwd_fused_persist(a.in, a.ics, a.Cin, dyb, dycs, a.Cout, a.wpd, dx, dxs, g, a.dW, a.db, a.accumulate,
                                              a.wgws, a.wgws_floats, s, a.ih, a.dxh, pending.first(s)));
        return report(2);
    }
    if (a.mfma && dx && wg && !a.ih.on() && !a.dxh.on() && conv3_mfma_bwd_fused_ok(a.Cin, a.Cout, a.ics, dycs, dxs, g)) {
        MI3D_TRY(conv3_mfma_bwd_fused(a.in, a.ics, a.Cin, dyb, dycs, a.Cout, a.wpd, dx, dxs, g, a.dW, a.db, a.accumulate, a.wgws,
                                      a.wgws_floats, a.skws, s, pending.first(s), ksp));
        dgrad_ks = conv3_mfma_bwd_ksplit(a.Cin, a.Cout, g);
        if (!Pending::waits(pending.pend)) report_slabs(conv3_mfma_bwd_wg_target(a.Cin, a.Cout, a.ics, dycs, dxs, g));
        return report(conv3_mfma_big_geo(g) ? 3 : 4);
    }
    if (wg) {
        SlabJob* ps = pending.first(s);
        if (a.mfma)
            MI3D_TRY(conv3_mfma_wgrad(a.in, a.ics, a.Cin, dyb, dycs, a.Cout, g, a.dW, a.db, a.accumulate, a.wgws, a.wgws_floats, s, a.ih, ps));
        else if (a.c1)
            MI3D_TRY(conv3_mfma_wgrad_c1((const float*)a.in, dyb, dycs, a.Cout, g, a.dW, a.db, a.accumulate, a.wgws, a.wgws_floats, s, ps));
        else
            MI3D_TRY(conv3_direct_wgrad(a.idt, a.dt, a.in, a.ics, a.Cin, dyb, dycs, a.Cout, g, a.dW, a.db, a.accumulate, a.wgws,
                                        a.wgws_floats, s));
    }
    if (dx) MI3D_TRY(dgrad(nullptr));
    return report(a.mfma ? 5 : a.c1 ? 1 : 0);
}

// One decoder up step, forward (ops.h UpHalf): the transposed conv into the up half of the concat buffer; where that half's
// geometry is not twice the input's (an odd side somewhere above, models/unet.py:81-83) it goes through the temporary and the
// nearest resize.  route: what was launched.
static inline bool up_resized(Geo g, Geo go) { return go.D != 2 * g.D || go.H != 2 * g.H || go.W != 2 * g.W; }
int up_half_forward(const UpHalf& a, hipStream_t s, mi3d_up_route* route) {
    const Geo g2{a.g.N, 2 * a.g.D, 2 * a.g.H, 2 * a.g.W};
    const bool rs = up_resized(a.g, a.go);
    MI3D_CHECK_ARG(!rs || a.tmp, "up_half_forward: the resize needs the temporary");
    void* dst = rs ? a.tmp : a.up;
    const int dcs = rs ? a.Cout : a.ucs;
    UpLaunch L;
    if (a.mfma) {
        MI3D_TRY(upconv2_mfma_fwd(a.in, a.ics, a.Cin, a.wp, a.bias, dst, dcs, a.Cout, a.g, s, &L));
    } else {
        MI3D_TRY(upconv2_pack(a.w, a.Cin, a.Cout, (float*)a.wp, a.wpb, s));
        MI3D_TRY(upconv2_fwd(a.dt, a.in, a.ics, a.Cin, (const float*)a.wp, a.bias, dst, dcs, a.Cout, a.g, s, &L));
    }
    if (rs) MI3D_TRY(nearest_resize_fwd(a.dt, dst, dcs, a.Cout, g2, a.up, a.ucs, a.go, s));
    if (route) {
        *route = mi3d_up_route{};
        route->kind = L.kind; route->gy = L.gy; route->tap_split = L.tap_split; route->wide = L.wide; route->strided = L.strided;
        route->resized = rs ? 1 : 0;
    }
    return 0;
}

// One decoder up step, backward (ops.h UpHalfBwd): the resize adjoint where the forward resized, then the transposed conv's
// backward.  The slab-sum slots, once: while the decoder conv's sum waits in `pending` (it reads the first slab workspace) the
// MFMA route takes `carry` and writes its slabs to the SECOND workspace, so both sums ride in the next BatchNorm-backward
// reduction (not under no_upbwd_carry / without a second workspace); otherwise it takes `first`.  a.leave: the sum stays in the
// slot it took; else it is launched here.  The direct kernels sum their slabs themselves, behind `first`.
int up_half_backward(const UpHalfBwd& a, Pending& pending, hipStream_t s, mi3d_up_route* route) {
    const Geo g2{a.g.N, 2 * a.g.D, 2 * a.g.H, 2 * a.g.W};
    const bool rs = up_resized(a.g, a.go);
    MI3D_CHECK_ARG(!rs || a.tmp, "up_half_backward: the resize adjoint needs the temporary");
    const void* gup = a.gup;
    int gucs = a.gucs;
    if (rs) {       // adjoint of the nearest resize in front of the concat (models/unet.py:81-83)
        MI3D_TRY(nearest_resize_bwd(a.dt, gup, gucs, a.Cout, a.go, a.tmp, a.Cout, g2, s));
        gup = a.tmp; gucs = a.Cout;
    }
    UpBwdLaunch L;
    bool left = false;
    if (a.mfma) {
        SlabJob* slot = (a.wgws2 && !mi3d_routes().no_upbwd_carry) ? pending.carry() : nullptr;
        float* slabs = slot ? a.wgws2 : a.wgws;
        if (!slot) slot = pending.first(s);
        MI3D_TRY(upconv2_mfma_bwd(a.in, a.ics, a.Cin, gup, gucs, a.Cout, a.wp, a.dx, a.dxcs, a.dW, a.db, a.accumulate, slabs,
                                  a.wgws_floats, a.g, s, a.leave ? slot : nullptr, &L));
        left = a.leave && Pending::waits(*slot);
    } else {
        pending.first(s);
        MI3D_TRY(upconv2_bwd(a.dt, a.in, a.ics, a.Cin, gup, gucs, a.Cout, a.wpb, a.dx, a.dxcs, a.dW, a.db, a.accumulate, a.wgws,
                             a.wgws_floats, a.g, s, &L));
    }
    if (route) {
        *route = mi3d_up_route{};
        route->kind = L.kind; route->ksplit = L.ksplit; route->persistent = L.persistent; route->slabs = L.slabs;
        route->slab_ew = L.slab_ew; route->wgrad_blocks = L.wgrad_blocks; route->dgrad_blocks = L.dgrad_blocks;
        route->pending = left ? 1 : 0; route->resized = rs ? 1 : 0;
    }
    return 0;
}

namespace {

constexpr int MAXL = MI3D_MAX_LEVELS;

struct HalfP {
    int Cin, Cout;
    size_t y, stat, wpf, wpd;     // byte offsets
    int pidx, bidx;
    int64_t drop_off;
    bool mfma;                    // bf16 implicit-GEMM path (conv3_mfma.hip) vs direct fp32-FMA path
    // first layer on the matrix cores (conv3_c1_fwd_mfma / conv3_mfma_wgrad_c1, taps are the K dimension).  Cin == 1 with
    // Cout % 16 == 0 can only be block 0, half 0 of a one-channel network (every other layer reads >= 2 channels or writes as
    // many as it reads), which is exactly where the input is the caller's fp32 tensor; never together with mfma (Cin % 16)
    bool c1;
    // Deferred weight gradient (round 4): with an aux stream the layer's dy gets its OWN buffer (dyk) that stays alive, the
    // data-gradient chain runs the input-gradient conv alone, and the weight gradient is launched later on the aux stream.
    //   1 = decoder layer at a 16-wide-tile level (levels 0-1 at 96^3): runs under the latency-bound deep-level chain
    //   2 = any layer at a deep level (8-wide tiles): runs under the bandwidth-bound encoder backward of levels 1-0
    //   0 = encoder layers at the 16-wide levels: nothing left to hide under, they keep the fused launch
    int defer;
    size_t dyk;
};
struct BlockP {
    int level;
    HalfP h[2];
    size_t z1;
};
struct Plan {
    mi3d_unet_desc d;
    int L, dt;
    size_t esz;
    int C[MAXL + 1];
    Geo geo[MAXL + 1];
    BlockP blk[2 * MAXL + 1];
    int nblk;
    size_t cat[MAXL], pool[MAXL], zb, zd[MAXL], upw[MAXL], xcl;
    bool up_mfma[MAXL];
    // planar[l]: the level's concat buffers cat[l] / gcat[l] hold the skip half and the up half as two [M][C] planes
    // instead of one interleaved [M][2C] tensor.  With C = 16 the interleaved halves are 32 B pieces of 64 B rows and
    // every kernel that touches ONE half (bn apply, max-pool fwd/bwd, upconv fwd/bwd) wastes half of each line.
    bool planar[MAXL];
    // resize[l]: the transposed conv's output (2x the level below) is smaller than the skip at level l (odd side somewhere
    // above) -> it goes to uptmp and is nearest-resized into the concat buffer (models/unet.py:81-83)
    bool resize[MAXL];
    size_t uptmp;
    Geo up_geo(int l) const { return Geo{geo[l + 1].N, 2 * geo[l + 1].D, 2 * geo[l + 1].H, 2 * geo[l + 1].W}; }
    int catcs(int l) const { return planar[l] ? C[l] : 2 * C[l]; }
    size_t half_off(int l) const { return (planar[l] ? (size_t)geo[l].M() * C[l] : (size_t)C[l]) * esz; }   // bytes to the up half
    Halves halves(int l) const { return halves_at(C[l] / 16, planar[l] ? geo[l].M() * C[l] - C[l] : 0); }
    size_t gz[MAXL + 1], gcat[MAXL], gp[MAXL], sB, sB2, sC;
    size_t bnws, wgws, wgws2, wgws3, statpart, skws, tkcount;
    // (block, half) after whose BatchNorm backward the pending deferred weight gradients of group 1 / 2 go to the aux stream
    int flush_b[2], flush_h[2];
    size_t wgws_floats;
    size_t total;
    int up_pidx(int i) const { return 8 * (L + 1) + 2 * i; }
    int final_pidx() const { return 8 * (L + 1) + 2 * L + 8 * L; }
};

int build_plan(const mi3d_unet_desc* d, Plan& p) {
    MI3D_CHECK_ARG(d != nullptr, "null descriptor");
    MI3D_CHECK_ARG(d->n_levels >= 1 && d->n_levels <= MAXL, "n_levels=%d out of range", d->n_levels);
    MI3D_CHECK_ARG(d->dtype == MI3D_F32 || d->dtype == MI3D_BF16, "bad dtype %d", d->dtype);
    MI3D_CHECK_ARG(d->in_channels >= 1 && d->out_channels >= 1 && d->out_channels <= MI3D_MAX_CLASSES,
                   "unsupported channel counts in=%d out=%d (out <= %d)", d->in_channels, d->out_channels, MI3D_MAX_CLASSES);
    MI3D_CHECK_ARG(d->N >= 1 && d->D >= 1 && d->H >= 1 && d->W >= 1, "bad shape");
    p.d = *d;
    p.L = d->n_levels;
    p.dt = d->dtype;
    p.esz = d->dtype == MI3D_F32 ? 4 : 2;
    // sides not divisible by 2^L: MaxPool3d floors and models/unet.py:81-83 nearest-resizes the upsampled tensor to the
    // skip's shape before the concat (resize[l]); every level must keep at least one voxel per side
    MI3D_CHECK_ARG((d->D >> p.L) >= 1 && (d->H >> p.L) >= 1 && (d->W >> p.L) >= 1,
                   "volume %dx%dx%d too small for %d pooling levels", d->D, d->H, d->W, p.L);
    for (int l = 0; l < p.L; l++) {
        MI3D_CHECK_ARG(d->features[l] >= 1 && d->features[l] <= 256, "feature %d out of range", d->features[l]);
        if (l > 0) MI3D_CHECK_ARG(d->features[l] == 2 * d->features[l - 1], "features must double per level");
        p.C[l] = d->features[l];
    }
    p.C[p.L] = 2 * d->features[p.L - 1];
    MI3D_CHECK_ARG(p.C[p.L] <= 256, "bottleneck width %d > 256", p.C[p.L]);
    for (int l = 0; l <= p.L; l++) p.geo[l] = Geo{d->N, d->D >> l, d->H >> l, d->W >> l};
    size_t up_elems = 0;
    for (int l = 0; l < p.L; l++) {
        Geo u = p.up_geo(l);
        p.resize[l] = u.D != p.geo[l].D || u.H != p.geo[l].H || u.W != p.geo[l].W;
        if (p.resize[l] && (size_t)u.M() * d->features[l] > up_elems) up_elems = (size_t)u.M() * d->features[l];
    }

    for (int l = 0; l < p.L; l++)
        p.planar[l] = p.dt == MI3D_BF16 && p.C[l] % 16 == 0 && conv3_mfma_halves_ok(2 * p.C[l], p.C[l], p.geo[l]) &&
                      conv3_mfma_halves_ok(p.C[l], 2 * p.C[l], p.geo[l]) && !mi3d_routes().no_planar;
    Arena A;
    int64_t drop_off = 0;
    size_t wg_floats = 0, maxCM = 0, statpart_floats = 1, skws_floats = 1;
    int maxC = 1;
    p.nblk = 2 * p.L + 1;
    for (int b = 0; b < p.nblk; b++) {
        BlockP& B = p.blk[b];
        int cin, cout;
        if (b < p.L) { B.level = b; cin = b == 0 ? d->in_channels : p.C[b - 1]; cout = p.C[b]; }
        else if (b == p.L) { B.level = p.L; cin = p.C[p.L - 1]; cout = p.C[p.L]; }
        else { int i = b - p.L - 1; B.level = p.L - 1 - i; cin = 2 * p.C[B.level]; cout = p.C[B.level]; }
        Geo g = p.geo[B.level];
        int pbase = b <= p.L ? 8 * b : 8 * (p.L + 1) + 2 * p.L + 8 * (b - p.L - 1);
        for (int h = 0; h < 2; h++) {
            HalfP& H = B.h[h];
            H.Cin = h == 0 ? cin : cout;
            H.Cout = cout;
            H.y = A.take((size_t)g.M() * cout * p.esz);
            H.stat = A.take((size_t)4 * cout * sizeof(float));
            // the shared areas (statistics rows, split-K partials, slabs) hold the largest layer's
            const ConvScratch S = conv3_scratch(p.dt, H.Cin, H.Cout, g);
            H.mfma = S.mfma; H.c1 = S.c1;
            H.wpf = A.take(S.wpf_bytes);
            H.wpd = A.take(S.wpd_bytes);
            if (S.mfma || S.c1) statpart_floats = std::max(statpart_floats, (size_t)S.stat_rows * 2 * cout);      // the direct kernels write no rows
            skws_floats = std::max(skws_floats, std::max(S.splitk_fwd_floats, S.splitk_bwd_floats));
            wg_floats = std::max(wg_floats, S.wgrad_floats);
            H.pidx = pbase + 4 * h;
            H.bidx = 6 * b + 3 * h;
            H.drop_off = drop_off;
            drop_off += (int64_t)d->N * cout;
            // the dy buffers are part of the layout whatever the route says (a route changed between the workspace query and a
            // launch must not move anything)
            H.defer = !H.mfma ? 0 : !conv3_mfma_big_geo(g) ? 2 : (b > p.L ? 1 : 0);
            H.dyk = H.defer ? A.take((size_t)g.M() * cout * p.esz) : 0;
        }
        B.z1 = A.take((size_t)g.M() * cout * p.esz);
        if ((size_t)g.M() * cout > maxCM) maxCM = (size_t)g.M() * cout;
        if (cout > maxC) maxC = cout;
    }
    for (int l = 0; l < p.L; l++) {
        p.cat[l] = A.take((size_t)p.geo[l].M() * 2 * p.C[l] * p.esz);
        p.pool[l] = A.take((size_t)p.geo[l + 1].M() * p.C[l] * p.esz);
        p.gcat[l] = A.take((size_t)p.geo[l].M() * 2 * p.C[l] * p.esz);
        p.gp[l] = A.take((size_t)p.geo[l + 1].M() * p.C[l] * p.esz);
        p.gz[l] = A.take((size_t)p.geo[l].M() * p.C[l] * p.esz);
    }
    p.gz[p.L] = A.take((size_t)p.geo[p.L].M() * p.C[p.L] * p.esz);
    p.zb = A.take((size_t)p.geo[p.L].M() * p.C[p.L] * p.esz);
    for (int i = 0; i < p.L; i++) {
        int l = p.L - 1 - i;
        p.zd[i] = A.take((size_t)p.geo[l].M() * p.C[l] * p.esz);
        // a level runs the kernels of its class only: the class's images and slabs
        const UpScratch U = upconv2_scratch(p.dt, 2 * p.C[l], p.C[l], p.geo[l + 1]);
        p.up_mfma[i] = U.mfma;
        p.upw[i] = A.take(U.pack_bytes);
        wg_floats = std::max(wg_floats, U.wgrad_floats);
    }
    p.uptmp = up_elems ? A.take(up_elems * p.esz) : 0;
    p.xcl = d->in_channels > 1 ? A.take((size_t)p.geo[0].M() * d->in_channels * p.esz) : 0;
    wg_floats = std::max(wg_floats, conv1_bwd_ws_floats(p.C[0], d->out_channels));
    p.sB = A.take(maxCM * p.esz);
    p.sB2 = A.take(maxCM * p.esz);
    p.sC = A.take(maxCM * p.esz);
    p.bnws = A.take(bn_ws_floats(maxC) * sizeof(float));
    p.statpart = A.take(statpart_floats * sizeof(float));
    p.tkcount = A.take((size_t)CONV3_TK_COUNTERS * sizeof(int));        // split-K ticket counters (zeroed by the forward's pack launch)
    p.skws = A.take(skws_floats * sizeof(float));
    p.wgws_floats = wg_floats;
    p.wgws = A.take(wg_floats * sizeof(float));
    p.wgws2 = A.take(wg_floats * sizeof(float));
    p.wgws3 = A.take(wg_floats * sizeof(float));       // slabs of the weight gradients on the aux stream
    // backward order of the conv layers: decoder.L-1 .. decoder.0 (level 0 first), bottleneck, encoder.L-1 .. 0; half 1 then 0
    for (int k = 0; k < 2; k++) p.flush_b[k] = p.flush_h[k] = -1;
    for (int q = 0; q < p.nblk; q++) {
        int b = 2 * p.L - q;
        for (int h = 1; h >= 0; h--) {
            int dfr = p.blk[b].h[h].defer;
            if (dfr) { p.flush_b[dfr - 1] = b; p.flush_h[dfr - 1] = h; }
        }
    }
    p.total = A.off;
    return 0;
}

// the state of one C call
struct Ctx {
    const Plan& p;
    char* ws = nullptr;
    const void* const* params = nullptr;
    hipStream_t s = nullptr;
    // optional second stream: the DEFERRED weight gradients (HalfP::defer) run there, off the data-gradient chain, behind
    // at most three forks per call (events 0..2) and one join (event 3); works eagerly and inside a hipGraph capture
    hipStream_t s2 = nullptr;
    hipEvent_t* ev = nullptr;
    int seq = 0;
    struct DJob { int b, h, dxcs; };      // dxcs = 0: the layer has no input gradient
    DJob dq[4 * MAXL + 2];             // weight gradients whose dy is ready and that have not been forked yet
    // forked (their event is recorded on the chain) but not yet ENQUEUED on the aux stream: the host enqueues them a few at a
    // time between the chain's next launches (drain_aux).  A step is launched by ONE host thread, and at the end of the
    // launch-bound deep-level chain it is barely ahead of the GPU: enqueueing the ten deep-level weight gradients and their slab
    // sums in one go left the chain's queue empty for ~125 us (profiles/r04_defer_eager_streams_before.txt)
    struct HJob { int b, h, dxcs, ev; };
    HJob hq[4 * MAXL + 2];
    int nhq = 0, hq_head = 0, waited_ev = -1;
    int ndq = 0, nfork = 0;
    bool aux_used = false;
    bool tk_zeroed = false;   // this call's pack launch cleared the split-K ticket counters
    // training & 4: another forward runs beside this one on a second stream (DANN source || target): the wide BatchNorm consumers
    // (whole-CU 1024-thread workgroups) get in each other's way there (+45 us/step measured); thin consumers + finalize launches
    bool beside = false;
    Pending pending;
    // the input gradient of a block's first conv (= the gradient of the pooled tensor one level up) left as split-K partials for
    // the MaxPool3d backward of the next segment to finish (no splitk_finish launch); pool_defer: the caller allows it
    int pool_ks = 0;
    bool pool_defer = false;
    template <typename T = void> T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }
    const float* P(int i) const { return reinterpret_cast<const float*>(params[i]); }
};

// The one way into a call that launches: plan, pointers, workspace size and alignment.  `fn` is the public function the
// caller used, `ptrs` whether the pointers only that function takes are all there.
int enter(Ctx& c, Plan& p, const mi3d_unet_desc* d, const char* fn, bool ptrs, const void* const* params, void* workspace,
          size_t workspace_bytes, void* stream) {
    MI3D_TRY(build_plan(d, p));
    MI3D_CHECK_ARG(ptrs && params && workspace, "%s: null pointer", fn);
    MI3D_CHECK_ARG(workspace_bytes >= p.total, "workspace too small: %zu < %zu", workspace_bytes, p.total);
    MI3D_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    c.ws = (char*)workspace;
    c.params = params;
    c.s = (hipStream_t)stream;
    return 0;
}

// What one conv layer (block b, half h) reads and writes; its route class is H.mfma / H.c1.  x = the network's input.
struct LayerIO {
    const HalfP& H;
    Geo g;
    const void* in; int ics, idt;     // input tensor: pointer, channel stride, dtype
    void* out; int ocs;               // activated output (z1 of the block for half 0, the block's output for half 1)
    Halves ih;                        // planes of the input: on() only for half 0 of a decoder block at a planar level
};
LayerIO layer_io(const Ctx& c, int b, int h, const float* x) {
    const Plan& p = c.p;
    const BlockP& B = p.blk[b];
    const HalfP& H = B.h[h];
    const int l = B.level;
    LayerIO v{H, p.geo[l], c.at(B.z1), H.Cout, p.dt, c.at(B.z1), H.Cout, Halves()};
    if (h == 1) {
        if (b < p.L) { v.out = c.at(p.cat[b]); v.ocs = p.catcs(b); }
        else v.out = c.at(b == p.L ? p.zb : p.zd[b - p.L - 1]);
    } else if (b == 0) {
        if (p.d.in_channels == 1) { v.in = x; v.ics = 1; v.idt = MI3D_F32; }
        else { v.in = c.at(p.xcl); v.ics = p.d.in_channels; }
    } else if (b <= p.L) { v.in = c.at(p.pool[b - 1]); v.ics = p.C[b - 1]; }
    else { v.in = c.at(p.cat[l]); v.ics = p.catcs(l); v.ih = p.halves(l); }
    return v;
}

// pooled != NULL (encoder blocks on even volumes): the second apply pass also writes MaxPool3d(2,2) of the block output
int block_forward(Ctx& c, int b, const float* x, void* const* buffers, const float* drop, int training,
                  void* pooled = nullptr, int pcs = 0) {
    const Plan& p = c.p;
    for (int h = 0; h < 2; h++) {
        const LayerIO v = layer_io(c, b, h, x);
        const HalfP& H = v.H;
        const Geo g = v.g;
        float* rm = buffers ? (float*)buffers[H.bidx] : nullptr;
        float* rv = buffers ? (float*)buffers[H.bidx + 1] : nullptr;
        int64_t* nbt = buffers ? (int64_t*)buffers[H.bidx + 2] : nullptr;
        // training == 2: deferred running-statistics update -- buffers[bidx] is a double[2C] side buffer (ops.h bn_deferred_apply)
        const float mom = training == 2 ? -1.f : p.d.bn_momentum;
        if (training == 2) { rv = nullptr; nbt = nullptr; }
        ConvBnHalf a{H.Cin, H.Cout, g, p.dt, H.mfma, H.c1, v.in, v.ics, v.idt, v.ih,
                     c.P(H.pidx), c.P(H.pidx + 1), c.P(H.pidx + 2), c.P(H.pidx + 3), c.at(H.wpf), c.at(H.wpd),
                     c.at(H.y), c.at<float>(H.stat), rm, rv, nbt, mom, p.d.bn_eps, training, c.tk_zeroed, c.beside,
                     c.at<float>(p.statpart), c.at<float>(p.skws), c.at<int>(p.tkcount), c.at<float>(p.bnws),
                     drop ? drop + H.drop_off : nullptr, v.out, v.ocs, h == 1 ? pooled : nullptr, pcs};
        MI3D_TRY(conv3_bn_half_forward(a, c.s));
    }
    return 0;
}

// enqueue up to `n` forked weight gradients on the aux stream (n < 0: all).  Each runs after the fork event of its group, one
// after the other there, followed by its slab sum, sharing the third slab workspace; nothing on the compute stream waits for
// them before the end of the step (unet_backward_impl joins).
int drain_aux(Ctx& c, const float* x, void* const* grads, int accumulate, int n) {
    const Plan& p = c.p;
    for (; c.hq_head < c.nhq && n != 0; c.hq_head++, n--) {
        const Ctx::HJob& j = c.hq[c.hq_head];
        if (j.ev != c.waited_ev) { MI3D_HIP(hipStreamWaitEvent(c.s2, c.ev[j.ev % 3], 0)); c.waited_ev = j.ev; }
        const LayerIO v = layer_io(c, j.b, j.h, x);
        const HalfP& H = v.H;
        MI3D_TRY(conv3_deferred_wgrad(v.in, v.ics, H.Cin, v.ih, c.at(H.dyk), H.Cout, H.Cout, v.g, j.dxcs, (float*)grads[H.pidx],
                                      (float*)grads[H.pidx + 1], accumulate, c.at<float>(p.wgws3), p.wgws_floats, c.s2));
        c.aux_used = true;
    }
    if (c.hq_head == c.nhq) c.hq_head = c.nhq = 0;
    return 0;
}

// Fork: the queued weight gradients may start once everything the compute stream has enqueued so far is done (their dy
// buffers are complete).  lazy: only the event is recorded here, the launches are enqueued by later drain_aux calls.
int flush_deferred(Ctx& c, const float* x, void* const* grads, int accumulate, bool lazy = false) {
    if (c.ndq == 0) return 0;
    MI3D_CHECK_ARG(c.nfork < 3, "flush_deferred: more than three forks in one call");
    const int e = c.nfork++;
    MI3D_HIP(hipEventRecord(c.ev[e % 3], c.s));
    for (int q = 0; q < c.ndq; q++) c.hq[c.nhq++] = Ctx::HJob{c.dq[q].b, c.dq[q].h, c.dq[q].dxcs, e};
    c.ndq = 0;
    if (!lazy) MI3D_TRY(drain_aux(c, x, grads, accumulate, -1));
    return 0;
}

// backward of block b given dz2 (dtype T, stride dzcs); writes dxin (may be NULL) with stride dxcs.  The per-layer decisions are
// conv3_bn_half_backward's; what stays here is the aux stream: the queue of deferred weight gradients and the fork points
struct ForkAt { Ctx* c; int b, h; const float* x; void* const* grads; int accumulate; bool dfr; int dxcs; };
int fork_after_bn(void* arg) {
    const ForkAt& f = *(const ForkAt*)arg;
    Ctx& c = *f.c;
    const Plan& p = c.p;
    // deferred weight gradient: queued for the aux stream (conv3_deferred_wgrad, drain_aux)
    if (f.dfr) c.dq[c.ndq++] = Ctx::DJob{f.b, f.h, f.dxcs};
    // fork points: what is queued goes to the aux stream when the chain has finished the last layer of a group (its BatchNorm
    // backward).  Group 1 forks when the GPU is still busy with the full-resolution decoder (the host is far ahead: enqueue at
    // once); group 2 forks at the end of the launch-bound deep chain: its launches are fed in between the chain's next ones.
    // (Measured and dropped, profiles/r04_experiments_aux_wgrad.txt and the fork-placement record beside it: one fork per layer +26 ... +43 us,
    // per deep layer only +6 us, the decoder fork one block later -1 us, another workgroup count for the aux kernels +10 ... +40 us,
    // deferring only some of the three groups 13 ... 102 us)
    if (c.s2 != nullptr && c.ev != nullptr)
        for (int q = 0; q < 2; q++)
            if (f.b == p.flush_b[q] && f.h == p.flush_h[q]) MI3D_TRY(flush_deferred(c, f.x, f.grads, f.accumulate, q == 1));
    return 0;
}
int block_backward(Ctx& c, int b, const float* x, void* const* grads, const float* drop, const void* dz2,
                   int dzcs, void* dxin, int dxcs, int accumulate) {
    const Plan& p = c.p;
    auto G = [&](int i) { return grads ? (float*)grads[i] : nullptr; };
    const bool aux = c.s2 != nullptr && c.ev != nullptr;
    float* const skws = c.at<float>(p.skws);
    const float* dz_skp = nullptr;      // dz of half 0 left as split-K partials by half 1's input gradient
    int dz_ks = 0;
    for (int h = 1; h >= 0; h--) {
        const LayerIO v = layer_io(c, b, h, x);
        const HalfP& H = v.H;
        int k = c.seq++;
        if (aux && c.nhq) MI3D_TRY(drain_aux(c, x, grads, accumulate, 3));      // feed the aux stream between the chain's launches
        const bool wg = G(H.pidx) || G(H.pidx + 1);
        // deferred weight gradient: dy goes to the layer's own buffer, which nobody overwrites before the aux stream has read it
        const bool dfr = aux && H.defer && wg;
        void* dx = h == 1 ? c.at(p.sC) : dxin;
        const int dxs = h == 1 ? H.Cin : dxcs;
        ForkAt f{&c, b, h, x, grads, accumulate, dfr, dx ? dxs : 0};
        // half 1's input gradient feeds straight into half 0's BatchNorm-backward reduction, half 0's into the MaxPool3d backward of
        // the next segment (pool_defer): a split-K result may stay as partials, filed here for whoever reads them
        ConvBnHalfBwd a{H.Cin, H.Cout, v.g, p.dt, H.mfma, H.c1, v.in, v.ics, v.idt, v.ih, c.at(H.wpd),
                        c.at(H.y), c.at<float>(H.stat), drop ? drop + H.drop_off : nullptr,
                        h == 1 ? dz2 : c.at(p.sC), h == 1 ? dzcs : H.Cout, h == 0 ? dz_skp : nullptr, h == 0 ? dz_ks : 0,
                        dfr ? c.at(H.dyk) : c.at((k & 1) ? p.sB2 : p.sB), H.Cout, dx, dxs, v.ih,
                        G(H.pidx), G(H.pidx + 1), G(H.pidx + 2), G(H.pidx + 3), accumulate,
                        c.at<float>(p.bnws), c.at<float>(p.wgws), p.wgws_floats, skws, h == 1 || c.pool_defer, dfr, fork_after_bn, &f};
        int ksd = 0;
        MI3D_TRY(conv3_bn_half_backward(a, c.pending, c.s, &ksd));
        if (ksd > 0 && h == 1) { dz_skp = skws; dz_ks = ksd; }
        if (ksd > 0 && h == 0) c.pool_ks = ksd;
    }
    return 0;
}

// inference forward of block b (conv3_bn_half_infer per half): no raw conv output, no statistics, no separate normalisation
// pass.  stat[0..C) = scale, stat[C..2C) = folded bias (bn_fold_all).
int block_infer(Ctx& c, int b, const float* x) {
    const Plan& p = c.p;
    for (int h = 0; h < 2; h++) {
        const LayerIO v = layer_io(c, b, h, x);
        const HalfP& H = v.H;
        const float* scale = c.at<float>(H.stat);
        ConvBnHalfInfer a{H.Cin, H.Cout, v.g, p.dt, H.mfma, H.c1, v.in, v.ics, v.idt, v.ih, c.P(H.pidx), c.at(H.wpf),
                          scale, scale + H.Cout, v.out, v.ocs, c.at<float>(p.skws)};
        MI3D_TRY(conv3_bn_half_infer(a, c.s));
    }
    return 0;
}

// Every MFMA weight image of the network (DoubleConv blocks, transposed convs) as jobs of ONE launch.  fold_scale (inference):
// the BatchNorm scale bn_fold_all leaves in stat[0..C) is multiplied into the forward images
int add_pack_jobs(const Ctx& c, PackJobs& J, bool fold_scale) {
    const Plan& p = c.p;
    for (int b = 0; b < p.nblk; b++)
        for (int h = 0; h < 2; h++) {
            const HalfP& H = p.blk[b].h[h];
            if (H.mfma)
                MI3D_TRY(pack_all_add_conv3(J, c.P(H.pidx), H.Cin, H.Cout, c.at(H.wpf), c.at(H.wpd), p.geo[p.blk[b].level],
                                            fold_scale ? c.at<float>(H.stat) : nullptr));
        }
    for (int i = 0; i < p.L; i++) {
        int l = p.L - 1 - i;
        if (p.up_mfma[i]) MI3D_TRY(pack_all_add_upconv(J, c.P(p.up_pidx(i)), 2 * p.C[l], p.C[l], c.at(p.upw[i])));
    }
    return 0;
}

// Decoder step i (level l = L-1-i): the transposed conv takes the block below (2C channels at level l + 1) to the up half of
// cat[l]; its backward takes the up half of gcat[l] back
struct UpIO {
    int l, Cin, Cout;
    Geo g;                       // INPUT geometry
    const void* in;
    float* w; float* wb;         // packed weights: the MFMA image or the direct forward image / the direct backward image
    size_t half; int cs;         // bytes to the up half of cat[l] and gcat[l] / their channel stride
};
UpIO up_io(const Ctx& c, int i) {
    const Plan& p = c.p;
    const int l = p.L - 1 - i, C = p.C[l];
    float* w = c.at<float>(p.upw[i]);
    return UpIO{l, 2 * C, C, p.geo[l + 1], c.at(i == 0 ? p.zb : p.zd[i - 1]), w, w + (size_t)cdiv(C, 8) * (2 * C) * 64,
                p.half_off(l), p.catcs(l)};
}
// forward of decoder step i, with the nearest resize where resize[l] (training and inference)
int up_forward(Ctx& c, int i) {
    const Plan& p = c.p;
    const UpIO u = up_io(c, i);
    char* up = c.at<char>(p.cat[u.l]) + u.half;
    UpHalf a{u.Cin, u.Cout, u.g, p.dt, p.up_mfma[i], u.in, u.Cin, c.P(p.up_pidx(i)), c.P(p.up_pidx(i) + 1), u.w, u.wb,
             up, u.cs, p.geo[u.l], p.resize[u.l] ? c.at(p.uptmp) : nullptr};
    return up_half_forward(a, c.s);
}

}  // namespace

extern "C" {

int mi3d_abi_version(void) { return 9; }

int mi3d_unet_num_params(const mi3d_unet_desc* d) { return d ? 8 * (2 * d->n_levels + 1) + 2 * d->n_levels + 2 : -1; }
int mi3d_unet_num_buffers(const mi3d_unet_desc* d) { return d ? 6 * (2 * d->n_levels + 1) : -1; }
int mi3d_unet_num_segments(const mi3d_unet_desc* d) { return d ? 2 * d->n_levels + 2 : -1; }

size_t mi3d_unet_workspace_bytes(const mi3d_unet_desc* d) {
    Plan p;
    if (build_plan(d, p) != 0) return 0;
    return p.total;
}

int64_t mi3d_unet_dropout_count(const mi3d_unet_desc* d) {
    Plan p;
    if (build_plan(d, p) != 0) return -1;
    const HalfP& last = p.blk[p.nblk - 1].h[1];
    return last.drop_off + (int64_t)d->N * last.Cout;
}

int mi3d_unet_segment_params(const mi3d_unet_desc* d, int seg, int* r) {
    Plan p;
    MI3D_TRY(build_plan(d, p));
    int L = p.L;
    MI3D_CHECK_ARG(seg >= 0 && seg < 2 * L + 2 && r, "bad segment %d", seg);
    r[2] = r[3] = -1;
    if (seg == 0) { r[0] = p.final_pidx(); r[1] = r[0] + 2; }
    else if (seg <= L) {
        int i = L - seg;          // decoder.i and upconvs.i
        r[0] = p.blk[L + 1 + i].h[0].pidx; r[1] = r[0] + 8;
        r[2] = p.up_pidx(i); r[3] = r[2] + 2;
    } else if (seg == L + 1) { r[0] = p.blk[L].h[0].pidx; r[1] = r[0] + 8; }
    else { int l = 2 * L + 1 - seg; r[0] = p.blk[l].h[0].pidx; r[1] = r[0] + 8; }
    return 0;
}

}  // extern "C"

// the segmentation loss of the training loop folded into the 1x1x1 head (head_loss.hip): forward half / backward half
struct HeadLoss {
    const int64_t* labels; LossCfg cfg; float* loss_out; float* coef; float* metrics_out; void* loss_ws; void* met_ws;   // forward
    const float* grad_scale;                                                                                              // backward
    const float* teacher;                                                                 // (N,C,V) teacher logits iff cfg.w_kd != 0
};
static LossCfg cfg_of(const mi3d_loss_cfg* c) {
    LossCfg k;
    k.w_ce = c->w_ce; k.region_kind = c->region_kind; k.w_reg = c->w_reg; k.alpha = c->alpha; k.beta = c->beta; k.eps = c->eps;
    k.w_kd = c->w_kd; k.temp = c->temperature > 0.f ? c->temperature : 1.f;
    return k;
}
// the loss configuration of a *_masked entry (ops.h loss_cfg_ignore)
#define MI3D_MASKED_CFG(k, cfg, ignore_index, what) \
    LossCfg k = cfg_of(cfg);                        \
    MI3D_CHECK_ARG(loss_cfg_ignore(k, ignore_index), what ": ignore_index %lld does not fit int32", (long long)(ignore_index))

static int unet_forward_impl(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* buffers,
                      const float* drop_scales, int training, float* logits, float* gap_out, void* workspace,
                      size_t workspace_bytes, void* stream, const HeadLoss* hl) {
    Plan p;
    Ctx c{p};
    MI3D_TRY(enter(c, p, d, "mi3d_unet_forward", x != nullptr, params, workspace, workspace_bytes, stream));
    c.beside = (training & 4) != 0;
    training &= 3;
    int L = p.L;
    if (d->in_channels > 1)
        MI3D_TRY(ncdhw_to_ndhwc(p.dt, x, c.at(p.xcl), d->in_channels, d->in_channels, d->N, p.geo[0].V(), c.s));
    {   // every MFMA weight pack of the network in one launch, which also clears the split-K ticket counters of a training forward
        PackJobs J;
        J.n = 0; J.nblocks = 0;
        if (training) { J.zero = c.at<int>(p.tkcount); J.nzero = CONV3_TK_COUNTERS; }
        MI3D_TRY(add_pack_jobs(c, J, false));
        if (training && J.n > 0) c.tk_zeroed = true;      // (pack_all_launch launches nothing for an empty job list)
        MI3D_TRY(pack_all_launch(J, c.s));
    }
    for (int l = 0; l < L; l++) {
        // fused apply + pool: even sides (every voxel in exactly one window) and 32-bit element indices
        const bool even = p.geo[l].D % 2 == 0 && p.geo[l].H % 2 == 0 && p.geo[l].W % 2 == 0 &&
                          p.geo[l].M() * p.C[l] < (1ll << 31) && !mi3d_routes().no_pool_fuse;
        MI3D_TRY(block_forward(c, l, x, buffers, drop_scales, training, even ? c.at(p.pool[l]) : nullptr, p.C[l]));
        if (!even) MI3D_TRY(maxpool2_fwd(p.dt, c.at(p.cat[l]), p.catcs(l), p.C[l], p.geo[l], c.at(p.pool[l]), p.C[l], c.s));
    }
    MI3D_TRY(block_forward(c, L, x, buffers, drop_scales, training));
    if (gap_out) MI3D_TRY(gap_fwd(p.dt, c.at(p.zb), p.C[L], p.C[L], d->N, p.geo[L].V(), gap_out, c.s));
    for (int i = 0; i < L; i++) {
        MI3D_TRY(up_forward(c, i));
        MI3D_TRY(block_forward(c, L + 1 + i, x, buffers, drop_scales, training));
    }
    if (hl) {
        MI3D_CHECK_ARG(head_loss_ok(p.dt, c.at(p.zd[L - 1]), p.C[0], p.C[0], d->out_channels, hl->cfg),
                       "mi3d_unet_forward_loss: no fused head + loss for this configuration (see mi3d_unet_head_loss_supported)");
        return head_loss_fwd(c.at(p.zd[L - 1]), p.C[0], p.C[0], c.P(p.final_pidx()), c.P(p.final_pidx() + 1), hl->labels, hl->teacher,
                             d->N, d->out_channels, p.geo[0].V(), hl->cfg, hl->loss_out, hl->coef, hl->loss_ws, c.s, d->D,
                             hl->metrics_out, hl->met_ws, logits);
    }
    if (logits)       // NULL: the caller does not want the logits (DANN target pass) or runs the head with mi3d_unet_head_loss_forward
        MI3D_TRY(conv1_fwd(p.dt, c.at(p.zd[L - 1]), p.C[0], p.C[0], c.P(p.final_pidx()), c.P(p.final_pidx() + 1), logits,
                           d->out_channels, d->N, p.geo[0].V(), c.s));
    return 0;
}

// head + loss on the decoder output the last mi3d_unet_forward / mi3d_unet_infer (logits = NULL) left in this workspace
static int unet_head_loss_forward_impl(const mi3d_unet_desc* d, const void* const* params, const int64_t* labels, const float* teacher_logits,
                                       LossCfg k, float* loss_out, float* coef, float* metrics_out, void* loss_workspace,
                                       void* metrics_workspace, float* logits_opt, void* workspace, size_t workspace_bytes, void* stream) {
    Plan p;
    Ctx c{p};
    MI3D_TRY(enter(c, p, d, "mi3d_unet_head_loss_forward", labels && loss_out && coef && loss_workspace, params, workspace,
                   workspace_bytes, stream));
    MI3D_CHECK_ARG(head_loss_ok(p.dt, c.at(p.zd[p.L - 1]), p.C[0], p.C[0], d->out_channels, k),
                   "mi3d_unet_head_loss_forward: no fused head + loss for this configuration (see mi3d_unet_head_loss_supported)");
    return head_loss_fwd(c.at(p.zd[p.L - 1]), p.C[0], p.C[0], c.P(p.final_pidx()), c.P(p.final_pidx() + 1), labels, teacher_logits, d->N,
                         d->out_channels, p.geo[0].V(), k, loss_out, coef, loss_workspace, c.s, d->D, metrics_out, metrics_workspace,
                         logits_opt);
}

extern "C" {

int mi3d_unet_head_loss_forward(const mi3d_unet_desc* d, const void* const* params, const int64_t* labels, const float* teacher_logits,
                                const mi3d_loss_cfg* cfg, float* loss_out, float* coef, float* metrics_out, void* loss_workspace,
                                void* metrics_workspace, float* logits_opt, void* workspace, size_t workspace_bytes, void* stream) {
    MI3D_CHECK_ARG(cfg, "mi3d_unet_head_loss_forward: null pointer");
    return unet_head_loss_forward_impl(d, params, labels, teacher_logits, cfg_of(cfg), loss_out, coef, metrics_out, loss_workspace,
                                       metrics_workspace, logits_opt, workspace, workspace_bytes, stream);
}
int mi3d_unet_head_loss_forward_masked(const mi3d_unet_desc* d, const void* const* params, const int64_t* labels,
                                       const float* teacher_logits, const mi3d_loss_cfg* cfg, int64_t ignore_index, float* loss_out,
                                       float* coef, float* metrics_out, void* loss_workspace, void* metrics_workspace, float* logits_opt,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    MI3D_CHECK_ARG(cfg, "mi3d_unet_head_loss_forward_masked: null pointer");
    MI3D_MASKED_CFG(k, cfg, ignore_index, "mi3d_unet_head_loss_forward_masked");
    return unet_head_loss_forward_impl(d, params, labels, teacher_logits, k, loss_out, coef, metrics_out, loss_workspace,
                                       metrics_workspace, logits_opt, workspace, workspace_bytes, stream);
}

// head + argmax (+ per-sample counts) on that same decoder output: the sibling of mi3d_unet_head_loss_forward for inference
int mi3d_unet_head_labels(const mi3d_unet_desc* d, const void* const* params, const int64_t* target, uint8_t* labels_out,
                          int64_t* counts, void* head_workspace, void* workspace, size_t workspace_bytes, void* stream) {
    Plan p;
    Ctx c{p};
    MI3D_TRY(enter(c, p, d, "mi3d_unet_head_labels", labels_out != nullptr, params, workspace, workspace_bytes, stream));
    return head_labels(p.dt, c.at(p.zd[p.L - 1]), p.C[0], p.C[0], c.P(p.final_pidx()), c.P(p.final_pidx() + 1), d->out_channels, d->N,
                       p.geo[0].V(), labels_out, target, counts, head_workspace, c.s);
}

// head + softmax + vote of one view of a flip / model ensemble on that same decoder output (mi3d_head_votes)
int mi3d_unet_head_votes(const mi3d_unet_desc* d, const void* const* params, int flip, int view, int views, int flags, float* votes,
                         uint8_t* labels_out, float* confidence, const int64_t* target, int64_t* counts, void* head_workspace,
                         void* workspace, size_t workspace_bytes, void* stream) {
    Plan p;
    Ctx c{p};
    MI3D_TRY(enter(c, p, d, "mi3d_unet_head_votes", true, params, workspace, workspace_bytes, stream));
    return head_votes(p.dt, c.at(p.zd[p.L - 1]), p.C[0], p.C[0], c.P(p.final_pidx()), c.P(p.final_pidx() + 1), d->out_channels, d->N,
                      p.geo[0].D, p.geo[0].H, p.geo[0].W, flip, view, views, flags, votes, labels_out, confidence, target, counts, head_workspace, c.s);
}

// head + softmax + weighted vote of the d->N window samples of that same decoder output into one accumulator (mi3d_head_votes_window)
int mi3d_unet_head_votes_window(const mi3d_unet_desc* d, const void* const* params, const int* flips, const float* g_d, const float* g_h,
                                const float* g_w, const int* origins, float* acc, int D, int H, int W, void* workspace,
                                size_t workspace_bytes, void* stream) {
    Plan p;
    Ctx c{p};
    MI3D_TRY(enter(c, p, d, "mi3d_unet_head_votes_window", true, params, workspace, workspace_bytes, stream));
    return head_votes_window(p.dt, c.at(p.zd[p.L - 1]), p.C[0], p.C[0], c.P(p.final_pidx()), c.P(p.final_pidx() + 1), d->out_channels, d->N,
                             p.geo[0].D, p.geo[0].H, p.geo[0].W, flips, g_d, g_h, g_w, origins, acc, D, H, W, c.s);
}

int mi3d_unet_forward(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* buffers,
                      const float* drop_scales, int training, float* logits, float* gap_out, void* workspace,
                      size_t workspace_bytes, void* stream) {
    return unet_forward_impl(d, x, params, buffers, drop_scales, training, logits, gap_out, workspace, workspace_bytes, stream, nullptr);
}

int mi3d_unet_head_loss_supported(const mi3d_unet_desc* d, const mi3d_loss_cfg* cfg) {
    Plan p;
    if (!d || !cfg || build_plan(d, p) != 0) return 0;
    LossCfg k = cfg_of(cfg);
    // the plan's activations are 256-byte aligned and dense: only dtype / channel counts / loss terms decide
    return head_loss_bwd_ok(p.dt, nullptr, p.C[0], p.C[0], d->out_channels, k, nullptr, p.C[0]) ? 1 : 0;
}

int mi3d_unet_forward_loss(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* buffers,
                           const float* drop_scales, int training, const int64_t* labels, const float* teacher_logits,
                           const mi3d_loss_cfg* cfg, float* loss_out, float* coef, float* metrics_out, void* loss_workspace,
                           void* metrics_workspace, float* logits_opt, float* gap_out, void* workspace, size_t workspace_bytes,
                           void* stream) {
    MI3D_CHECK_ARG(labels && cfg && loss_out && coef && loss_workspace, "mi3d_unet_forward_loss: null pointer");
    HeadLoss hl{labels, cfg_of(cfg), loss_out, coef, metrics_out, loss_workspace, metrics_workspace, nullptr, teacher_logits};
    return unet_forward_impl(d, x, params, buffers, drop_scales, training, logits_opt, gap_out, workspace, workspace_bytes, stream, &hl);
}
int mi3d_unet_forward_loss_masked(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* buffers,
                                  const float* drop_scales, int training, const int64_t* labels, const float* teacher_logits,
                                  const mi3d_loss_cfg* cfg, int64_t ignore_index, float* loss_out, float* coef, float* metrics_out,
                                  void* loss_workspace, void* metrics_workspace, float* logits_opt, float* gap_out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    MI3D_CHECK_ARG(labels && cfg && loss_out && coef && loss_workspace, "mi3d_unet_forward_loss_masked: null pointer");
    MI3D_MASKED_CFG(k, cfg, ignore_index, "mi3d_unet_forward_loss_masked");
    HeadLoss hl{labels, k, loss_out, coef, metrics_out, loss_workspace, metrics_workspace, nullptr, teacher_logits};
    return unet_forward_impl(d, x, params, buffers, drop_scales, training, logits_opt, gap_out, workspace, workspace_bytes, stream, &hl);
}

int mi3d_unet_bn_apply_deferred(const mi3d_unet_desc* d, void* const* buffers, const void* const* side, void* stream) {
    Plan p;
    MI3D_TRY(build_plan(d, p));
    MI3D_CHECK_ARG(buffers && side, "mi3d_unet_bn_apply_deferred: null pointer");
    BnDeferJobs J;
    J.n = 0; J.momentum = d->bn_momentum;
    for (int b = 0; b < p.nblk; b++)
        for (int h = 0; h < 2; h++) {
            const HalfP& H = p.blk[b].h[h];
            MI3D_CHECK_ARG(buffers[H.bidx] && buffers[H.bidx + 1] && side[H.bidx], "mi3d_unet_bn_apply_deferred: missing buffer %d", H.bidx);
            J.j[J.n++] = BnDeferJob{(float*)buffers[H.bidx], (float*)buffers[H.bidx + 1], (int64_t*)buffers[H.bidx + 2],
                                    (const double*)side[H.bidx], H.Cout};
        }
    return bn_deferred_apply(J, (hipStream_t)stream);
}

int mi3d_unet_infer(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* buffers,
                    float* logits, float* gap_out, void* workspace, size_t workspace_bytes, void* stream) {
    Plan p;
    Ctx c{p};
    MI3D_TRY(enter(c, p, d, "mi3d_unet_infer", x && buffers, params, workspace, workspace_bytes, stream));
    int L = p.L;
    if (d->in_channels > 1)
        MI3D_TRY(ncdhw_to_ndhwc(p.dt, x, c.at(p.xcl), d->in_channels, d->in_channels, d->N, p.geo[0].V(), c.s));
    {   // launch 1: every BatchNorm folded; launch 2: every MFMA weight pack, BatchNorm scale multiplied in
        BnFoldJobs F;
        F.n = 0; F.eps = d->bn_eps;
        for (int b = 0; b < p.nblk; b++)
            for (int h = 0; h < 2; h++) {
                const HalfP& H = p.blk[b].h[h];
                MI3D_CHECK_ARG(buffers[H.bidx] && buffers[H.bidx + 1], "mi3d_unet_infer needs running statistics");
                float* scale = c.at<float>(H.stat);
                F.j[F.n++] = BnFoldJob{c.P(H.pidx + 2), c.P(H.pidx + 3), (const float*)buffers[H.bidx], (const float*)buffers[H.bidx + 1],
                                       c.P(H.pidx + 1), scale, scale + H.Cout, H.Cout};
            }
        PackJobs J;
        J.n = 0; J.nblocks = 0;
        MI3D_TRY(add_pack_jobs(c, J, true));
        MI3D_TRY(bn_fold_all(F, c.s));
        MI3D_TRY(pack_all_launch(J, c.s));
    }
    for (int l = 0; l < L; l++) {
        MI3D_TRY(block_infer(c, l, x));
        MI3D_TRY(maxpool2_fwd(p.dt, c.at(p.cat[l]), p.catcs(l), p.C[l], p.geo[l], c.at(p.pool[l]), p.C[l], c.s));
    }
    MI3D_TRY(block_infer(c, L, x));
    if (gap_out) MI3D_TRY(gap_fwd(p.dt, c.at(p.zb), p.C[L], p.C[L], d->N, p.geo[L].V(), gap_out, c.s));
    for (int i = 0; i < L; i++) {
        MI3D_TRY(up_forward(c, i));
        MI3D_TRY(block_infer(c, L + 1 + i, x));
    }
    if (logits)
        MI3D_TRY(conv1_fwd(p.dt, c.at(p.zd[L - 1]), p.C[0], p.C[0], c.P(p.final_pidx()), c.P(p.final_pidx() + 1), logits,
                           d->out_channels, d->N, p.geo[0].V(), c.s));
    return 0;
}

}  // extern "C"

// Exchange marks (data parallel): "record this event once every gradient of the segments <= seg is complete".  Set by
// mi3d_unet_backward_marks for the NEXT backward call of the calling thread; that call stays ONE run of launches (a weight-gradient
// slab sum of segment seg rides in the first BatchNorm-backward reduction of segment seg + 1, and the event is recorded right
// behind that launch) instead of being cut into two calls at the exchange.
struct BwdMarks { int n = 0; int seg[4]; hipEvent_t ev[4]; };
static thread_local BwdMarks g_marks;
extern "C" int mi3d_unet_backward_marks(const int* segs, void* const* events, int n) {
    MI3D_CHECK_ARG(n >= 0 && n <= 4 && (n == 0 || (segs && events)), "mi3d_unet_backward_marks: at most 4 marks");
    g_marks.n = n;
    for (int i = 0; i < n; i++) { g_marks.seg[i] = segs[i]; g_marks.ev[i] = (hipEvent_t)events[i]; }
    return 0;
}
extern "C" int mi3d_stream_wait_event(void* stream, void* event) {
    MI3D_CHECK_ARG(event, "mi3d_stream_wait_event: null event");
    MI3D_HIP(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
    return 0;
}

static int unet_backward_impl(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* grads,
                       const float* drop_scales, const float* dlogits_in, const float* dgap, float gap_scale, int accumulate,
                       int seg_begin, int seg_end, void* workspace, size_t workspace_bytes, void* stream, void* aux_stream,
                       void* const* events, int aux_join, const HeadLoss* hl) {
    Plan p;
    Ctx c{p};
    MI3D_TRY(enter(c, p, d, "mi3d_unet_backward", x && grads, params, workspace, workspace_bytes, stream));
    // `dlogits` below only says "the segmentation branch has a gradient": with the fused head it is never dereferenced
    const float* dlogits = hl ? reinterpret_cast<const float*>(hl->coef) : dlogits_in;
    MI3D_CHECK_ARG(dlogits || dgap, "mi3d_unet_backward: neither dlogits nor dgap given");
    int L = p.L, nseg = 2 * L + 2;
    MI3D_CHECK_ARG(seg_begin >= 0 && seg_end <= nseg && seg_begin <= seg_end, "bad segment range [%d,%d)", seg_begin, seg_end);
    if (aux_stream && events) { c.s2 = (hipStream_t)aux_stream; c.ev = (hipEvent_t*)events; }
    float* wgws = c.at<float>(p.wgws);
    auto G = [&](int i) { return (float*)grads[i]; };
    BwdMarks marks = g_marks;
    g_marks.n = 0;
    for (int seg = seg_begin; seg < seg_end; seg++) {
        if (seg > seg_begin)
            for (int i = 0; i < marks.n; i++)
                if (marks.seg[i] == seg - 1) MI3D_TRY(c.pending.set_mark(marks.ev[i], c.s));
        if (seg == 0) {
            if (!dlogits) continue;
            SlabJob* ps = c.pending.first(c.s);
            if (hl) {
                MI3D_CHECK_ARG(head_loss_bwd_ok(p.dt, c.at(p.zd[L - 1]), p.C[0], p.C[0], d->out_channels, hl->cfg, c.at(p.gz[0]), p.C[0]),
                               "mi3d_unet_backward_loss: no fused head + loss for this configuration (see mi3d_unet_head_loss_supported)");
                MI3D_TRY(head_loss_bwd(c.at(p.zd[L - 1]), p.C[0], p.C[0], c.P(p.final_pidx()), c.P(p.final_pidx() + 1), hl->labels,
                                       hl->teacher, d->out_channels, hl->cfg, hl->coef, hl->grad_scale, c.at(p.gz[0]), p.C[0], G(p.final_pidx()),
                                       G(p.final_pidx() + 1), accumulate, wgws, d->N, p.geo[0].V(), c.s, ps));
            } else
                MI3D_TRY(conv1_bwd(p.dt, c.at(p.zd[L - 1]), p.C[0], p.C[0], c.P(p.final_pidx()), dlogits, d->out_channels,
                                   c.at(p.gz[0]), p.C[0], G(p.final_pidx()), G(p.final_pidx() + 1), accumulate, wgws, d->N,
                                   p.geo[0].V(), c.s, ps));
        } else if (seg <= L) {
            if (!dlogits) continue;
            int l = seg - 1, i = L - 1 - l;       // decoder.i works at level l
            MI3D_TRY(block_backward(c, L + 1 + i, x, grads, drop_scales, c.at(p.gz[l]), p.C[l], c.at(p.gcat[l]), p.catcs(l), accumulate));
            const UpIO u = up_io(c, i);
            UpHalfBwd a{u.Cin, u.Cout, u.g, p.dt, p.up_mfma[i], u.in, u.Cin, u.w, u.wb, c.at<char>(p.gcat[l]) + u.half, u.cs, p.geo[l],
                        p.resize[l] ? c.at(p.uptmp) : nullptr, c.at(p.gz[l + 1]), u.Cin, G(p.up_pidx(i)), G(p.up_pidx(i) + 1), accumulate,
                        wgws, c.at<float>(p.wgws2), p.wgws_floats, true};
            MI3D_TRY(up_half_backward(a, c.pending, c.s));
        } else if (seg == L + 1) {
            if (dgap)
                MI3D_TRY(gap_bwd(p.dt, dgap, gap_scale, c.at(p.gz[L]), p.C[L], p.C[L], d->N, p.geo[L].V(), dlogits ? 1 : 0, c.s));
            // (the gradient of the pooled tensor may stay split-K partials when the MaxPool3d backward that reads it is launched
            // by this very call: a later call would not know about them)
            c.pool_defer = seg + 1 < seg_end && !mi3d_routes().no_pool_splitk;
            MI3D_TRY(block_backward(c, L, x, grads, drop_scales, c.at(p.gz[L]), p.C[L], c.at(p.gp[L - 1]), p.C[L - 1], accumulate));
            c.pool_defer = false;
        } else {
            int l = 2 * L + 1 - seg;              // encoder.l
            MI3D_TRY(maxpool2_bwd(p.dt, c.at(p.gp[l]), p.C[l], c.at(p.cat[l]), p.catcs(l), dlogits ? c.at(p.gcat[l]) : nullptr,
                                  p.catcs(l), c.at(p.gz[l]), p.C[l], p.C[l], p.geo[l], c.s,
                                  c.pool_ks > 0 ? c.at<float>(p.skws) : nullptr, c.pool_ks));
            c.pool_ks = 0;
            void* dx = l > 0 ? c.at(p.gp[l - 1]) : nullptr;
            c.pool_defer = l > 0 && seg + 1 < seg_end && !mi3d_routes().no_pool_splitk;
            MI3D_TRY(block_backward(c, l, x, grads, drop_scales, c.at(p.gz[l]), p.C[l], dx, l > 0 ? p.C[l - 1] : 0, accumulate));
            c.pool_defer = false;
        }
    }
    MI3D_TRY(c.pending.finish(c.s));
    for (int i = 0; i < marks.n; i++)
        if (marks.seg[i] == seg_end - 1) MI3D_HIP(hipEventRecord(marks.ev[i], c.s));
    // weight gradients still queued (a call that ends before the group's own fork point): they go out now, so that every
    // gradient of the segments [seg_begin, seg_end) is at least in flight when the call returns
    if (c.s2 && c.ev) {
        MI3D_TRY(flush_deferred(c, x, grads, accumulate));
        MI3D_TRY(drain_aux(c, x, grads, accumulate, -1));
    }
    if (c.aux_used) {
        // event 3 = "the aux stream has finished what this call gave it".  aux_join: the compute stream waits for it here, i.e.
        // everything is ordered before whatever the caller enqueues next on `stream`; otherwise the CALLER orders its consumers
        // (optimizer, gradient exchange, the end of a graph capture) after event 3 / the aux stream
        MI3D_HIP(hipEventRecord(c.ev[3], c.s2));
        if (aux_join) MI3D_HIP(hipStreamWaitEvent(c.s, c.ev[3], 0));
    }
    return 0;
}

extern "C" {

int mi3d_unet_backward(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* grads,
                       const float* drop_scales, const float* dlogits, const float* dgap, float gap_scale, int accumulate,
                       int seg_begin, int seg_end, void* workspace, size_t workspace_bytes, void* stream, void* aux_stream,
                       void* const* events, int aux_join) {
    return unet_backward_impl(d, x, params, grads, drop_scales, dlogits, dgap, gap_scale, accumulate, seg_begin, seg_end, workspace,
                              workspace_bytes, stream, aux_stream, events, aux_join, nullptr);
}

int mi3d_unet_backward_loss(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* grads,
                            const float* drop_scales, const int64_t* labels, const float* teacher_logits, const mi3d_loss_cfg* cfg,
                            const float* coef, const float* grad_scale, const float* dgap, float gap_scale, int accumulate, int seg_begin,
                            int seg_end, void* workspace, size_t workspace_bytes, void* stream, void* aux_stream, void* const* events,
                            int aux_join) {
    MI3D_CHECK_ARG(labels && cfg && coef, "mi3d_unet_backward_loss: null pointer");
    HeadLoss hl{labels, cfg_of(cfg), nullptr, const_cast<float*>(coef), nullptr, nullptr, nullptr, grad_scale, teacher_logits};
    return unet_backward_impl(d, x, params, grads, drop_scales, nullptr, dgap, gap_scale, accumulate, seg_begin, seg_end, workspace,
                              workspace_bytes, stream, aux_stream, events, aux_join, &hl);
}
int mi3d_unet_backward_loss_masked(const mi3d_unet_desc* d, const float* x, const void* const* params, void* const* grads,
                                   const float* drop_scales, const int64_t* labels, const float* teacher_logits,
                                   const mi3d_loss_cfg* cfg, int64_t ignore_index, const float* coef, const float* grad_scale,
                                   const float* dgap, float gap_scale, int accumulate, int seg_begin, int seg_end, void* workspace,
                                   size_t workspace_bytes, void* stream, void* aux_stream, void* const* events, int aux_join) {
    MI3D_CHECK_ARG(labels && cfg && coef, "mi3d_unet_backward_loss_masked: null pointer");
    MI3D_MASKED_CFG(k, cfg, ignore_index, "mi3d_unet_backward_loss_masked");
    HeadLoss hl{labels, k, nullptr, const_cast<float*>(coef), nullptr, nullptr, nullptr, grad_scale, teacher_logits};
    return unet_backward_impl(d, x, params, grads, drop_scales, nullptr, dgap, gap_scale, accumulate, seg_begin, seg_end, workspace,
                              workspace_bytes, stream, aux_stream, events, aux_join, &hl);
}

}  // extern "C"
