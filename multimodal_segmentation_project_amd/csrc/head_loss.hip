// head_loss.hip — final 1x1x1 conv (channels-last -> NCDHW fp32 logits), the segmentation loss family and
// the per-step metrics.  All HBM-bound single-pass kernels with two-stage deterministic reductions.
//
// Reference: nn.Conv3d(features[0], out_channels, 1)  models/unet.py:62,87
//            combined_loss / tversky_loss / combined_ce_tversky_loss / distillation_loss  utils/metrics.py:14-40,137-190
//            'dice' variant train_unet.py:186-198
//            calculate_iou / calculate_dice / calculate_accuracy  utils/metrics.py:65-129 (incl. quirk Q1)
//
// Loss family (one parametrisation, see LossCfg):
//   L = w_ce*CE + w_reg*mean_{c>=1} R_c + w_kd*T^2*mean_{n,c,v} KL(p_t^T || p_s^T)
//   dL/dz_k = w_ce/M (p_k - [t=k]) + p_k (g_k - sum_c g_c p_c) + w_kd*T/(M*C) (ps_k - pt_k),
//   g_c = w_reg/(C-1) * (A_c [t=c] + B_c),  A_c, B_c = dR_c/dI_c-ish coefficients computed once from the sums.
#include <type_traits>

#include "../../include/mi3d.h"
#include "mfma_tile.h"
#include "ops.h"

int slab_reduce(const float* slabs, int nslab, int64_t slab_sz, int64_t nW, float* dW, float* db, int accumulate,
                hipStream_t s);

namespace {
constexpr int BLK = 256;
constexpr int MAXC = MI3D_MAX_CLASSES;
constexpr int CINB = 16;    // input-channel block of the 1x1x1 conv kernels
constexpr int LOSS_MAXBLK = 512;

// ------------------------------------------------------------------------------------------ conv 1x1x1
template <typename T, bool VEC>
__device__ __forceinline__ void load_cin_block(const T* zp, int nci, float (&zv)[CINB]) {
    if constexpr (VEC) {
        float a[8], b[8];
        ld8<T>(zp, a);
        ld8<T>(zp + 8, b);
#pragma unroll
        for (int i = 0; i < 8; i++) { zv[i] = a[i]; zv[8 + i] = b[i]; }
    } else {
#pragma unroll
        for (int i = 0; i < CINB; i++) zv[i] = i < nci ? to_f<T>(zp[i]) : 0.f;
    }
}

// The logits of ONE voxel, classes co0 .. co0 + nco - 1: acc[j] = bias[co0 + j], then fmaf(z[ci], w[co][ci], acc[j]) over ci in
// ascending order.  The one place where the bits of a logit are decided: conv1_fwd_kernel stores what this returns and
// head_labels_kernel takes its argmax, so a label is the first maximum of exactly the logits the head would have written.
template <typename T, bool VEC, int NCO>
__device__ __forceinline__ void conv1_voxel(const T* __restrict__ zrow, int Cin, const float* __restrict__ w,
                                            const float* __restrict__ bias, int co0, int nco, float (&acc)[NCO]) {
#pragma unroll
    for (int j = 0; j < NCO; j++) acc[j] = (bias && j < nco) ? bias[co0 + j] : 0.f;
    for (int c0 = 0; c0 < Cin; c0 += CINB) {
        int nci = min(CINB, Cin - c0);
        float zv[CINB];
        load_cin_block<T, VEC>(zrow + c0, nci, zv);
#pragma unroll
        for (int j = 0; j < NCO; j++) {
            if (j < nco) {
#pragma unroll
                for (int i = 0; i < CINB; i++)
                    if (VEC || i < nci) acc[j] = fmaf(zv[i], w[(int64_t)(co0 + j) * Cin + c0 + i], acc[j]);
            }
        }
    }
}

// logits[n][co][v] = bias[co] + sum_ci z[n,v,ci] * w[co][ci]       (Cout <= NCO per blockIdx.z group)
// grid = (blocks over voxel groups, N, cout groups); a thread owns VV consecutive voxels of one sample so the fp32
// class planes are written as 16-byte stores and no per-voxel 64-bit division is needed.
template <typename T, bool VEC, int NCO, int VV>
__global__ __launch_bounds__(BLK) void conv1_fwd_kernel(const T* __restrict__ z, int zcs, int Cin, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ logits, int Cout,
                                                        int64_t V) {
    int n = blockIdx.y;
    int co0 = blockIdx.z * NCO;
    int nco = min(NCO, Cout - co0);
    const T* zn = z + (int64_t)n * V * zcs;
    float* ln = logits + ((int64_t)n * Cout + co0) * V;
    int64_t ngrp = V / VV;
    for (int64_t grp = (int64_t)blockIdx.x * BLK + threadIdx.x; grp < ngrp; grp += (int64_t)gridDim.x * BLK) {
        int64_t v0 = grp * VV;
        float acc[VV][NCO];
#pragma unroll
        for (int k = 0; k < VV; k++) conv1_voxel<T, VEC, NCO>(zn + (v0 + k) * zcs, Cin, w, bias, co0, nco, acc[k]);
#pragma unroll
        for (int j = 0; j < NCO; j++) {
            if (j < nco) {
                if constexpr (VV == 4) *reinterpret_cast<float4*>(ln + (int64_t)j * V + v0) = float4{acc[0][j], acc[1][j], acc[2][j], acc[3][j]};
                else ln[(int64_t)j * V + v0] = acc[0][j];
            }
        }
    }
}

// per block (blockIdx.z = 16-channel input block): dz[v][ci] = sum_co dl[co][v] w[co][ci];
// slab[blockIdx.y * gridDim.x + blockIdx.x] = { dW[co][ci] partial, db[co] partial }
template <typename T, bool VEC, int NCO, int VV>
__global__ __launch_bounds__(BLK) void conv1_bwd_kernel(const T* __restrict__ z, int zcs, int Cin, const float* __restrict__ w,
                                                        const float* __restrict__ dl, int Cout, T* __restrict__ dz, int dzcs,
                                                        int64_t V, float* __restrict__ slabs) {
    __shared__ float red[4][NCO * CINB + NCO];
    int n = blockIdx.y;
    int c0 = blockIdx.z * CINB;
    int nci = min(CINB, Cin - c0);
    const T* zn = z + (int64_t)n * V * zcs + c0;
    T* dzn = dz ? dz + (int64_t)n * V * dzcs + c0 : nullptr;
    const float* dln = dl + (int64_t)n * Cout * V;
    float aw[NCO][CINB], ab[NCO], wr[NCO][CINB];
#pragma unroll
    for (int j = 0; j < NCO; j++) {
        ab[j] = 0.f;
#pragma unroll
        for (int i = 0; i < CINB; i++) { aw[j][i] = 0.f; wr[j][i] = (j < Cout && i < nci) ? w[(int64_t)j * Cin + c0 + i] : 0.f; }
    }
    int64_t ngrp = V / VV;
    for (int64_t grp = (int64_t)blockIdx.x * BLK + threadIdx.x; grp < ngrp; grp += (int64_t)gridDim.x * BLK) {
        int64_t v0 = grp * VV;
        float g[NCO][VV];
#pragma unroll
        for (int j = 0; j < NCO; j++) {
            if (j < Cout) {
                if constexpr (VV == 4) {
                    float4 t = *reinterpret_cast<const float4*>(dln + (int64_t)j * V + v0);
                    g[j][0] = t.x; g[j][1] = t.y; g[j][2] = t.z; g[j][3] = t.w;
                } else g[j][0] = dln[(int64_t)j * V + v0];
            } else {
#pragma unroll
                for (int k = 0; k < VV; k++) g[j][k] = 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < VV; k++) {
            float zv[CINB], o[CINB];
            load_cin_block<T, VEC>(zn + (v0 + k) * zcs, nci, zv);
#pragma unroll
            for (int i = 0; i < CINB; i++) o[i] = 0.f;
#pragma unroll
            for (int j = 0; j < NCO; j++) {
                ab[j] += g[j][k];
#pragma unroll
                for (int i = 0; i < CINB; i++) {
                    aw[j][i] = fmaf(g[j][k], zv[i], aw[j][i]);
                    o[i] = fmaf(g[j][k], wr[j][i], o[i]);
                }
            }
            if (dzn) {
                if constexpr (VEC) {
                    float lo[8], hi[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) { lo[i] = o[i]; hi[i] = o[8 + i]; }
                    st8<T>(dzn + (v0 + k) * dzcs, lo);
                    st8<T>(dzn + (v0 + k) * dzcs + 8, hi);
                } else {
#pragma unroll
                    for (int i = 0; i < CINB; i++) if (i < nci) dzn[(v0 + k) * dzcs + i] = from_f<T>(o[i]);
                }
            }
        }
    }
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < NCO; j++) {
#pragma unroll
        for (int i = 0; i < CINB; i++) {
            float sv = wave_sum(aw[j][i]);
            if (lane == 0) red[wave][j * CINB + i] = sv;
        }
        float sb = wave_sum(ab[j]);
        if (lane == 0) red[wave][NCO * CINB + j] = sb;
    }
    __syncthreads();
    int64_t nW = (int64_t)Cout * Cin;
    float* slab = slabs + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (nW + Cout);
    for (int idx = threadIdx.x; idx < NCO * CINB + NCO; idx += BLK) {
        float sv = red[0][idx] + red[1][idx] + red[2][idx] + red[3][idx];
        if (idx < NCO * CINB) {
            int j = idx / CINB, i = idx - j * CINB;
            if (j < Cout && i < nci) slab[(int64_t)j * Cin + c0 + i] = sv;
        } else {
            int j = idx - NCO * CINB;
            if (j < Cout && blockIdx.z == 0) slab[nW + j] = sv;
        }
    }
}

// ---- bf16 fast path of the backward (Cout <= 8, 16-channel input blocks): both contractions on the matrix cores.
// The scalar kernel above spends 128 FMAs + conversions per voxel (VALU-bound: 40 us at 96^3 N=2 for 18 us of traffic).
//   dz[v][ci] = sum_co dl[co][v] w[co][ci]   : A = w^T (16 ci x 32 k), class j sits at k = 8*(j&3) + (j>>2), rest zero;
//                                               B = dl: lane (voxel n, k-group kg) supplies dl[kg (+4)][v_n]  -> one
//                                               scalar load per lane and class slot, no gather
//   dW[co][ci] = sum_v dl[co][v] z[v][ci]    : K = 32 voxels; A = z^T via the transposing LDS read of the wave's own
//                                               32 x 16 tile, B = dl: lane (co = n, kg) supplies 8 consecutive voxels
//                                               of class n (two float4 loads); result rows = ci, columns = co
// A wave owns 32 consecutive voxels per iteration; workgroup = 4 waves; slab layout as the scalar kernel.
constexpr int C1W = 8;          // waves per workgroup: one slab per workgroup, so more waves = same parallelism with fewer slabs
__global__ __launch_bounds__(C1W * 64) void conv1_bwd_mfma_kernel(const bf16* __restrict__ z, int zcs, int Cin, const float* __restrict__ w,
                                                             const float* __restrict__ dl, int Cout, bf16* __restrict__ dz, int dzcs,
                                                             int64_t V, float* __restrict__ slabs) {
    __shared__ __attribute__((aligned(16))) bf16 zt[C1W][32 * 16];
    __shared__ float red[C1W][64][4];
    __shared__ float redb[C1W][16];
    int n = blockIdx.y, c0 = blockIdx.z * 16;
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int vn = lane & 15, kg = lane >> 4;
    const bf16* zn = z + (int64_t)n * V * zcs + c0;
    bf16* dzn = dz ? dz + (int64_t)n * V * dzcs + c0 : nullptr;
    const float* dln = dl + (int64_t)n * Cout * V;
    // A fragment of the dz product: lane (m = ci = vn, kg): slot s holds w[kg + 4 s][ci]
    bf16x8 aw;
#pragma unroll
    for (int j = 0; j < 8; j++) aw[j] = (bf16)0.f;
    aw[0] = (bf16)(kg < Cout ? w[(int64_t)kg * Cin + c0 + vn] : 0.f);
    aw[1] = (bf16)(kg + 4 < Cout ? w[(int64_t)(kg + 4) * Cin + c0 + vn] : 0.f);
    f32x4 accW = {0.f, 0.f, 0.f, 0.f};
    float dbs = 0.f;
    const char* ztb = reinterpret_cast<const char*>(zt[wave]);
    int laneK = ((8 * kg + ((lane & 15) >> 2)) * 16 + 4 * (lane & 3)) * 2;
    for (int64_t v0 = ((int64_t)blockIdx.x * C1W + wave) * 32; v0 < V; v0 += (int64_t)gridDim.x * (C1W * 32)) {
        // stage this wave's 32 x 16 z tile (zero rows beyond V)
        {
            int64_t v = v0 + (lane >> 1);
            bf16x8 t = {0, 0, 0, 0, 0, 0, 0, 0};
            if (v < V) t = *reinterpret_cast<const bf16x8*>(zn + v * zcs + (lane & 1) * 8);
            *reinterpret_cast<bf16x8*>(zt[wave] + (lane >> 1) * 16 + (lane & 1) * 8) = t;
        }
        // dW: B = dl, 8 consecutive voxels of class vn
        bf16x8 bd = {0, 0, 0, 0, 0, 0, 0, 0};
        if (vn < Cout) {
            int64_t vb = v0 + 8 * kg;
            float t8[8];
            if (vb + 8 <= V && ((V & 3) == 0)) {
                float4 p = *reinterpret_cast<const float4*>(dln + (int64_t)vn * V + vb), q = *reinterpret_cast<const float4*>(dln + (int64_t)vn * V + vb + 4);
                t8[0] = p.x; t8[1] = p.y; t8[2] = p.z; t8[3] = p.w; t8[4] = q.x; t8[5] = q.y; t8[6] = q.z; t8[7] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) t8[j] = (vb + j < V) ? dln[(int64_t)vn * V + vb + j] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 8; j++) { bd[j] = (bf16)t8[j]; dbs += t8[j]; }
        }
        // dz: two 16-voxel blocks
#pragma unroll
        for (int nb = 0; nb < 2; nb++) {
            int64_t v = v0 + nb * 16 + vn;
            bf16x8 bl = {0, 0, 0, 0, 0, 0, 0, 0};
            if (v < V) {
                if (kg < Cout) bl[0] = (bf16)dln[(int64_t)kg * V + v];
                if (kg + 4 < Cout) bl[1] = (bf16)dln[(int64_t)(kg + 4) * V + v];
            }
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw, bl, o, 0, 0, 0);
            if (dzn && v < V) {
                bf16x4 ob = {(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
                *reinterpret_cast<bf16x4*>(dzn + v * dzcs + 4 * kg) = ob;
            }
        }
        // the tile is private to this wave: LDS writes above are complete for the wave before the transposing read
        __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0)
        __builtin_amdgcn_wave_barrier();
        bf16x8 az = tr_frag(ztb, laneK);
        accW = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az, bd, accW, 0, 0, 0);
        __builtin_amdgcn_wave_barrier();
    }
    // accW: rows ci = 4*kg + r, column co = vn.  Cross-wave sum, then the slab of this block
    *reinterpret_cast<f32x4*>(&red[wave][lane][0]) = accW;
    float sb = dbs;
    sb += __shfl_xor(sb, 16, 64);
    sb += __shfl_xor(sb, 32, 64);
    if (lane < 16) redb[wave][lane] = sb;
    __syncthreads();
    int64_t nW = (int64_t)Cout * Cin;
    float* slab = slabs + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (nW + Cout);
    if (threadIdx.x < 64) {
        int l = threadIdx.x, co = l & 15, g4 = l >> 4;
        if (co < Cout) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float sv = 0.f;
#pragma unroll
                for (int wv = 0; wv < C1W; wv++) sv += red[wv][l][r];
                slab[(int64_t)co * Cin + c0 + 4 * g4 + r] = sv;
            }
        }
    } else if (threadIdx.x < 64 + 16) {
        int co = threadIdx.x - 64;
        if (co < Cout && blockIdx.z == 0) {
            float sv = 0.f;
#pragma unroll
            for (int wv = 0; wv < C1W; wv++) sv += redb[wv][co];
            slab[nW + co] = sv;
        }
    }
}

// ---------------------------------------------------------------------------------------- seg loss
// per-voxel softmax helpers (C <= NC, fully unrolled with predicates)
template <int NC>
__device__ __forceinline__ void softmax_c(const float (&z)[NC], int C, float inv_t, float (&p)[NC], float& lse) {
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < NC; c++) if (c < C) mx = fmaxf(mx, z[c] * inv_t);
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < NC; c++) { p[c] = c < C ? __expf(z[c] * inv_t - mx) : 0.f; se += p[c]; }
    float r = __builtin_amdgcn_rcpf(se);          // 1 ulp; the IEEE division costs ~10 VALU slots per voxel in VALU-bound passes
#pragma unroll
    for (int c = 0; c < NC; c++) p[c] *= r;
    lse = mx + __logf(se);
}

// VV consecutive voxels of one sample: class planes as 16-byte loads (VV = 4) -- grid = (blocks, N), no per-voxel
// 64-bit division
template <int NC, int VV>
__device__ __forceinline__ void load_planes(const float* __restrict__ base, int C, int64_t V, int64_t v0, float (&z)[VV][NC]) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
        if (c < C) {
            if constexpr (VV == 4) {
                float4 t = *reinterpret_cast<const float4*>(base + (int64_t)c * V + v0);
                z[0][c] = t.x; z[1][c] = t.y; z[2][c] = t.z; z[3][c] = t.w;
            } else z[0][c] = base[(int64_t)c * V + v0];
        } else {
#pragma unroll
            for (int k = 0; k < VV; k++) z[k][c] = 0.f;
        }
    }
}
template <int VV>
__device__ __forceinline__ void load_labels(const int64_t* __restrict__ lb, int (&t)[VV]) {
    if constexpr (VV == 4) {
        longlong2 a = *reinterpret_cast<const longlong2*>(lb), b = *reinterpret_cast<const longlong2*>(lb + 2);
        t[0] = (int)a.x; t[1] = (int)a.y; t[2] = (int)b.x; t[3] = (int)b.y;
    } else t[0] = (int)lb[0];
}

constexpr int NQ = 2 + 3 * MAXC;   // ce, kl, I[c], P[c], T[c]

// METRICS: the same pass also produces the argmax / label count partials of seg_metrics_kernel (the training step needs
// both on the same logits: one read of logits + labels instead of two).
// The pass is VALU-bound (4 classes: softmax + per-class sums + argmax per voxel), so what can leave the vector unit does:
// EXACT (C == NC) drops every `c < C` predicate, TEACH compiles the distillation term in or out, and the integer counts
// (label histogram, argmax histogram, intersections) are wave ballots + scalar popcounts — the vector unit only does the
// compares.  T[c] = sum [t == c] is taken from the exact label histogram instead of a float accumulator.
// MASK (the *_masked entries, contract: include/mi3d.h): a voxel whose label is `ign` becomes the label -1, which matches no class
// in the I sums and the ballots, and its CE term, its P terms and its argmax are selected away; the distillation term stays.
// The selects add no rounding, and the label histogram stays exact, so M_valid = sum_c T[c] reaches loss_scalars as an integer.
template <int NC, int VV, bool METRICS, bool EXACT, bool TEACH, bool MASK>
__global__ __launch_bounds__(BLK) void seg_loss_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ teacher, int C_, int64_t V,
                                                           float inv_t, double* __restrict__ part,
                                                           unsigned long long* __restrict__ counts, int ign) {
    const int C = EXACT ? NC : C_;
    constexpr int NQL = 2 + 3 * NC;
    __shared__ float red[4][NQL];
    __shared__ unsigned redc[4][3 * NC + 1];
    unsigned ni[NC], np[NC], nt[NC];                 // wave-uniform (scalar registers)
#pragma unroll
    for (int c = 0; c < NC; c++) ni[c] = np[c] = nt[c] = 0;
    int n = blockIdx.y;
    const float* lg = logits + (int64_t)n * C * V;
    const float* tg = TEACH ? teacher + (int64_t)n * C * V : nullptr;
    const int64_t* lb = labels + (int64_t)n * V;
    float q[2 + 2 * NC];                             // ce, kl, I[c], P[c]
#pragma unroll
    for (int i = 0; i < 2 + 2 * NC; i++) q[i] = 0.f;
    int64_t ngrp = V / VV;
    for (int64_t grp = (int64_t)blockIdx.x * BLK + threadIdx.x; grp < ngrp; grp += (int64_t)gridDim.x * BLK) {
        int64_t v0 = grp * VV;
        float z[VV][NC];
        int t[VV];
        load_planes<NC, VV>(lg, C, V, v0, z);
        load_labels<VV>(lb + v0, t);
        float zt_[VV][NC];
        if constexpr (TEACH) load_planes<NC, VV>(tg, C, V, v0, zt_);
#pragma unroll
        for (int k = 0; k < VV; k++) {
            float p[NC], lse;
            softmax_c<NC>(z[k], C, 1.f, p, lse);
            bool scored = true;
            if constexpr (MASK) {
                scored = t[k] != ign;
                t[k] = scored ? t[k] : -1;
            }
            float zt = 0.f;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (EXACT || c < C) {
                    bool is = (c == t[k]);
                    zt = is ? z[k][c] : zt;
                    q[2 + c] += is ? p[c] : 0.f;
                    if constexpr (MASK) q[2 + NC + c] += scored ? p[c] : 0.f;
                    else q[2 + NC + c] += p[c];
                }
            }
            if constexpr (MASK) q[0] += scored ? lse - zt : 0.f;
            else q[0] += lse - zt;
            {
                float bvv = z[k][0];
                int best = 0;
#pragma unroll
                for (int c = 1; c < NC; c++)
                    if ((EXACT || c < C) && z[k][c] > bvv) { bvv = z[k][c]; best = c; }
                if constexpr (MASK) best = scored ? best : -1;
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    unsigned long long mt = __ballot(t[k] == c);
                    nt[c] += (unsigned)__popcll(mt);
                    if constexpr (METRICS) {
                        unsigned long long mb = __ballot(best == c);
                        np[c] += (unsigned)__popcll(mb);
                        ni[c] += (unsigned)__popcll(mb & mt);
                    }
                }
            }
            if constexpr (TEACH) {
                float ps[NC], pt[NC], ls, lt;
                softmax_c<NC>(z[k], C, inv_t, ps, ls);
                softmax_c<NC>(zt_[k], C, inv_t, pt, lt);
                float kl = 0.f;
#pragma unroll
                for (int c = 0; c < NC; c++)
                    if ((EXACT || c < C) && pt[c] > 0.f) kl += pt[c] * ((zt_[k][c] * inv_t - lt) - (z[k][c] * inv_t - ls));
                q[1] += kl;
            }
        }
    }
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < 2 + 2 * NC; i++) {
        float sv = wave_sum(q[i]);
        if (lane == 0) red[wave][i] = sv;
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            red[wave][2 + 2 * NC + c] = (float)nt[c];                     // exact: a wave sees < 2^24 voxels per block
            redc[wave][c] = ni[c]; redc[wave][NC + c] = np[c]; redc[wave][2 * NC + c] = nt[c];
        }
    }
    __syncthreads();
    // partial rows are COMPACT: 2 + 3C doubles (ce, kl, I[c], P[c], T[c]) and 3C + 1 counts — the single finalize
    // workgroup is bound by pulling the rows through one CU
    const int nqc = 2 + 3 * C;
    if ((int)threadIdx.x < nqc) {
        int i = threadIdx.x, src = i;
        if (i >= 2) { int k = (i - 2) / C, c = (i - 2) % C; src = 2 + k * NC + c; }
        double v = (double)red[0][src] + (double)red[1][src] + (double)red[2][src] + (double)red[3][src];
        part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nqc + i] = v;
    }
    if constexpr (METRICS) {
        if ((int)threadIdx.x < 3 * C + 1) {
            int i = threadIdx.x;
            unsigned long long v = 0;
            if (i < 3 * C) {
                int src = (i / C) * NC + (i % C);
                v = (unsigned long long)redc[0][src] + redc[1][src] + redc[2][src] + redc[3][src];
            } else {                                            // n_correct = sum_c n_inter[c]
#pragma unroll
                for (int c = 0; c < NC; c++) v += (unsigned long long)redc[0][c] + redc[1][c] + redc[2][c] + redc[3][c];
            }
            counts[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (3 * C + 1) + i] = v;
        }
    }
}

__device__ __forceinline__ void loss_row_sum(const double* __restrict__ part, int nblk, int C, int q, int lane, double* sums);
__device__ __forceinline__ void loss_scalars(const double* sums, int N, int C, int64_t V, LossCfg cfg, float* loss_out, float* coef);
// one 1024-thread block: wave w sums quantities w, w+16 over the block partials (lane-strided doubles + wave tree:
// fixed order), then thread 0 computes the loss and the gradient coefficients
__device__ __forceinline__ void seg_loss_finalize_body(const double* __restrict__ part, int nblk, int N, int C,
                                                       int64_t V, LossCfg cfg, float* loss_out, float* coef) {
    __shared__ double sums[NQ];
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nqc = 2 + 3 * C;
    if (threadIdx.x < NQ) sums[threadIdx.x] = 0.0;
    __syncthreads();
    for (int q = wave; q < nqc; q += 16) loss_row_sum(part, nblk, C, q, lane, sums);
    __syncthreads();
    if (threadIdx.x == 0) loss_scalars(sums, N, C, V, cfg, loss_out, coef);
}

// quantity q of the compact partial rows, summed by one wave (lane-strided doubles + wave tree: fixed order) into the MAXC layout
__device__ __forceinline__ void loss_row_sum(const double* __restrict__ part, int nblk, int C, int q, int lane, double* sums) {
    const int nqc = 2 + 3 * C;
    double s = 0.0;
    for (int b = lane; b < nblk; b += 64) s += part[(int64_t)b * nqc + q];
    s = wave_sum_d(s);
    if (lane == 0) sums[q < 2 ? q : 2 + ((q - 2) / C) * MAXC + (q - 2) % C] = s;
}

__device__ __forceinline__ void loss_scalars(const double* sums, int N, int C, int64_t V, LossCfg cfg, float* loss_out, float* coef) {
    {
        double M = (double)N * (double)V;
        // the divisor of the CE mean: every voxel, or with cfg.mask M_valid = sum_c T_c, the exact label histogram over [0, C)
        // (integers below 2^53 in doubles).  M_valid = 0: the CE sum is an exact 0 and ce_s is set to 0 (mi3d.h: not torch's NaN)
        double Mce = M;
        if (cfg.mask) {
            Mce = 0.0;
            for (int c = 0; c < C; c++) Mce += sums[2 + 2 * MAXC + c];
        }
        const bool none_valid = cfg.mask && Mce == 0.0;
        if (none_valid) Mce = 1.0;
        double reg = 0.0;
        double sc = C > 1 ? (double)cfg.w_reg / (double)(C - 1) : 0.0;
        for (int c = 0; c < MAXC; c++) { coef[c] = 0.f; coef[MAXC + c] = 0.f; }
        for (int c = 1; c < C; c++) {
            double I = sums[2 + c], P = sums[2 + MAXC + c], T = sums[2 + 2 * MAXC + c], eps = cfg.eps;
            double A = 0.0, B = 0.0;
            if (cfg.region_kind == 1) {
                double U = P + T;
                reg += 1.0 - (2.0 * I + eps) / (U + eps);
                A = -2.0 / (U + eps);
                B = (2.0 * I + eps) / ((U + eps) * (U + eps));
            } else if (cfg.region_kind == 2) {
                double fp = P - I, fn = T - I, num = I + eps, den = I + cfg.alpha * fp + cfg.beta * fn + eps;
                reg += 1.0 - num / den;
                A = -(1.0 / den) + num / (den * den) * (1.0 - (double)cfg.alpha - (double)cfg.beta);
                B = num / (den * den) * (double)cfg.alpha;
            }
            coef[c] = (float)(A * sc);
            coef[MAXC + c] = (float)(B * sc);
        }
        if (C > 1) reg /= (double)(C - 1);
        double loss = (double)cfg.w_ce * sums[0] / Mce + (double)cfg.w_reg * reg +
                      (double)cfg.w_kd * (double)cfg.temp * (double)cfg.temp * sums[1] / (M * C);
        coef[2 * MAXC + 0] = none_valid ? 0.f : (float)((double)cfg.w_ce / Mce);
        coef[2 * MAXC + 1] = (float)((double)cfg.w_kd * (double)cfg.temp / (M * C));
        coef[2 * MAXC + 2] = (float)loss;
        coef[2 * MAXC + 3] = 0.f;
        *loss_out = (float)loss;
    }
}

__global__ __launch_bounds__(1024) void seg_loss_finalize_kernel(const double* __restrict__ part, int nblk, int N, int C,
                                                                  int64_t V, LossCfg cfg, float* loss_out, float* coef) {
    seg_loss_finalize_body(part, nblk, N, C, V, cfg, loss_out, coef);
}

// distillation term of dL/dz: kd_s (ps - pt).  ps and pt are products (softmax_c: exp * 1/sum), so under implicit contraction
// the difference becomes fma(e, r, -pt), fma(-et, rt, ps) or a plain subtraction depending on the kernel this is inlined into
// (measured: one ulp between the VV = 4 and VV = 1 instantiations of seg_loss_bwd_kernel at C = 3 with a teacher); as in
// dlogits_voxel the operations are taken as written
template <int NC>
__device__ __forceinline__ void kd_voxel(const float (&ps)[NC], const float (&pt)[NC], float kd_s, float (&kd)[NC]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < NC; c++) kd[c] = kd_s * (ps[c] - pt[c]);
}

// dL/dz of one voxel (header of this file); shared by the plain backward pass and the head-fused one so that both
// produce the same bits from the same logits
template <int NC>
__device__ __forceinline__ void dlogits_voxel(const float (&z)[NC], int t, int C, const float (&A)[NC], const float (&B)[NC],
                                              float ce_s, float go, const float (&kd)[NC], float (&o)[NC]) {
    // no implicit contraction in here: which multiply fuses with which add would otherwise depend on the kernel this is inlined
    // into (measured: one ulp between the two callers at C = 3); the fused multiply-adds are written out
#pragma clang fp contract(off)
    float p[NC], g[NC], lse;
    softmax_c<NC>(z, C, 1.f, p, lse);
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        g[c] = (c == t ? A[c] : 0.f) + B[c];
        dot = fmaf(g[c], p[c], dot);
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        float u = p[c] * (g[c] - dot) + kd[c];
        o[c] = go * fmaf(ce_s, p[c] - (c == t ? 1.f : 0.f), u);
    }
}

// The gradient of a voxel the masked entries ignore: what dlogits_voxel gives with A = B = ce_s = 0, i.e. go * kd[c] (without a
// teacher a zero).  A select per class behind the unchanged expression: the voxels that count keep dlogits_voxel's bits.
template <int NC>
__device__ __forceinline__ void dlogits_ignored(bool ignored, float go, const float (&kd)[NC], float (&o)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; c++) o[c] = ignored ? go * kd[c] : o[c];
}

template <int NC, int VV, bool EXACT, bool TEACH, bool MASK>
__global__ __launch_bounds__(BLK) void seg_loss_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ teacher, int C_, int64_t V,
                                                           float inv_t, const float* __restrict__ coef,
                                                           const float* __restrict__ grad_out, float* __restrict__ dlogits, int ign) {
    const int C = EXACT ? NC : C_;
    int n = blockIdx.y;
    const float* lg = logits + (int64_t)n * C * V;
    const float* tg = TEACH ? teacher + (int64_t)n * C * V : nullptr;
    const int64_t* lb = labels + (int64_t)n * V;
    float* dg = dlogits + (int64_t)n * C * V;
    float go = grad_out ? grad_out[0] : 1.f;
    float A[NC], B[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) { A[c] = coef[c]; B[c] = coef[MAXC + c]; }
    float ce_s = coef[2 * MAXC], kd_s = coef[2 * MAXC + 1];
    int64_t ngrp = V / VV;
    for (int64_t grp = (int64_t)blockIdx.x * BLK + threadIdx.x; grp < ngrp; grp += (int64_t)gridDim.x * BLK) {
        int64_t v0 = grp * VV;
        float z[VV][NC], o[VV][NC];
        int t[VV];
        load_planes<NC, VV>(lg, C, V, v0, z);
        load_labels<VV>(lb + v0, t);
        float zt_[VV][NC];
        if constexpr (TEACH) load_planes<NC, VV>(tg, C, V, v0, zt_);
#pragma unroll
        for (int k = 0; k < VV; k++) {
            float kd[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) kd[c] = 0.f;
            if constexpr (TEACH) {
                float ps[NC], pt[NC], ls, lt;
                softmax_c<NC>(z[k], C, inv_t, ps, ls);
                softmax_c<NC>(zt_[k], C, inv_t, pt, lt);
                kd_voxel<NC>(ps, pt, kd_s, kd);
            }
            dlogits_voxel<NC>(z[k], t[k], C, A, B, ce_s, go, kd, o[k]);
            if constexpr (MASK) dlogits_ignored<NC>(t[k] == ign, go, kd, o[k]);
        }
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (EXACT || c < C) {
                if constexpr (VV == 4) *reinterpret_cast<float4*>(dg + (int64_t)c * V + v0) = float4{o[0][c], o[1][c], o[2][c], o[3][c]};
                else dg[(int64_t)c * V + v0] = o[0][c];
            }
        }
    }
}

// ------------------------------------------------------------------------------- head + loss in one pass (training step)
// The training step needs the logits only inside the loss: logits = head(z) feed seg_loss_fwd (+ metrics) and, recomputed from
// the same z, seg_loss_bwd -> conv1_bwd.  Unfused that is logits written once and read twice and dlogits written and read once
// (5 x 28 MB at 96^3 N=2) and two more launches; fused, neither tensor exists.  The head is evaluated with conv1_fwd_kernel's
// exact expression (bias, then fmaf over ci in order), so every logit has the bits of the unfused path; the forward sums differ
// from seg_loss_fwd_kernel's only in the order the voxels are added (one voxel per thread here: consecutive lanes read
// consecutive 32-byte channel rows), the backward is bit-identical to seg_loss_bwd + conv1_bwd_mfma given the same `coef`.
template <int NC>
__device__ __forceinline__ void head_logits16(const bf16* __restrict__ zrow, int Cin, const float* __restrict__ w,
                                              const float* __restrict__ bias, int C, float (&z)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; c++) z[c] = (bias && c < C) ? bias[c] : 0.f;
    for (int c0 = 0; c0 < Cin; c0 += CINB) {
        float zv[CINB];
        load_cin_block<bf16, true>(zrow + c0, CINB, zv);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c < C) {
#pragma unroll
                for (int i = 0; i < CINB; i++) z[c] = fmaf(zv[i], w[(int64_t)c * Cin + c0 + i], z[c]);
            }
        }
    }
}

// HLW waves per workgroup: the partial rows (one per workgroup) are capped at LOSS_MAXBLK for the single-workgroup finalize, so the
// waves a streaming pass needs to cover the memory latency come from fat workgroups (1024 threads: 32 waves per CU at 2 per CU)
constexpr int HLW = 16;
// MASK: an ignored voxel is a lane past V for the CE term, the I / P sums, `best` and the ballots (scored = false, t = -1), and a
// live one for the distillation term and logits_opt.
template <int NC, bool METRICS, bool EXACT, bool TEACH, bool MASK>
__global__ __launch_bounds__(HLW * 64) void head_loss_fwd_kernel(const bf16* __restrict__ zin, int zcs, int Cin, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const int64_t* __restrict__ labels,
                                                            const float* __restrict__ teacher, float inv_t,
                                                            int C_, int64_t V, double* __restrict__ part,
                                                            unsigned long long* __restrict__ counts, float* __restrict__ logits_opt,
                                                            int ign) {
    const int C = EXACT ? NC : C_;
    constexpr int NQL = 2 + 3 * NC;
    __shared__ float red[HLW][NQL];
    __shared__ unsigned redc[HLW][3 * NC + 1];
    unsigned ni[NC], np[NC], nt[NC];                 // wave-uniform (scalar registers)
#pragma unroll
    for (int c = 0; c < NC; c++) ni[c] = np[c] = nt[c] = 0;
    int n = blockIdx.y;
    const bf16* zn = zin + (int64_t)n * V * zcs;
    const int64_t* lb = labels + (int64_t)n * V;
    const float* tg = TEACH ? teacher + (int64_t)n * C * V : nullptr;
    float q[2 + 2 * NC];                             // ce, kl, I[c], P[c]
#pragma unroll
    for (int i = 0; i < 2 + 2 * NC; i++) q[i] = 0.f;
    // every wave runs the same number of iterations (the ballots below are wave-wide): out-of-range lanes carry t = -1.
    // Two 64-voxel groups per iteration, loads of both issued first (a wave has only ~3 iterations: latency, not issue, bounds it)
    constexpr int U = 2;
    const int64_t gstride = (int64_t)gridDim.x * (HLW * 64);
    int64_t base = (int64_t)blockIdx.x * (HLW * 64) + (threadIdx.x & ~63);
    for (; base < V; base += U * gstride) {
        bf16x8 zr[U][2];
        int tt[U];
        bool lv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            int64_t v = base + u * gstride + (threadIdx.x & 63);
            lv[u] = v < V;
            tt[u] = -1;
            zr[u][0] = zr[u][1] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (lv[u]) {
                static_assert(CINB == 16, "one 32-byte row");
                zr[u][0] = *reinterpret_cast<const bf16x8*>(zn + v * zcs);
                zr[u][1] = *reinterpret_cast<const bf16x8*>(zn + v * zcs + 8);
                tt[u] = (int)lb[v];
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (base + u * gstride >= V) break;                       // wave-uniform
            int64_t v = base + u * gstride + (threadIdx.x & 63);
            bool live = lv[u];
            float z[NC];
            int t = tt[u];
            bool scored = live;                          // the voxel counts in the label-dependent sums
            if constexpr (MASK) {
                scored = live && t != ign;
                t = scored ? t : -1;
            }
            if (Cin == CINB) {
                __attribute__((aligned(16))) bf16 row[16];
                *reinterpret_cast<bf16x8*>(row) = zr[u][0];
                *reinterpret_cast<bf16x8*>(row + 8) = zr[u][1];
                head_logits16<NC>(row, CINB, w, bias, C, z);
            } else if (live) head_logits16<NC>(zn + v * zcs, Cin, w, bias, C, z);
            if (live) {
                if (logits_opt) {
#pragma unroll
                    for (int c = 0; c < NC; c++)
                        if (EXACT || c < C) logits_opt[((int64_t)n * C + c) * V + v] = z[c];
                }
            } else {
#pragma unroll
                for (int c = 0; c < NC; c++) z[c] = 0.f;
            }
            float p[NC], lse;
            softmax_c<NC>(z, C, 1.f, p, lse);
            float zt = 0.f;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (EXACT || c < C) {
                    bool is = (c == t);
                    zt = is ? z[c] : zt;
                    q[2 + c] += is ? p[c] : 0.f;
                    q[2 + NC + c] += scored ? p[c] : 0.f;
                }
            }
            q[0] += scored ? lse - zt : 0.f;
            if constexpr (TEACH) {                       // the distillation term of seg_loss_fwd_kernel, teacher logits from memory
                float ztv[NC];
#pragma unroll
                for (int c = 0; c < NC; c++) ztv[c] = ((EXACT || c < C) && live) ? tg[(int64_t)c * V + v] : 0.f;
                float ps[NC], pt[NC], ls, lt;
                softmax_c<NC>(z, C, inv_t, ps, ls);
                softmax_c<NC>(ztv, C, inv_t, pt, lt);
                float kl = 0.f;
#pragma unroll
                for (int c = 0; c < NC; c++)
                    if ((EXACT || c < C) && pt[c] > 0.f) kl += pt[c] * ((ztv[c] * inv_t - lt) - (z[c] * inv_t - ls));
                q[1] += live ? kl : 0.f;
            }
            float bvv = z[0];
            int best = 0;
#pragma unroll
            for (int c = 1; c < NC; c++)
                if ((EXACT || c < C) && z[c] > bvv) { bvv = z[c]; best = c; }
            if (!scored) best = -1;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                unsigned long long mt = __ballot(t == c);
                nt[c] += (unsigned)__popcll(mt);
                if constexpr (METRICS) {
                    unsigned long long mb = __ballot(best == c);
                    np[c] += (unsigned)__popcll(mb);
                    ni[c] += (unsigned)__popcll(mb & mt);
                }
            }
        }
    }
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < 2 + 2 * NC; i++) {
        float sv = wave_sum(q[i]);
        if (lane == 0) red[wave][i] = sv;
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            red[wave][2 + 2 * NC + c] = (float)nt[c];
            redc[wave][c] = ni[c]; redc[wave][NC + c] = np[c]; redc[wave][2 * NC + c] = nt[c];
        }
    }
    __syncthreads();
    const int nqc = 2 + 3 * C;                        // the compact rows of seg_loss_fwd_kernel: same finalize kernels
    if ((int)threadIdx.x < nqc) {
        int i = threadIdx.x, src = i;
        if (i >= 2) { int k = (i - 2) / C, c = (i - 2) % C; src = 2 + k * NC + c; }
        double v = 0.0;
#pragma unroll
        for (int wv = 0; wv < HLW; wv++) v += (double)red[wv][src];
        part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nqc + i] = v;
    }
    if constexpr (METRICS) {
        if ((int)threadIdx.x < 3 * C + 1) {
            int i = threadIdx.x;
            unsigned long long v = 0;
            if (i < 3 * C) {
                int src = (i / C) * NC + (i % C);
                for (int wv = 0; wv < HLW; wv++) v += redc[wv][src];
            } else {
                for (int wv = 0; wv < HLW; wv++)
#pragma unroll
                    for (int c = 0; c < NC; c++) v += redc[wv][c];
            }
            counts[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (3 * C + 1) + i] = v;
        }
    }
}

// conv1_bwd_mfma_kernel with dlogits made on the spot: the wave stages its 32 x 16 z tile as before, lanes l and l + 32
// re-derive voxel l's logits from that tile (head_logits16: the forward's bits), turn them into dL/dz with dlogits_voxel and
// leave them in a wave-private [class][32 voxels] LDS tile, from which both MFMA operands are read where the plain kernel
// reads the dlogits planes.  Cin = 16 (one input block), Cout <= 4.
// MASK: the ignored voxel's dlogits are selected in registers (dlogits_ignored) before they go into the tile: no LDS access more,
// the wave-private tile protocol as it is.
template <bool TEACH, bool MASK>
__global__ __launch_bounds__(C1W * 64) void head_loss_bwd_mfma_kernel(const bf16* __restrict__ z, int zcs, const float* __restrict__ w,
                                                                      const float* __restrict__ bias, const int64_t* __restrict__ labels,
                                                                      const float* __restrict__ teacher, float inv_t,
                                                                      int Cout, const float* __restrict__ coef,
                                                                      const float* __restrict__ grad_out, bf16* __restrict__ dz, int dzcs,
                                                                      int64_t V, float* __restrict__ slabs, int ign) {
    constexpr int NC = 4, Cin = 16;
    __shared__ __attribute__((aligned(16))) bf16 zt[C1W][2][32 * 16];
    __shared__ __attribute__((aligned(16))) float dlt[C1W][2][NC * 32];
    __shared__ float red[C1W][64][4];
    __shared__ float redb[C1W][16];
    int n = blockIdx.y;
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int vn = lane & 15, kg = lane >> 4;
    const bf16* zn = z + (int64_t)n * V * zcs;
    bf16* dzn = dz ? dz + (int64_t)n * V * dzcs : nullptr;
    const bool wide_dz = dzn && (dzcs & 7) == 0 && (reinterpret_cast<uintptr_t>(dzn) & 15) == 0;       // uniform: 16-byte dz stores
    const int64_t* lb = labels + (int64_t)n * V;
    const float* tg = TEACH ? teacher + (int64_t)n * Cout * V : nullptr;
    float go = grad_out ? grad_out[0] : 1.f;
    float A[NC], B[NC], kd0[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) { A[c] = coef[c]; B[c] = coef[MAXC + c]; kd0[c] = 0.f; }
    float ce_s = coef[2 * MAXC], kd_s = coef[2 * MAXC + 1];
    bf16x8 aw;
#pragma unroll
    for (int j = 0; j < 8; j++) aw[j] = (bf16)0.f;
    aw[0] = (bf16)(kg < Cout ? w[(int64_t)kg * Cin + vn] : 0.f);
    f32x4 accW = {0.f, 0.f, 0.f, 0.f};
    float dbs = 0.f;
    int laneK = ((8 * kg + ((lane & 15) >> 2)) * 16 + 4 * (lane & 3)) * 2;
    // the wave's 32-voxel chunks are those of conv1_bwd_mfma_kernel, in its order, but taken two at a time: lanes 0-31 make the
    // dlogits of chunk k, lanes 32-63 those of chunk k + 1 (64 distinct voxels per pass of the per-voxel arithmetic); a chunk
    // beyond V is all zeros and adds nothing
    const int64_t stride = (int64_t)gridDim.x * (C1W * 32);
    for (int64_t v0 = ((int64_t)blockIdx.x * C1W + wave) * 32; v0 < V; v0 += 2 * stride) {
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            int64_t v = v0 + hh * stride + (lane >> 1);
            bf16x8 t = {0, 0, 0, 0, 0, 0, 0, 0};
            if (v < V) t = *reinterpret_cast<const bf16x8*>(zn + v * zcs + (lane & 1) * 8);
            *reinterpret_cast<bf16x8*>(zt[wave][hh] + (lane >> 1) * 16 + (lane & 1) * 8) = t;
        }
        const int hl = lane >> 5;
        int64_t vl = v0 + hl * stride + (lane & 31);
        int tl = vl < V ? (int)lb[vl] : 0;
        __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): the tiles are private to this wave
        __builtin_amdgcn_wave_barrier();
        {
            float zl[NC], o[NC];
            head_logits16<NC>(zt[wave][hl] + (lane & 31) * 16, Cin, w, bias, Cout, zl);
            if constexpr (TEACH) {                       // the distillation term of seg_loss_bwd_kernel
                float ztv[NC], ps[NC], pt[NC], ls, lt;
#pragma unroll
                for (int c = 0; c < NC; c++) ztv[c] = (c < Cout && vl < V) ? tg[(int64_t)c * V + vl] : 0.f;
                softmax_c<NC>(zl, Cout, inv_t, ps, ls);
                softmax_c<NC>(ztv, Cout, inv_t, pt, lt);
                kd_voxel<NC>(ps, pt, kd_s, kd0);
            }
            dlogits_voxel<NC>(zl, tl, Cout, A, B, ce_s, go, kd0, o);
            if constexpr (MASK) dlogits_ignored<NC>(tl == ign, go, kd0, o);
#pragma unroll
            for (int c = 0; c < NC; c++) dlt[wave][hl][c * 32 + (lane & 31)] = (c < Cout && vl < V) ? o[c] : 0.f;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            const int64_t vc = v0 + hh * stride;
            // dW: B = dl, 8 consecutive voxels of class vn
            bf16x8 bd = {0, 0, 0, 0, 0, 0, 0, 0};
            if (vn < Cout) {
                float4 p4 = *reinterpret_cast<const float4*>(&dlt[wave][hh][vn * 32 + 8 * kg]), q4 = *reinterpret_cast<const float4*>(&dlt[wave][hh][vn * 32 + 8 * kg + 4]);
                float t8[8] = {p4.x, p4.y, p4.z, p4.w, q4.x, q4.y, q4.z, q4.w};
#pragma unroll
                for (int j = 0; j < 8; j++) { bd[j] = (bf16)t8[j]; dbs += t8[j]; }
            }
            bf16x4 obn[2];
#pragma unroll
            for (int nb = 0; nb < 2; nb++) {
                int64_t v = vc + nb * 16 + vn;
                bf16x8 bl = {0, 0, 0, 0, 0, 0, 0, 0};
                if (v < V && kg < Cout) bl[0] = (bf16)dlt[wave][hh][kg * 32 + nb * 16 + vn];
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw, bl, o, 0, 0, 0);
                obn[nb] = bf16x4{(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
                if (!wide_dz && dzn && v < V) *reinterpret_cast<bf16x4*>(dzn + v * dzcs + 4 * kg) = obn[nb];
            }
            if (wide_dz) {
                // 16-byte stores (round 4): the two 16-voxel groups trade halves (v_permlane16_swap); lane (vn, kg) then holds channels
                // (kg >> 1) * 8 .. + 7 of voxel vc + (kg & 1) * 16 + vn
                u32x4 wv = swap_halves16(obn[0], obn[1]);
                const int64_t vw = vc + (kg & 1) * 16 + vn;
                if (vw < V) *reinterpret_cast<u32x4*>(dzn + vw * dzcs + (kg >> 1) * 8) = wv;
            }
            bf16x8 az = tr_frag(reinterpret_cast<const char*>(zt[wave][hh]), laneK);
            accW = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az, bd, accW, 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
    *reinterpret_cast<f32x4*>(&red[wave][lane][0]) = accW;
    float sb = dbs;
    sb += __shfl_xor(sb, 16, 64);
    sb += __shfl_xor(sb, 32, 64);
    if (lane < 16) redb[wave][lane] = sb;
    __syncthreads();
    int64_t nW = (int64_t)Cout * Cin;
    float* slab = slabs + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (nW + Cout);
    if (threadIdx.x < 64) {
        int l = threadIdx.x, co = l & 15, g4 = l >> 4;
        if (co < Cout) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float sv = 0.f;
#pragma unroll
                for (int wv = 0; wv < C1W; wv++) sv += red[wv][l][r];
                slab[(int64_t)co * Cin + 4 * g4 + r] = sv;
            }
        }
    } else if (threadIdx.x < 64 + 16) {
        int co = threadIdx.x - 64;
        if (co < Cout) {
            float sv = 0.f;
#pragma unroll
            for (int wv = 0; wv < C1W; wv++) sv += redb[wv][co];
            slab[nW + co] = sv;
        }
    }
}

// ------------------------------------------------------------------------------------------ metrics
// The predicted class of one voxel: the first maximum under a strict `>` scan from class 0, which is torch.argmax for finite
// logits.  A NaN never wins a comparison and, once it is the running maximum, never loses one: a NaN logit 0 gives class 0, a
// NaN elsewhere is never chosen.
template <int NC>
__device__ __forceinline__ int first_argmax(const float (&z)[NC], int C) {
    float bv = z[0];
    int best = 0;
#pragma unroll
    for (int c = 1; c < NC; c++)
        if (c < C && z[c] > bv) { bv = z[c]; best = c; }
    return best;
}

// Exact argmax / label counts of the voxels one thread has seen, and their way into one partial row per block:
// per-thread counts -> wave sums -> LDS -> 3C + 1 integers {n_inter[C], n_pred[C], n_label[C], n_correct} (no floating point,
// no atomics).  A label outside [0, C) counts nowhere.  A thread sees < 2^32 voxels.
template <int NC>
struct VoxelCounts {
    unsigned ni[NC], np[NC], nt[NC], nc;
    __device__ __forceinline__ VoxelCounts() : nc(0) {
#pragma unroll
        for (int c = 0; c < NC; c++) ni[c] = np[c] = nt[c] = 0;
    }
    __device__ __forceinline__ void add(int best, int t) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            ni[c] += (best == c && t == c) ? 1u : 0u;
            np[c] += (best == c) ? 1u : 0u;
            nt[c] += (t == c) ? 1u : 0u;
        }
        nc += (best == t) ? 1u : 0u;
    }
    // every thread of the BLK-thread block calls this once; row: the block's 3C + 1 entries
    __device__ __forceinline__ void store_block_row(int C, unsigned long long* __restrict__ row) const {
        __shared__ unsigned red[BLK / 64][3 * NC + 1];
        int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        auto wsum = [&](unsigned v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; };
#pragma unroll
        for (int c = 0; c < NC; c++) {
            unsigned a = wsum(ni[c]), b = wsum(np[c]), d = wsum(nt[c]);
            if (lane == 0) { red[wave][c] = a; red[wave][NC + c] = b; red[wave][2 * NC + c] = d; }
        }
        unsigned e = wsum(nc);
        if (lane == 0) red[wave][3 * NC] = e;
        __syncthreads();
        if ((int)threadIdx.x < 3 * C + 1) {                       // compact row: 3C + 1 counts
            int i = threadIdx.x;
            int src = i == 3 * C ? 3 * NC : (i / C) * NC + (i % C);
            unsigned long long v = 0;
#pragma unroll
            for (int wv = 0; wv < BLK / 64; wv++) v += red[wv][src];
            row[i] = v;
        }
    }
};

template <int NC, int VV>
__global__ __launch_bounds__(BLK) void seg_metrics_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                          int C, int64_t V, unsigned long long* __restrict__ counts) {
    int n = blockIdx.y;
    const float* lg = logits + (int64_t)n * C * V;
    const int64_t* lb = labels + (int64_t)n * V;
    VoxelCounts<NC> cnt;
    int64_t ngrp = V / VV;
    for (int64_t grp = (int64_t)blockIdx.x * BLK + threadIdx.x; grp < ngrp; grp += (int64_t)gridDim.x * BLK) {
        int64_t v0 = grp * VV;
        float z[VV][NC];
        int t[VV];
        load_planes<NC, VV>(lg, C, V, v0, z);
        load_labels<VV>(lb + v0, t);
#pragma unroll
        for (int k = 0; k < VV; k++) cnt.add(first_argmax<NC>(z[k], C), t[k]);
    }
    cnt.store_block_row(C, counts + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (3 * C + 1));
}

// ---------------------------------------------------------------------------- head + argmax + per-sample counts in one pass
// labels[n][v] = first_argmax(conv1_voxel(z[n][v])) as uint8, and with TARGET the exact counts of seg_metrics_kernel per
// (sample, block).  HBM-bound: Cin * sizeof(T) bytes read and 1 byte written per voxel (+ 8 with a target).
// A wave owns 64 * HLV consecutive voxels per iteration and takes them in HLV rounds of 64, lane l the voxel 64 k + l of round k:
// consecutive lanes read consecutive channel rows, as conv1_fwd_kernel does (a thread that owns consecutive voxels
// spreads every load instruction of the wave over 64 cache lines: the note at conv1_fwd's launch).  The 64 * HLV label bytes of the
// wave go through its own LDS tile, written a byte per lane and round in voxel order and read back 16 bytes per lane, so a
// thread still ends with its HLV = 16 labels in ONE 16-byte store and the wave writes 1 KiB contiguously.  A chunk that is
// not whole (the tail of V) or whose first byte is not 16-byte aligned (n * V odd) stores its live bytes directly instead.
// Out-of-range lanes of a tail chunk recompute the sample's last voxel and neither store nor count it.
constexpr int HLV = 16;
template <typename T, bool VEC, int NC, bool TARGET>
__global__ __launch_bounds__(BLK) void head_labels_kernel(const T* __restrict__ z, int zcs, int Cin, const float* __restrict__ w,
                                                          const float* __restrict__ bias, int C, int64_t V,
                                                          uint8_t* __restrict__ labels, const int64_t* __restrict__ target,
                                                          unsigned long long* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[BLK / 64][64 * HLV];
    const int n = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const T* zn = z + (int64_t)n * V * zcs;
    uint8_t* ln = labels + (int64_t)n * V;
    const int64_t* tn = TARGET ? target + (int64_t)n * V : nullptr;
    VoxelCounts<NC> cnt;
    // ONE: the whole channel row is one block (the network's head: Cin = 16).  The channel loop of conv1_voxel then has a
    // constant single trip and the loads of all rounds can be issued ahead of the arithmetic; same fmaf chain either way.
    auto chunks = [&](auto ONE) {
        const int cin = decltype(ONE)::value ? CINB : Cin;
        for (int64_t base = ((int64_t)blockIdx.x * (BLK / 64) + wave) * (64 * HLV); base < V; base += (int64_t)gridDim.x * (BLK * HLV)) {
            const bool wide = base + 64 * HLV <= V && (reinterpret_cast<uintptr_t>(ln + base) & 15) == 0;      // wave-uniform
#pragma unroll
            for (int k = 0; k < HLV; k++) {
                const int64_t v = base + k * 64 + lane;
                const bool live = v < V;
                const int64_t vc = live ? v : V - 1;
                float acc[NC];
                conv1_voxel<T, VEC, NC>(zn + vc * zcs, cin, w, bias, 0, C, acc);
                const int best = first_argmax<NC>(acc, C);
                if constexpr (TARGET) {
                    const int64_t tv = tn[vc];
                    if (live) cnt.add(best, (tv >= 0 && tv < C) ? (int)tv : -1);
                }
                if (wide) tile[wave][k * 64 + lane] = (uint8_t)best;
                else if (live) ln[v] = (uint8_t)best;
            }
            if (wide) {
                // the tile is private to this wave: its LDS writes are complete for the wave before the wide read
                __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0)
                __builtin_amdgcn_wave_barrier();
                *reinterpret_cast<uint4*>(ln + base + lane * HLV) = *reinterpret_cast<const uint4*>(&tile[wave][lane * HLV]);
                __builtin_amdgcn_wave_barrier();
            }
        }
    };
    if (VEC && Cin == CINB) chunks(std::integral_constant<bool, VEC>{});
    else chunks(std::false_type{});
    if constexpr (TARGET) cnt.store_block_row(C, counts + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (3 * C + 1));
}

// ------------------------------------------------------------------ head + softmax + vote of one view (flip / model ensembles)
// One view of an ensemble: z is the decoder output of model(flip(x)), and the view's probabilities are added into the planar
// float32 vote volume (N, C, D, H, W) AT THE UN-FLIPPED VOXEL.  The kernel walks the OUTPUT voxels linearly and gathers the
// channel row of z at the mirrored index (flip bit 0: W, 1: H, 2: D): the gather sits on the side with the widest unit (a whole
// 2 Cin-byte channel row per voxel stays contiguous, and a W flip only reverses the order in which a wave touches the same rows),
// and the C vote planes and the label bytes, which are 4- and 1-byte units, stay linear.
//   MODE & VOTE_FIRST   the votes are not read: votes = p (no memset)
//   neither             votes = votes + p
//   MODE & VOTE_LAST    total = votes + p stays in registers: first_argmax -> uint8 label (+ counts with TARGET); confidence, if
//                       asked for, total[label] / views (IEEE division); the total is written back only with `keep`
// p = softmax_c of conv1_voxel's logits; the adds are float32 adds in view order (__fadd_rn: never contracted with the
// product inside softmax_c), one thread owns a voxel, no atomics: the same bits on every run.
// HBM-bound: per voxel Cin * sizeof(T) bytes of z, and of votes 4 C written (FIRST), 8 C (neither), 4 C read + 1 label byte (LAST).
// A thread owns VV consecutive output voxels, as in conv1_fwd_kernel and seg_metrics_kernel: with VV = 4 (V % 4 == 0, aligned
// planes) every plane access is 16 bytes and the labels are one 4-byte store.  The other candidate, head_labels_kernel's
// lane-per-voxel rounds with an LDS label tile, was built and timed against a 4-voxel kernel in one process at 192^3, bf16,
// 4 classes, all three axes mirrored (same bits): FIRST 75 us against 96, MIDDLE 136 against 112, LAST 110 against 97 -- 1.00 ms
// against 0.86 ms for the eight passes of a flip ensemble (profiles/votes_timing.txt): the vote planes are most of the traffic
// and decide, not the z rows, so the 4-voxel walk is the one kept.
// (d, h, w): the group's first voxel is decoded with two 32-bit divisions, the others step from it with a carry; V < 2^31 is
// the launcher's check.
constexpr int VOTE_FIRST = 1, VOTE_LAST = 2;
template <typename T, bool VEC, int NC, int VV, int MODE, bool TARGET>
__global__ __launch_bounds__(BLK) void head_votes_kernel(const T* __restrict__ z, int zcs, int Cin, const float* __restrict__ w,
                                                         const float* __restrict__ bias, int C, int D, int H, int W, int flip,
                                                         float views, int keep, float* __restrict__ votes,
                                                         uint8_t* __restrict__ labels, float* __restrict__ confidence,
                                                         const int64_t* __restrict__ target, unsigned long long* __restrict__ counts) {
    constexpr bool FIRST = (MODE & VOTE_FIRST) != 0, LAST = (MODE & VOTE_LAST) != 0;
    const int n = blockIdx.y;
    const unsigned V = (unsigned)D * (unsigned)H * (unsigned)W;
    const T* zn = z + (int64_t)n * V * zcs;
    float* vn = votes ? votes + (int64_t)n * C * V : nullptr;
    uint8_t* ln = LAST ? labels + (int64_t)n * V : nullptr;
    float* cn = (LAST && confidence) ? confidence + (int64_t)n * V : nullptr;
    const int64_t* tn = TARGET ? target + (int64_t)n * V : nullptr;
    const bool fw = flip & 1, fh = flip & 2, fd = flip & 4;
    VoxelCounts<NC> cnt;
    // ONE: the whole channel row is one block (the network's head: Cin = 16), as in head_labels_kernel: a constant single trip
    auto groups = [&](auto ONE) {
        const int cin = decltype(ONE)::value ? CINB : Cin;
        for (unsigned grp = blockIdx.x * BLK + threadIdx.x; grp < V / VV; grp += gridDim.x * BLK) {
            const unsigned v0 = grp * VV, row = v0 / (unsigned)W;
            unsigned xw = v0 - row * (unsigned)W, xd = row / (unsigned)H, xh = row - xd * (unsigned)H;
            float p[VV][NC];
#pragma unroll
            for (int k = 0; k < VV; k++) {
                const unsigned sw = fw ? W - 1 - xw : xw, sh = fh ? H - 1 - xh : xh, sd = fd ? D - 1 - xd : xd;
                float acc[NC], lse;
                conv1_voxel<T, VEC, NC>(zn + (((int64_t)sd * H + sh) * W + sw) * zcs, cin, w, bias, 0, C, acc);
                softmax_c<NC>(acc, C, 1.f, p[k], lse);
                if (++xw == (unsigned)W) {                   // the next voxel of the group
                    xw = 0;
                    if (++xh == (unsigned)H) { xh = 0; xd++; }
                }
            }
            if constexpr (!FIRST) {
                float t[VV][NC];
                load_planes<NC, VV>(vn, C, V, v0, t);
#pragma unroll
                for (int k = 0; k < VV; k++) {
#pragma unroll
                    for (int c = 0; c < NC; c++) p[k][c] = __fadd_rn(t[k][c], p[k][c]);
                }
            }
            if (!LAST || keep) {
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    if (c < C) {
                        if constexpr (VV == 4) *reinterpret_cast<float4*>(vn + (int64_t)c * V + v0) = float4{p[0][c], p[1][c], p[2][c], p[3][c]};
                        else vn[(int64_t)c * V + v0] = p[0][c];
                    }
                }
            }
            if constexpr (LAST) {
                int best[VV];
                float cf[VV];
#pragma unroll
                for (int k = 0; k < VV; k++) {
                    best[k] = first_argmax<NC>(p[k], C);
                    float top = p[k][0];
#pragma unroll
                    for (int c = 1; c < NC; c++) top = best[k] == c ? p[k][c] : top;
                    cf[k] = __fdiv_rn(top, views);
                }
                if constexpr (TARGET) {
#pragma unroll
                    for (int k = 0; k < VV; k++) {
                        const int64_t tv = tn[v0 + k];
                        cnt.add(best[k], (tv >= 0 && tv < C) ? (int)tv : -1);
                    }
                }
                if constexpr (VV == 4) {
                    *reinterpret_cast<unsigned*>(ln + v0) = (unsigned)best[0] | (unsigned)best[1] << 8 | (unsigned)best[2] << 16 | (unsigned)best[3] << 24;
                    if (cn) *reinterpret_cast<float4*>(cn + v0) = float4{cf[0], cf[1], cf[2], cf[3]};
                } else {
                    ln[v0] = (uint8_t)best[0];
                    if (cn) cn[v0] = cf[0];
                }
            }
        }
    };
    if (VEC && Cin == CINB) groups(std::integral_constant<bool, VEC>{});
    else groups(std::false_type{});
    if constexpr (TARGET) cnt.store_block_row(C, counts + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (3 * C + 1));
}

// ------------------------------------------------------ head + softmax + WEIGHTED vote of one window (sliding-window inference)
// One window sample of sides d x h x w at origin (od, oh, ow) of the accumulator acc (C, D, H, W): head_votes_kernel's walk and
// mirror map, within the window, and
//     acc[c][o + x] = acc[c][o + x] + ((g_d[xd] * g_h[xh]) * g_w[xw]) * p[c]       __fmul_rn, then __fadd_rn: never contracted
// Windows overlap in acc, so a launch handles ONE sample and the stream orders the samples: one thread owns a voxel, nothing is
// atomic, the same bits on every run.  VV = 4 where W, w and ow are multiples of 4 (the launcher's check): a group then stays
// inside one window row and is 16-byte aligned in every plane; VV = 1 is the same arithmetic per voxel, so both give the same bits.
// HBM-bound: per window voxel Cin * sizeof(T) bytes of z and 8 C of acc (the three tables stay in cache); v < 2^31 because the
// window lies inside a volume the launcher holds to that.
template <typename T, bool VEC, int NC, int VV>
__global__ __launch_bounds__(BLK) void head_votes_window_kernel(const T* __restrict__ zn, int zcs, int Cin, const float* __restrict__ w,
                                                                const float* __restrict__ bias, int C, int d, int h, int wd, int flip,
                                                                const float* __restrict__ gd, const float* __restrict__ gh,
                                                                const float* __restrict__ gw, int od, int oh, int ow,
                                                                float* __restrict__ acc, int H, int W, int64_t V) {
    const unsigned v = (unsigned)d * (unsigned)h * (unsigned)wd;
    const bool fw = flip & 1, fh = flip & 2, fd = flip & 4;
    auto groups = [&](auto ONE) {
        const int cin = decltype(ONE)::value ? CINB : Cin;
        for (unsigned grp = blockIdx.x * BLK + threadIdx.x; grp < v / VV; grp += gridDim.x * BLK) {
            const unsigned v0 = grp * VV, row = v0 / (unsigned)wd;
            const unsigned xw = v0 - row * (unsigned)wd, xd = row / (unsigned)h, xh = row - xd * (unsigned)h;
            const unsigned sh = fh ? h - 1 - xh : xh, sd = fd ? d - 1 - xd : xd;
            const float gdh = __fmul_rn(gd[xd], gh[xh]);
            const int64_t a0 = ((int64_t)(od + (int)xd) * H + (oh + (int)xh)) * W + (ow + (int)xw);
            float p[VV][NC];
#pragma unroll
            for (int k = 0; k < VV; k++) {
                const unsigned sw = fw ? wd - 1 - (xw + k) : xw + k;
                float lg[NC], lse;
                conv1_voxel<T, VEC, NC>(zn + (((int64_t)sd * h + sh) * wd + sw) * zcs, cin, w, bias, 0, C, lg);
                softmax_c<NC>(lg, C, 1.f, p[k], lse);
                const float wt = __fmul_rn(gdh, gw[xw + k]);
#pragma unroll
                for (int c = 0; c < NC; c++) p[k][c] = __fmul_rn(wt, p[k][c]);
            }
            float t[VV][NC];
            load_planes<NC, VV>(acc, C, V, a0, t);
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (c < C) {
                    if constexpr (VV == 4)
                        *reinterpret_cast<float4*>(acc + (int64_t)c * V + a0) = float4{__fadd_rn(t[0][c], p[0][c]), __fadd_rn(t[1][c], p[1][c]),
                                                                                       __fadd_rn(t[2][c], p[2][c]), __fadd_rn(t[3][c], p[3][c])};
                    else acc[(int64_t)c * V + a0] = __fadd_rn(t[0][c], p[0][c]);
                }
            }
        }
    };
    if (VEC && Cin == CINB) groups(std::integral_constant<bool, VEC>{});
    else groups(std::false_type{});
}

// The finishing pass of the window votes: per voxel of acc (C, D, H, W)
//     norm = ((n_d[xd] * n_h[xh]) * n_w[xw]) * views         __fmul_rn each
//     label = first_argmax(acc);  confidence = acc[label] / norm;  with `normalize` acc[c] = acc[c] / norm     (IEEE divisions)
// and with TARGET the counts of head_votes_kernel's last view.  VV = 4 where W % 4 == 0 and every pointer is aligned.
// HBM-bound: 4 C bytes read (+ 4 C written with normalize), 1 label byte (+ 4 confidence, + 8 target) per voxel.
template <int NC, int VV, bool TARGET>
__global__ __launch_bounds__(BLK) void votes_finish_kernel(float* __restrict__ acc, int C, int D, int H, int W, const float* __restrict__ nd,
                                                           const float* __restrict__ nh, const float* __restrict__ nw, float views,
                                                           int normalize, uint8_t* __restrict__ labels, float* __restrict__ confidence,
                                                           const int64_t* __restrict__ target, unsigned long long* __restrict__ counts) {
    const unsigned V = (unsigned)D * (unsigned)H * (unsigned)W;
    VoxelCounts<NC> cnt;
    for (unsigned grp = blockIdx.x * BLK + threadIdx.x; grp < V / VV; grp += gridDim.x * BLK) {
        const unsigned v0 = grp * VV, row = v0 / (unsigned)W;
        const unsigned xw = v0 - row * (unsigned)W, xd = row / (unsigned)H, xh = row - xd * (unsigned)H;
        const float ndh = __fmul_rn(nd[xd], nh[xh]);
        float t[VV][NC], norm[VV], cf[VV];
        int best[VV];
        load_planes<NC, VV>(acc, C, V, v0, t);
#pragma unroll
        for (int k = 0; k < VV; k++) {
            norm[k] = __fmul_rn(__fmul_rn(ndh, nw[xw + k]), views);
            best[k] = first_argmax<NC>(t[k], C);
            float top = t[k][0];
#pragma unroll
            for (int c = 1; c < NC; c++) top = best[k] == c ? t[k][c] : top;
            cf[k] = __fdiv_rn(top, norm[k]);
            if constexpr (TARGET) {
                const int64_t tv = target[v0 + k];
                cnt.add(best[k], (tv >= 0 && tv < C) ? (int)tv : -1);
            }
        }
        if (normalize) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (c < C) {
                    if constexpr (VV == 4)
                        *reinterpret_cast<float4*>(acc + (int64_t)c * V + v0) = float4{__fdiv_rn(t[0][c], norm[0]), __fdiv_rn(t[1][c], norm[1]),
                                                                                       __fdiv_rn(t[2][c], norm[2]), __fdiv_rn(t[3][c], norm[3])};
                    else acc[(int64_t)c * V + v0] = __fdiv_rn(t[0][c], norm[0]);
                }
            }
        }
        if constexpr (VV == 4) {
            *reinterpret_cast<unsigned*>(labels + v0) = (unsigned)best[0] | (unsigned)best[1] << 8 | (unsigned)best[2] << 16 | (unsigned)best[3] << 24;
            if (confidence) *reinterpret_cast<float4*>(confidence + v0) = float4{cf[0], cf[1], cf[2], cf[3]};
        } else {
            labels[v0] = (uint8_t)best[0];
            if (confidence) confidence[v0] = cf[0];
        }
    }
    if constexpr (TARGET) cnt.store_block_row(C, counts + (int64_t)blockIdx.x * (3 * C + 1));
}

__device__ __forceinline__ void count_row_sum(const unsigned long long* part, int nblk, int C, int q, int lane, unsigned long long* counts);
__device__ __forceinline__ void metric_scalars(const unsigned long long* counts, int N, int C, int D, int64_t V, float* out, int mask = 0);
// Q1: the reference's class loop is range(1, pred.size(1)) AFTER argmax -> bound = first spatial dim D
__device__ __forceinline__ void seg_metrics_finalize_body(const unsigned long long* part, int nblk, int N, int C,
                                                          int D, int64_t V, float* out) {
    __shared__ unsigned long long counts[3 * MAXC + 1];
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ncc = 3 * C + 1;
    if (threadIdx.x < 3 * MAXC + 1) counts[threadIdx.x] = 0;
    __syncthreads();
    for (int q = wave; q < ncc; q += 16) count_row_sum(part, nblk, C, q, lane, counts);     // exact integer sums, wave-parallel
    __syncthreads();
    if (threadIdx.x != 0) return;
    metric_scalars(counts, N, C, D, V, out);
}

__device__ __forceinline__ void count_row_sum(const unsigned long long* part, int nblk, int C, int q, int lane, unsigned long long* counts) {
    const int ncc = 3 * C + 1;
    unsigned long long s = 0;
    for (int b = lane; b < nblk; b += 64) s += part[(int64_t)b * ncc + q];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) counts[q == 3 * C ? 3 * MAXC : (q / C) * MAXC + q % C] = s;
}

// mask (the masked loss + metrics pass): the counts leave the ignored voxels out, and accuracy divides by M_valid = sum_c n_label[c]
// (0 when that is 0)
__device__ __forceinline__ void metric_scalars(const unsigned long long* counts, int N, int C, int D, int64_t V, float* out, int mask) {
    float iou = 0.f, dice = 0.f;
    int valid = 0;
    for (int c = 1; c < D && c < C; c++) {
        unsigned long long nt = counts[2 * MAXC + c];
        if (nt > 0) {
            float inter = (float)counts[c];
            float sum = (float)(long long)(counts[MAXC + c] + nt);
            iou += (inter + 1e-5f) / ((sum - inter) + 1e-5f);
            dice += (2.f * inter + 1e-5f) / (sum + 1e-5f);
            valid++;
        }
    }
    float dv = (float)(valid > 1 ? valid : 1);
    out[0] = iou / dv;
    out[1] = dice / dv;
    if (mask) {
        unsigned long long mv = 0;
        for (int c = 0; c < C; c++) mv += counts[2 * MAXC + c];
        out[2] = mv ? (float)((double)counts[3 * MAXC] / (double)mv) : 0.f;
        return;
    }
    out[2] = (float)((double)counts[3 * MAXC] / ((double)N * (double)V));
}

__global__ __launch_bounds__(1024) void seg_metrics_finalize_kernel(const unsigned long long* part, int nblk, int N, int C,
                                                                    int D, int64_t V, float* out) {
    seg_metrics_finalize_body(part, nblk, N, C, D, V, out);
}
// both finalizes of the fused loss + metrics pass in one launch (one chain link less)
__global__ __launch_bounds__(1024) void seg_loss_metrics_finalize_kernel(const double* __restrict__ part, const unsigned long long* cnt,
                                                                         int nblk, int N, int C, int D, int64_t V, LossCfg cfg,
                                                                         float* loss_out, float* coef, float* met_out) {
    // all 2 + 3C + 3C + 1 row sums in ONE phase (two rounds of the 16 waves, every load issued before the first wait), then the
    // two scalar tails on two waves at once: same sums in the same order as the two bodies one after the other, one
    // memory round trip and one serial tail less on the step's dependent chain
    __shared__ double sums[NQ];
    __shared__ unsigned long long counts[3 * MAXC + 1];
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nqc = 2 + 3 * C, ncc = 3 * C + 1;
    if (threadIdx.x < NQ) sums[threadIdx.x] = 0.0;
    if (threadIdx.x < 3 * MAXC + 1) counts[threadIdx.x] = 0;
    __syncthreads();
    for (int q = wave; q < nqc + ncc; q += 16) {
        if (q < nqc) loss_row_sum(part, nblk, C, q, lane, sums);
        else count_row_sum(cnt, nblk, C, q - nqc, lane, counts);
    }
    __syncthreads();
    if (threadIdx.x == 0) loss_scalars(sums, N, C, V, cfg, loss_out, coef);
    if (threadIdx.x == 64) metric_scalars(counts, N, C, D, V, met_out, cfg.mask);
}

// raw exact counts for the per-class evaluation metrics (test_model.py:242-285): out[0..C) n_inter, [C..2C) n_pred,
// [2C..3C) n_tgt, [3C] n_correct  (int64).  Block b sums rows [b * nblk, (b + 1) * nblk) into out[b]: one block for the sum over
// the batch (seg_metrics), one block per sample for per-sample counts (head_labels)
__global__ __launch_bounds__(1024) void seg_counts_finalize_kernel(const unsigned long long* part, int nblk, int C, long long* out) {
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    part += (int64_t)blockIdx.x * nblk * (3 * C + 1);
    out += (int64_t)blockIdx.x * (3 * C + 1);
    for (int q = wave; q < 3 * C + 1; q += 16) {            // rows and output share the compact layout
        unsigned long long s = 0;
        for (int b = lane; b < nblk; b += 64) s += part[(int64_t)b * (3 * C + 1) + q];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) out[q] = (long long)s;
    }
}

constexpr int METRIC_BLOCKS = 512;
inline int sgrid(int64_t total, int cap) {
    int64_t w = (total + BLK - 1) / BLK;
    return (int)(w < 1 ? 1 : (w > cap ? cap : w));
}
inline bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }
constexpr int CONV1_NBLK = 512;
}  // namespace

// blocks per sample for the (blocks, N) grids: `cap` blocks in total, at least one per sample
inline int per_sample_blocks(int64_t V, int vv, int N, int cap) {
    int64_t w = (V / vv + BLK - 1) / BLK, c = cap / N;
    if (c < 1) c = 1;
    return (int)(w < 1 ? 1 : (w > c ? c : w));
}
inline bool vv4(int64_t V, const void* a, const void* b = nullptr, const void* c = nullptr) {
    return V % 4 == 0 && al16(a) && al16(b) && al16(c);
}

int conv1_fwd(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, float* logits, int Cout,
              int N, int64_t V, hipStream_t s) {
    MI3D_CHECK_ARG(Cin >= 1 && Cout >= 1, "conv1_fwd: bad channels");
    DISPATCH_T(dtype, T, {
        bool vec = Cin % CINB == 0 && zcs % 8 == 0 && al16(z);
        // one voxel per thread: consecutive lanes read consecutive 32-byte channel rows (a thread owning 4 voxels would
        // spread every 16-byte load instruction of a wave over 64 cache lines -- measured 1.7x slower)
        if (vec && Cout <= 4) {
            dim3 grid((unsigned)per_sample_blocks(V, 1, N, 4096), (unsigned)N, 1);
            conv1_fwd_kernel<T, true, 4, 1><<<grid, BLK, 0, s>>>((const T*)z, zcs, Cin, w, bias, logits, Cout, V);
        } else {
            dim3 grid((unsigned)per_sample_blocks(V, 1, N, 4096), (unsigned)N, (unsigned)cdiv(Cout, MAXC));
            if (vec) conv1_fwd_kernel<T, true, MAXC, 1><<<grid, BLK, 0, s>>>((const T*)z, zcs, Cin, w, bias, logits, Cout, V);
            else conv1_fwd_kernel<T, false, MAXC, 1><<<grid, BLK, 0, s>>>((const T*)z, zcs, Cin, w, bias, logits, Cout, V);
        }
        MI3D_LAUNCH_CHECK();
    });
    return 0;
}

size_t conv1_bwd_ws_floats(int Cin, int Cout) { return (size_t)8192 * ((size_t)Cin * Cout + Cout); }

int conv1_bwd(int dtype, const void* z, int zcs, int Cin, const float* w, const float* dlogits, int Cout, void* dz,
              int dzcs, float* dW, float* db, int accumulate, float* ws, int N, int64_t V, hipStream_t s, SlabJob* pend) {
    MI3D_CHECK_ARG(Cout <= MAXC, "conv1_bwd: out_channels %d > %d unsupported", Cout, MAXC);
    MI3D_CHECK_ARG(N <= CONV1_NBLK, "conv1_bwd: batch %d > %d unsupported", N, CONV1_NBLK);
    int64_t nW = (int64_t)Cin * Cout;
    int nslab = 0;
    // every slab element is written by exactly one (blockIdx.x, blockIdx.y, blockIdx.z) block
    if (dtype == MI3D_BF16 && Cin % 16 == 0 && zcs % 8 == 0 && al16(z) && (!dz || (dzcs % 4 == 0 && ((uintptr_t)dz % 8) == 0))) {
        const int capb = 1024;             // 8-wave workgroups, one slab each (conv1_bwd_ws_floats covers 8192)
        int64_t want = (V + C1W * 32 - 1) / (C1W * 32);       // voxels per workgroup iteration
        int bx = capb / N < 1 ? 1 : capb / N;
        if (bx > want) bx = (int)want;
        dim3 grid((unsigned)bx, (unsigned)N, (unsigned)(Cin / 16));
        conv1_bwd_mfma_kernel<<<grid, C1W * 64, 0, s>>>((const bf16*)z, zcs, Cin, w, dlogits, Cout, (bf16*)dz, dzcs, V, ws);
        MI3D_LAUNCH_CHECK();
        if (pend) { *pend = slab_job_make(0, ws, bx * N, nW + Cout, nW, dW, db, Cin, Cout, accumulate); return 0; }
        return slab_reduce(ws, bx * N, nW + Cout, nW, dW, db, accumulate, s);
    }
    DISPATCH_T(dtype, T, {
        bool vec = Cin % CINB == 0 && zcs % 8 == 0 && al16(z) && (!dz || (dzcs % 8 == 0 && al16(dz)));
        bool v4 = false;        // see conv1_fwd: one voxel per thread keeps the channel-row loads coalesced
        int bx = per_sample_blocks(V, v4 ? 4 : 1, N, CONV1_NBLK);
        nslab = bx * N;
        dim3 grid((unsigned)bx, (unsigned)N, (unsigned)cdiv(Cin, CINB));
        if (v4) conv1_bwd_kernel<T, true, 4, 4><<<grid, BLK, 0, s>>>((const T*)z, zcs, Cin, w, dlogits, Cout, (T*)dz, dzcs, V, ws);
        else if (vec && Cout <= 4) conv1_bwd_kernel<T, true, 4, 1><<<grid, BLK, 0, s>>>((const T*)z, zcs, Cin, w, dlogits, Cout, (T*)dz, dzcs, V, ws);
        else if (vec) conv1_bwd_kernel<T, true, MAXC, 1><<<grid, BLK, 0, s>>>((const T*)z, zcs, Cin, w, dlogits, Cout, (T*)dz, dzcs, V, ws);
        else if (Cout <= 4) conv1_bwd_kernel<T, false, 4, 1><<<grid, BLK, 0, s>>>((const T*)z, zcs, Cin, w, dlogits, Cout, (T*)dz, dzcs, V, ws);
        else conv1_bwd_kernel<T, false, MAXC, 1><<<grid, BLK, 0, s>>>((const T*)z, zcs, Cin, w, dlogits, Cout, (T*)dz, dzcs, V, ws);
        MI3D_LAUNCH_CHECK();
    });
    return slab_reduce(ws, nslab, nW + Cout, nW, dW, db, accumulate, s);
}

size_t seg_loss_ws_bytes(int C) { return (size_t)LOSS_MAXBLK * NQ * sizeof(double); }

int seg_loss_fwd(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int64_t V, LossCfg cfg,
                 float* loss_out, float* coef, void* ws, hipStream_t s, int D, float* metrics_out, void* metrics_ws) {
    MI3D_CHECK_ARG(C >= 1 && C <= MAXC, "seg_loss: %d classes unsupported (max %d)", C, MAXC);
    MI3D_CHECK_ARG(cfg.w_kd == 0.f || teacher, "seg_loss: distillation weight without teacher logits");
    MI3D_CHECK_ARG(N <= LOSS_MAXBLK, "seg_loss: batch %d > %d unsupported", N, LOSS_MAXBLK);
    const float* tch = cfg.w_kd != 0.f ? teacher : nullptr;
    bool v4 = vv4(V, logits, labels, tch);
    int bx = per_sample_blocks(V, v4 ? 4 : 1, N, LOSS_MAXBLK);
    dim3 grid((unsigned)bx, (unsigned)N);
    float it = 1.f / cfg.temp;
    bool met = metrics_out && metrics_ws;
    unsigned long long* cw = (unsigned long long*)metrics_ws;
#define SLF4(NC_, VV_, EX_, TE_, MA_)                                                                                     \
    do {                                                                                                                   \
        if (met) seg_loss_fwd_kernel<NC_, VV_, true, EX_, TE_, MA_><<<grid, BLK, 0, s>>>(logits, labels, tch, C, V, it, (double*)ws, cw, cfg.ignore);   \
        else seg_loss_fwd_kernel<NC_, VV_, false, EX_, TE_, MA_><<<grid, BLK, 0, s>>>(logits, labels, tch, C, V, it, (double*)ws, nullptr, cfg.ignore); \
    } while (0)
#define SLF3(NC_, VV_, EX_, TE_) do { if (cfg.mask) SLF4(NC_, VV_, EX_, TE_, true); else SLF4(NC_, VV_, EX_, TE_, false); } while (0)
#define SLF(NC_, VV_)                                                                                                      \
    do {                                                                                                                   \
        if (C == NC_ && tch) SLF3(NC_, VV_, true, true);                                                                  \
        else if (C == NC_) SLF3(NC_, VV_, true, false);                                                                   \
        else if (tch) SLF3(NC_, VV_, false, true);                                                                        \
        else SLF3(NC_, VV_, false, false);                                                                                \
    } while (0)
    if (C <= 4 && v4) SLF(4, 4);
    else if (C <= 4) SLF(4, 1);
    else if (v4) SLF(MAXC, 4);
    else SLF(MAXC, 1);
#undef SLF4
#undef SLF3
#undef SLF
    MI3D_LAUNCH_CHECK();
    if (met) seg_loss_metrics_finalize_kernel<<<1, 1024, 0, s>>>((const double*)ws, cw, bx * N, N, C, D, V, cfg, loss_out, coef, metrics_out);
    else seg_loss_finalize_kernel<<<1, 1024, 0, s>>>((const double*)ws, bx * N, N, C, V, cfg, loss_out, coef);
    MI3D_LAUNCH_CHECK();
    return 0;
}

int seg_loss_bwd(const float* logits, const int64_t* labels, const float* teacher, int N, int C, int64_t V, LossCfg cfg,
                 const float* coef, const float* grad_out, float* dlogits, hipStream_t s) {
    MI3D_CHECK_ARG(C >= 1 && C <= MAXC, "seg_loss_bwd: %d classes unsupported", C);
    MI3D_CHECK_ARG(cfg.w_kd == 0.f || teacher, "seg_loss_bwd: distillation weight without teacher logits");
    const float* tch = cfg.w_kd != 0.f ? teacher : nullptr;
    bool v4 = vv4(V, logits, labels, tch) && al16(dlogits);
    dim3 grid((unsigned)per_sample_blocks(V, v4 ? 4 : 1, N, 4096), (unsigned)N);
    float it = 1.f / cfg.temp;
#define SLB4(NC_, VV_, EX_, TE_, MA_) seg_loss_bwd_kernel<NC_, VV_, EX_, TE_, MA_><<<grid, BLK, 0, s>>>(logits, labels, tch, C, V, it, coef, grad_out, dlogits, cfg.ignore)
#define SLB3(NC_, VV_, EX_, TE_) do { if (cfg.mask) SLB4(NC_, VV_, EX_, TE_, true); else SLB4(NC_, VV_, EX_, TE_, false); } while (0)
#define SLB(NC_, VV_)                                                         \
    do {                                                                      \
        if (C == NC_ && tch) SLB3(NC_, VV_, true, true);                      \
        else if (C == NC_) SLB3(NC_, VV_, true, false);                       \
        else if (tch) SLB3(NC_, VV_, false, true);                            \
        else SLB3(NC_, VV_, false, false);                                    \
    } while (0)
    if (C <= 4 && v4) SLB(4, 4);
    else if (C <= 4) SLB(4, 1);
    else if (v4) SLB(MAXC, 4);
    else SLB(MAXC, 1);
#undef SLB
#undef SLB3
#undef SLB4
    MI3D_LAUNCH_CHECK();
    return 0;
}

size_t seg_metrics_ws_bytes(int C) { return (size_t)METRIC_BLOCKS * (3 * MAXC + 1) * sizeof(unsigned long long); }

int seg_metrics(const float* logits, const int64_t* labels, int N, int C, int D, int64_t V, float* out, void* ws,
                hipStream_t s, int64_t* counts_out) {
    MI3D_CHECK_ARG(C >= 1 && C <= MAXC, "seg_metrics: %d classes unsupported", C);
    MI3D_CHECK_ARG(N <= METRIC_BLOCKS, "seg_metrics: batch %d > %d unsupported", N, METRIC_BLOCKS);
    bool v4 = vv4(V, logits, labels);
    int bx = per_sample_blocks(V, v4 ? 4 : 1, N, METRIC_BLOCKS);
    dim3 grid((unsigned)bx, (unsigned)N);
    unsigned long long* cw = (unsigned long long*)ws;
    if (C <= 4 && v4) seg_metrics_kernel<4, 4><<<grid, BLK, 0, s>>>(logits, labels, C, V, cw);
    else if (C <= 4) seg_metrics_kernel<4, 1><<<grid, BLK, 0, s>>>(logits, labels, C, V, cw);
    else if (v4) seg_metrics_kernel<MAXC, 4><<<grid, BLK, 0, s>>>(logits, labels, C, V, cw);
    else seg_metrics_kernel<MAXC, 1><<<grid, BLK, 0, s>>>(logits, labels, C, V, cw);
    MI3D_LAUNCH_CHECK();
    if (out) seg_metrics_finalize_kernel<<<1, 1024, 0, s>>>((const unsigned long long*)ws, bx * N, N, C, D, V, out);
    if (counts_out) seg_counts_finalize_kernel<<<1, 1024, 0, s>>>((const unsigned long long*)ws, bx * N, C, (long long*)counts_out);
    MI3D_LAUNCH_CHECK();
    return 0;
}

// ---- head + argmax (+ per-sample counts)
constexpr int HEAD_LABEL_BLOCKS = 2048;      // partial rows in all: a streaming grid of eight 256-thread blocks per CU
static int head_labels_blocks(int N, int64_t V) {
    int64_t want = (V + BLK * HLV - 1) / (BLK * HLV), cap = HEAD_LABEL_BLOCKS / N < 1 ? 1 : HEAD_LABEL_BLOCKS / N;
    return (int)(want < cap ? want : cap);
}
size_t head_labels_ws_bytes(int N, int Cout) {
    if (N < 1 || Cout < 1 || Cout > MAXC) return 0;
    return (size_t)(N > HEAD_LABEL_BLOCKS ? N : HEAD_LABEL_BLOCKS) * (3 * Cout + 1) * sizeof(unsigned long long);
}

int head_labels(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, int Cout, int N, int64_t V,
                uint8_t* labels, const int64_t* target, int64_t* counts, void* ws, hipStream_t s) {
    MI3D_CHECK_ARG(Cin >= 1 && zcs >= Cin, "head_labels: bad channels (Cin %d, stride %d)", Cin, zcs);
    MI3D_CHECK_ARG(Cout >= 1 && Cout <= MAXC, "head_labels: %d classes unsupported (max %d)", Cout, MAXC);
    MI3D_CHECK_ARG(N >= 1 && N <= 65535 && V >= 1, "head_labels: bad batch %d or volume %lld", N, (long long)V);
    MI3D_CHECK_ARG(!target == !counts, "head_labels: target and counts come together");
    MI3D_CHECK_ARG(!target || ws, "head_labels: counts need the workspace");
    dim3 grid((unsigned)head_labels_blocks(N, V), (unsigned)N);
    unsigned long long* rows = (unsigned long long*)ws;
    const bool vec = Cin % CINB == 0 && zcs % 8 == 0 && al16(z);      // as conv1_fwd
#define HLAB(VEC_, NC_)                                                                                                                          \
    do {                                                                                                                                          \
        if (target) head_labels_kernel<T, VEC_, NC_, true><<<grid, BLK, 0, s>>>((const T*)z, zcs, Cin, w, bias, Cout, V, labels, target, rows);   \
        else head_labels_kernel<T, VEC_, NC_, false><<<grid, BLK, 0, s>>>((const T*)z, zcs, Cin, w, bias, Cout, V, labels, nullptr, nullptr);     \
    } while (0)
    DISPATCH_T(dtype, T, {
        if (vec && Cout <= 4) HLAB(true, 4);
        else if (vec) HLAB(true, MAXC);
        else if (Cout <= 4) HLAB(false, 4);
        else HLAB(false, MAXC);
        MI3D_LAUNCH_CHECK();
    });
#undef HLAB
    if (target) {
        seg_counts_finalize_kernel<<<N, 1024, 0, s>>>(rows, (int)grid.x, Cout, (long long*)counts);
        MI3D_LAUNCH_CHECK();
    }
    return 0;
}

// ---- head + softmax + vote of one view (+ argmax, counts, confidence on the last)
int head_votes(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, int Cout, int N, int D, int H, int W,
               int flip, int view, int views, int flags, float* votes, uint8_t* labels, float* confidence, const int64_t* target,
               int64_t* counts, void* ws, hipStream_t s) {
    MI3D_CHECK_ARG(Cin >= 1 && zcs >= Cin, "head_votes: bad channels (Cin %d, stride %d)", Cin, zcs);
    MI3D_CHECK_ARG(Cout >= 1 && Cout <= MAXC, "head_votes: %d classes unsupported (max %d)", Cout, MAXC);
    MI3D_CHECK_ARG(N >= 1 && N <= 65535 && D >= 1 && H >= 1 && W >= 1 && (int64_t)D * H * W < (1ll << 31),
                   "head_votes: bad batch %d or volume %d x %d x %d (below 2^31 voxels per sample)", N, D, H, W);
    MI3D_CHECK_ARG(flip >= 0 && flip < 8, "head_votes: flip code %d outside [0, 8)", flip);
    MI3D_CHECK_ARG(views >= 1 && view >= 0 && view < views, "head_votes: view %d outside [0, %d)", view, views);
    MI3D_CHECK_ARG((flags & ~MI3D_VOTES_KEEP) == 0, "head_votes: unknown flags 0x%x", flags);
    const bool first = view == 0, last = view == views - 1, keep = (flags & MI3D_VOTES_KEEP) != 0;
    if (!last) {
        MI3D_CHECK_ARG(!labels && !confidence && !target && !counts,
                       "head_votes: labels, confidence, target and counts belong to the last view (view %d of %d)", view, views);
    } else {
        MI3D_CHECK_ARG(labels, "head_votes: the last view needs labels_out");
        MI3D_CHECK_ARG(!target == !counts, "head_votes: target and counts come together");
        MI3D_CHECK_ARG(!target || ws, "head_votes: counts need the workspace");
    }
    MI3D_CHECK_ARG(votes || (views == 1 && !keep), "head_votes: the vote volume is NULL (only a single view that does not keep it may)");
    const int64_t V = (int64_t)D * H * W;
    // a thread owns 4 consecutive voxels where every plane, label and confidence access of a group is aligned
    const bool v4 = V % 4 == 0 && al16(votes) && (uintptr_t)labels % 4 == 0 && al16(confidence);
    const int64_t want = (V / (v4 ? 4 : 1) + BLK - 1) / BLK, cap = HEAD_LABEL_BLOCKS / N < 1 ? 1 : HEAD_LABEL_BLOCKS / N;
    dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)N);
    unsigned long long* rows = (unsigned long long*)ws;
    const bool vec = Cin % CINB == 0 && zcs % 8 == 0 && al16(z);      // as conv1_fwd
#define HVOTE(VEC_, NC_, VV_, MODE_, TGT_)                                                                                                \
    head_votes_kernel<T, VEC_, NC_, VV_, MODE_, TGT_><<<grid, BLK, 0, s>>>((const T*)z, zcs, Cin, w, bias, Cout, D, H, W, flip, (float)views, \
                                                                           keep ? 1 : 0, votes, labels, confidence, target, rows)
#define HVOTE_MODE(VEC_, NC_, VV_)                                                                                                        \
    do {                                                                                                                                   \
        if (last && target) { if (first) HVOTE(VEC_, NC_, VV_, VOTE_FIRST | VOTE_LAST, true); else HVOTE(VEC_, NC_, VV_, VOTE_LAST, true); }   \
        else if (last) { if (first) HVOTE(VEC_, NC_, VV_, VOTE_FIRST | VOTE_LAST, false); else HVOTE(VEC_, NC_, VV_, VOTE_LAST, false); }      \
        else if (first) HVOTE(VEC_, NC_, VV_, VOTE_FIRST, false);                                                                          \
        else HVOTE(VEC_, NC_, VV_, 0, false);                                                                                              \
    } while (0)
#define HVOTE_VV(VEC_, NC_)                  \
    do {                                     \
        if (v4) HVOTE_MODE(VEC_, NC_, 4);    \
        else HVOTE_MODE(VEC_, NC_, 1);       \
    } while (0)
    DISPATCH_T(dtype, T, {
        if (vec && Cout <= 4) HVOTE_VV(true, 4);
        else if (vec) HVOTE_VV(true, MAXC);
        else if (Cout <= 4) HVOTE_VV(false, 4);
        else HVOTE_VV(false, MAXC);
        MI3D_LAUNCH_CHECK();
    });
#undef HVOTE_VV
#undef HVOTE_MODE
#undef HVOTE
    if (last && target) {
        seg_counts_finalize_kernel<<<N, 1024, 0, s>>>(rows, (int)grid.x, Cout, (long long*)counts);
        MI3D_LAUNCH_CHECK();
    }
    return 0;
}

// ---- head + softmax + weighted vote of N window samples into one accumulator (contract: include/mi3d.h mi3d_head_votes_window)
int head_votes_window(int dtype, const void* z, int zcs, int Cin, const float* w, const float* bias, int Cout, int N, int d, int h, int wd,
                      const int* flips, const float* gd, const float* gh, const float* gw, const int* origins, float* acc, int D, int H,
                      int W, hipStream_t s) {
    MI3D_CHECK_ARG(Cin >= 1 && zcs >= Cin, "head_votes_window: bad channels (Cin %d, stride %d)", Cin, zcs);
    MI3D_CHECK_ARG(Cout >= 1 && Cout <= MAXC, "head_votes_window: %d classes unsupported (max %d)", Cout, MAXC);
    MI3D_CHECK_ARG(D >= 1 && H >= 1 && W >= 1 && (int64_t)D * H * W < (1ll << 31),
                   "head_votes_window: bad volume %d x %d x %d (below 2^31 voxels)", D, H, W);
    MI3D_CHECK_ARG(N >= 1 && N <= 65535 && d >= 1 && h >= 1 && wd >= 1 && d <= D && h <= H && wd <= W,
                   "head_votes_window: bad batch %d or window %d x %d x %d (inside the volume %d x %d x %d)", N, d, h, wd, D, H, W);
    MI3D_CHECK_ARG(gd && gh && gw, "head_votes_window: a weight table is NULL");
    MI3D_CHECK_ARG(flips && origins && acc, "head_votes_window: flips, origins or the accumulator is NULL");
    for (int n = 0; n < N; n++) {
        const int* o = origins + 3 * n;
        MI3D_CHECK_ARG(flips[n] >= 0 && flips[n] < 8, "head_votes_window: flip code %d of sample %d outside [0, 8)", flips[n], n);
        MI3D_CHECK_ARG(o[0] >= 0 && o[0] <= D - d && o[1] >= 0 && o[1] <= H - h && o[2] >= 0 && o[2] <= W - wd,
                       "head_votes_window: sample %d at (%d, %d, %d) leaves the window outside the volume", n, o[0], o[1], o[2]);
    }
    const int64_t V = (int64_t)D * H * W, v = (int64_t)d * h * wd;
    const bool vec = Cin % CINB == 0 && zcs % 8 == 0 && al16(z);      // as conv1_fwd; a sample is a whole number of channel rows
#define HWIN(VEC_, NC_, VV_)                                                                                                           \
    head_votes_window_kernel<T, VEC_, NC_, VV_><<<grid, BLK, 0, s>>>((const T*)z + (int64_t)n * v * zcs, zcs, Cin, w, bias, Cout, d, h, wd, \
                                                                     flips[n], gd, gh, gw, o[0], o[1], o[2], acc, H, W, V)
#define HWIN_VV(VEC_, NC_)             \
    do {                               \
        if (v4) HWIN(VEC_, NC_, 4);    \
        else HWIN(VEC_, NC_, 1);       \
    } while (0)
    for (int n = 0; n < N; n++) {          // the samples may overlap in acc: the stream keeps them in sample order
        const int* o = origins + 3 * n;
        // a thread owns 4 consecutive voxels where a group stays in one window row and is aligned in every plane
        const bool v4 = W % 4 == 0 && wd % 4 == 0 && o[2] % 4 == 0 && al16(acc);
        const int64_t want = (v / (v4 ? 4 : 1) + BLK - 1) / BLK;
        dim3 grid((unsigned)(want < HEAD_LABEL_BLOCKS ? want : HEAD_LABEL_BLOCKS));
        DISPATCH_T(dtype, T, {
            if (vec && Cout <= 4) HWIN_VV(true, 4);
            else if (vec) HWIN_VV(true, MAXC);
            else if (Cout <= 4) HWIN_VV(false, 4);
            else HWIN_VV(false, MAXC);
            MI3D_LAUNCH_CHECK();
        });
    }
#undef HWIN_VV
#undef HWIN
    return 0;
}

// ---- labels, confidence, mean probabilities and counts from the weighted totals (contract: include/mi3d.h mi3d_votes_finish)
int votes_finish(float* acc, int Cout, int D, int H, int W, const float* nd, const float* nh, const float* nw, int views, int flags,
                 uint8_t* labels, float* confidence, const int64_t* target, int64_t* counts, void* ws, hipStream_t s) {
    MI3D_CHECK_ARG(acc && labels, "votes_finish: the accumulator or labels_out is NULL");
    MI3D_CHECK_ARG(Cout >= 1 && Cout <= MAXC, "votes_finish: %d classes unsupported (max %d)", Cout, MAXC);
    MI3D_CHECK_ARG(D >= 1 && H >= 1 && W >= 1 && (int64_t)D * H * W < (1ll << 31),
                   "votes_finish: bad volume %d x %d x %d (below 2^31 voxels)", D, H, W);
    MI3D_CHECK_ARG(nd && nh && nw, "votes_finish: a norm table is NULL");
    MI3D_CHECK_ARG(views >= 1, "votes_finish: %d views per window", views);
    MI3D_CHECK_ARG((flags & ~MI3D_VOTES_NORMALIZE) == 0, "votes_finish: unknown flags 0x%x", flags);
    MI3D_CHECK_ARG(!target == !counts, "votes_finish: target and counts come together");
    MI3D_CHECK_ARG(!target || ws, "votes_finish: counts need the workspace");
    const int64_t V = (int64_t)D * H * W;
    const bool v4 = W % 4 == 0 && al16(acc) && (uintptr_t)labels % 4 == 0 && al16(confidence);
    const int64_t want = (V / (v4 ? 4 : 1) + BLK - 1) / BLK;
    dim3 grid((unsigned)(want < HEAD_LABEL_BLOCKS ? want : HEAD_LABEL_BLOCKS));
    unsigned long long* rows = (unsigned long long*)ws;
    const int normalize = (flags & MI3D_VOTES_NORMALIZE) != 0;
#define VFIN(NC_, VV_, TGT_) \
    votes_finish_kernel<NC_, VV_, TGT_><<<grid, BLK, 0, s>>>(acc, Cout, D, H, W, nd, nh, nw, (float)views, normalize, labels, confidence, target, rows)
#define VFIN_VV(NC_)                                                      \
    do {                                                                  \
        if (v4) { if (target) VFIN(NC_, 4, true); else VFIN(NC_, 4, false); } \
        else { if (target) VFIN(NC_, 1, true); else VFIN(NC_, 1, false); }    \
    } while (0)
    if (Cout <= 4) VFIN_VV(4);
    else VFIN_VV(MAXC);
    MI3D_LAUNCH_CHECK();
#undef VFIN_VV
#undef VFIN
    if (target) {
        seg_counts_finalize_kernel<<<1, 1024, 0, s>>>(rows, (int)grid.x, Cout, (long long*)counts);
        MI3D_LAUNCH_CHECK();
    }
    return 0;
}

// ---- head + loss fused (training step)
bool head_loss_ok(int dtype, const void* z, int zcs, int Cin, int C, LossCfg cfg) {
    return dtype == MI3D_BF16 && Cin % CINB == 0 && zcs % 8 == 0 && al16(z) && C >= 1 && C <= 4 && !mi3d_routes().no_head_loss;
}
bool head_loss_bwd_ok(int dtype, const void* z, int zcs, int Cin, int C, LossCfg cfg, const void* dz, int dzcs) {
    return head_loss_ok(dtype, z, zcs, Cin, C, cfg) && Cin == 16 && (!dz || (dzcs % 4 == 0 && ((uintptr_t)dz % 8) == 0));
}

int head_loss_fwd(const void* z, int zcs, int Cin, const float* w, const float* bias, const int64_t* labels, const float* teacher,
                  int N, int C, int64_t V, LossCfg cfg, float* loss_out, float* coef, void* ws, hipStream_t s, int D, float* metrics_out,
                  void* metrics_ws, float* logits_opt) {
    MI3D_CHECK_ARG(head_loss_ok(MI3D_BF16, z, zcs, Cin, C, cfg), "head_loss_fwd: unsupported shape Cin=%d C=%d", Cin, C);
    MI3D_CHECK_ARG(cfg.w_kd == 0.f || teacher, "head_loss_fwd: distillation weight without teacher logits");
    const float* tch = cfg.w_kd != 0.f ? teacher : nullptr;
    const float it = 1.f / cfg.temp;
    MI3D_CHECK_ARG(N <= LOSS_MAXBLK, "head_loss_fwd: batch %d > %d unsupported", N, LOSS_MAXBLK);
    int64_t wantb = (V + HLW * 64 - 1) / (HLW * 64), capb = LOSS_MAXBLK / N < 1 ? 1 : LOSS_MAXBLK / N;
    int bx = (int)(wantb < capb ? wantb : capb);
    dim3 grid((unsigned)bx, (unsigned)N);
    bool met = metrics_out && metrics_ws;
    unsigned long long* cw = (unsigned long long*)metrics_ws;
    const bf16* zp = (const bf16*)z;
#define HLF4(ME_, EX_, TE_, MA_) head_loss_fwd_kernel<4, ME_, EX_, TE_, MA_><<<grid, HLW * 64, 0, s>>>(zp, zcs, Cin, w, bias, labels, tch, it, C, V, (double*)ws, cw, logits_opt, cfg.ignore)
#define HLF3(ME_, EX_, TE_) do { if (cfg.mask) HLF4(ME_, EX_, TE_, true); else HLF4(ME_, EX_, TE_, false); } while (0)
#define HLF(ME_, EX_) do { if (tch) HLF3(ME_, EX_, true); else HLF3(ME_, EX_, false); } while (0)
    if (met && C == 4) HLF(true, true);
    else if (met) HLF(true, false);
    else if (C == 4) HLF(false, true);
    else HLF(false, false);
#undef HLF
#undef HLF3
#undef HLF4
    MI3D_LAUNCH_CHECK();
    if (met) seg_loss_metrics_finalize_kernel<<<1, 1024, 0, s>>>((const double*)ws, cw, bx * N, N, C, D, V, cfg, loss_out, coef, metrics_out);
    else seg_loss_finalize_kernel<<<1, 1024, 0, s>>>((const double*)ws, bx * N, N, C, V, cfg, loss_out, coef);
    MI3D_LAUNCH_CHECK();
    return 0;
}

int head_loss_bwd(const void* z, int zcs, int Cin, const float* w, const float* bias, const int64_t* labels, const float* teacher, int C,
                  LossCfg cfg, const float* coef, const float* grad_out, void* dz, int dzcs, float* dW, float* db, int accumulate,
                  float* ws, int N, int64_t V, hipStream_t s, SlabJob* pend) {
    MI3D_CHECK_ARG(head_loss_bwd_ok(MI3D_BF16, z, zcs, Cin, C, cfg, dz, dzcs), "head_loss_bwd: unsupported shape Cin=%d C=%d", Cin, C);
    MI3D_CHECK_ARG(cfg.w_kd == 0.f || teacher, "head_loss_bwd: distillation weight without teacher logits");
    const float* tch = cfg.w_kd != 0.f ? teacher : nullptr;
    const float it = 1.f / cfg.temp;
    MI3D_CHECK_ARG(N <= CONV1_NBLK, "head_loss_bwd: batch %d > %d unsupported", N, CONV1_NBLK);
    int64_t nW = (int64_t)Cin * C;
    const int capb = 1024;             // as conv1_bwd's matrix-core route: same workgroup -> voxel map, same slabs
    int64_t want = (V + C1W * 32 - 1) / (C1W * 32);
    int bx = capb / N < 1 ? 1 : capb / N;
    if (bx > want) bx = (int)want;
    dim3 grid((unsigned)bx, (unsigned)N, 1);
#define HLB(TE_, MA_) head_loss_bwd_mfma_kernel<TE_, MA_><<<grid, C1W * 64, 0, s>>>((const bf16*)z, zcs, w, bias, labels, tch, it, C, coef, grad_out, (bf16*)dz, dzcs, V, ws, cfg.ignore)
    if (tch && cfg.mask) HLB(true, true);
    else if (tch) HLB(true, false);
    else if (cfg.mask) HLB(false, true);
    else HLB(false, false);
#undef HLB
    MI3D_LAUNCH_CHECK();
    if (pend) { *pend = slab_job_make(0, ws, bx * N, nW + C, nW, dW, db, Cin, C, accumulate); return 0; }
    return slab_reduce(ws, bx * N, nW + C, nW, dW, db, accumulate, s);
}
