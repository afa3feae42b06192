// entropy_loss.hip — entropy minimisation (MinEnt of ADVENT, Vu et al., CVPR 2019) on the logits: the mean over the volume of the
// Shannon entropy of softmax(logits) at the selected voxels, in units of ln C, and its gradient.  A sibling of boundary_loss.hip.
// Contract: include/mi3d.h mi3d_entropy_loss.  Per voxel, in the log-sum-exp form (p log p is never formed: a saturated voxel gives
// exactly 0, never a NaN):
//     d_j = z_j - max z,  e_j = exp(d_j),  se = sum e_j,  p_j = e_j / se,  H = log(se) - sum_j p_j d_j
//     loss (+)= weight * sum_selected H / (N V ln C)      dlogits[k] (+)= grad_scale * weight / (N V ln C) * p_k (log(se) - d_k - H)
// The divisor does not depend on what is selected, so the gradient of a voxel needs nothing but the voxel: value and gradient leave
// ONE pass.  An unselected voxel adds nothing to the sum; its gradient is 0, and under ADD_GRAD its dlogits keep their bits.
//
// One streaming pass, HBM-bound: 4 C bytes read and 4 C written per voxel (+ 4 C read under ADD_GRAD, + 8 with labels).
// grid = (blocks, N).  VV = 4: a thread owns four consecutive voxels of one sample, every plane of the channel-planar logits and
// gradients is one 16-byte access; VV = 1 is the same per-voxel code for V % 4 != 0 or pointers that are not 16-byte aligned.  C is a
// template argument: the logits of a voxel stay in registers.
// The sum: float32 per voxel, double from the thread's accumulator on; a fixed shuffle tree per wave, the waves in ascending order,
// one double per workgroup in its own slot; the finishing launch adds the slots in a fixed order.  No float atomics: the same bits
// on every run.
#include "../../include/mi3d.h"
#include "ops.h"

namespace {
constexpr int BLK = 256, NW = BLK / 64;
constexpr int MAXC = MI3D_MAX_CLASSES;
constexpr int ENT_BLOCKS = 2048;         // in all: eight 256-thread blocks per CU, as the other streaming passes

// want_ignored: MI3D_ENT_IGNORED selects labels == ign, MI3D_ENT_COUNTED labels != ign (read only where MASKED)
template <int NC, int VV, bool MASKED, bool GRAD, bool ADD>
__global__ __launch_bounds__(BLK) void entropy_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, long long ign,
                                                      bool want_ignored, int64_t V, float wn, const float* __restrict__ grad_scale,
                                                      float* dlogits, double* __restrict__ partial) {
    __shared__ double wave_sum[NW];
    const int n = blockIdx.y;
    const float* zn = logits + (int64_t)n * NC * V;
    float* dn = GRAD ? dlogits + (int64_t)n * NC * V : nullptr;
    const int64_t* ln = MASKED ? labels + (int64_t)n * V : nullptr;
    const float s = GRAD ? (grad_scale ? grad_scale[0] : 1.f) * wn : 0.f;
    double acc = 0.0;
    const int64_t ngrp = V / VV;
    for (int64_t grp = (int64_t)blockIdx.x * BLK + threadIdx.x; grp < ngrp; grp += (int64_t)gridDim.x * BLK) {
        const int64_t v0 = grp * VV;
        float z[NC][VV];
        bool sel[VV];
#pragma unroll
        for (int j = 0; j < NC; j++) {
            if constexpr (VV == 4) {
                const float4 a = *reinterpret_cast<const float4*>(zn + j * V + v0);
                z[j][0] = a.x, z[j][1] = a.y, z[j][2] = a.z, z[j][3] = a.w;
            } else {
                z[j][0] = zn[j * V + v0];
            }
        }
        if constexpr (MASKED && VV == 4) {
            const longlong2 a = *reinterpret_cast<const longlong2*>(ln + v0), b = *reinterpret_cast<const longlong2*>(ln + v0 + 2);
            sel[0] = (a.x == ign) == want_ignored, sel[1] = (a.y == ign) == want_ignored;
            sel[2] = (b.x == ign) == want_ignored, sel[3] = (b.y == ign) == want_ignored;
        } else if constexpr (MASKED) {
            sel[0] = (ln[v0] == ign) == want_ignored;
        } else {
#pragma unroll
            for (int k = 0; k < VV; k++) sel[k] = true;
        }
        float g[NC][VV];
#pragma unroll
        for (int k = 0; k < VV; k++) {
            float mx = z[0][k];
#pragma unroll
            for (int j = 1; j < NC; j++) mx = fmaxf(mx, z[j][k]);
            float d[NC], p[NC], se = 0.f;
#pragma unroll
            for (int j = 0; j < NC; j++) d[j] = z[j][k] - mx, p[j] = expf(d[j]), se += p[j];
            const float inv = 1.f / se, lse = logf(se);
            float pd = 0.f;
#pragma unroll
            for (int j = 0; j < NC; j++) p[j] *= inv, pd += p[j] * d[j];
            const float h = lse - pd;
            if (sel[k]) acc += (double)h;
#pragma unroll
            for (int j = 0; j < NC; j++) g[j][k] = s * p[j] * (lse - d[j] - h);
        }
        if constexpr (GRAD) {
#pragma unroll
            for (int j = 0; j < NC; j++) {
                float* o_at = dn + j * V + v0;
                if constexpr (VV == 4) {
                    float4 o = float4{0.f, 0.f, 0.f, 0.f};
                    if constexpr (ADD) o = *reinterpret_cast<const float4*>(o_at);
                    // an unselected voxel: a zero, or under ADD the value that was there, bit for bit
                    o.x = sel[0] ? (ADD ? o.x + g[j][0] : g[j][0]) : o.x;
                    o.y = sel[1] ? (ADD ? o.y + g[j][1] : g[j][1]) : o.y;
                    o.z = sel[2] ? (ADD ? o.z + g[j][2] : g[j][2]) : o.z;
                    o.w = sel[3] ? (ADD ? o.w + g[j][3] : g[j][3]) : o.w;
                    *reinterpret_cast<float4*>(o_at) = o;
                } else {
                    const float o = ADD ? o_at[0] : 0.f;
                    o_at[0] = sel[0] ? (ADD ? o + g[j][0] : g[j][0]) : o;
                }
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = wave_sum[0];
        for (int w = 1; w < NW; w++) sum = sum + wave_sum[w];
        partial[(int64_t)n * gridDim.x + blockIdx.x] = sum;          // every workgroup writes its slot
    }
}

// One workgroup: thread t adds the slots t, t + 256, ... in that order, then the fixed tree.  loss (+)= (float)(weight * sum / (N V ln C)).
__global__ __launch_bounds__(BLK) void entropy_finish_kernel(const double* __restrict__ partial, int64_t slots, double w_over_nvl, int add,
                                                             float* loss_out) {
    __shared__ double wave_sum[NW];
    double acc = 0.0;
    for (int64_t b = threadIdx.x; b < slots; b += BLK) acc = acc + partial[b];
    for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = wave_sum[0];
        for (int w = 1; w < NW; w++) sum = sum + wave_sum[w];
        const float term = (float)(sum * w_over_nvl);
        loss_out[0] = add ? loss_out[0] + term : term;
    }
}

int64_t blocks_per_sample(int N, int64_t groups) {
    const int64_t want = (groups + BLK - 1) / BLK, cap = ENT_BLOCKS / N < 1 ? 1 : ENT_BLOCKS / N;
    return want < cap ? want : cap;
}

template <int NC, int VV, bool MASKED, bool GRAD>
void launch_add(bool add, dim3 grid, hipStream_t s, const float* logits, const int64_t* labels, long long ign, bool want_ignored, int64_t V,
                float wn, const float* grad_scale, float* dlogits, double* partial) {
    if (add) entropy_kernel<NC, VV, MASKED, GRAD, true><<<grid, BLK, 0, s>>>(logits, labels, ign, want_ignored, V, wn, grad_scale, dlogits, partial);
    else entropy_kernel<NC, VV, MASKED, GRAD, false><<<grid, BLK, 0, s>>>(logits, labels, ign, want_ignored, V, wn, grad_scale, dlogits, partial);
}
template <int NC, int VV, typename... A> void launch_variant(bool masked, bool grad, bool add, A... a) {
    if (masked && grad) launch_add<NC, VV, true, true>(add, a...);
    else if (masked) launch_add<NC, VV, true, false>(false, a...);
    else if (grad) launch_add<NC, VV, false, true>(add, a...);
    else launch_add<NC, VV, false, false>(false, a...);
}
template <int NC, typename... A> void launch_width(bool v4, A... a) {
    if (v4) launch_variant<NC, 4>(a...);
    else launch_variant<NC, 1>(a...);
}
template <typename... A> void launch_classes(int C, A... a) {
    switch (C) {
        case 2: launch_width<2>(a...); break;
        case 3: launch_width<3>(a...); break;
        case 4: launch_width<4>(a...); break;
        case 5: launch_width<5>(a...); break;
        case 6: launch_width<6>(a...); break;
        case 7: launch_width<7>(a...); break;
        default: launch_width<8>(a...); break;
    }
}
}  // namespace

extern "C" {

size_t mi3d_entropy_loss_workspace_bytes(int N, int64_t V) {
    if (N < 1 || N > 65535 || V < 1) {
        mi3d_set_error("mi3d_entropy_loss_workspace_bytes: N in [1, 65535] and V >= 1 expected, got %d and %lld", N, (long long)V);
        return 0;
    }
    return (size_t)(N * blocks_per_sample(N, V)) * sizeof(double);          // the scalar route has the most workgroups
}

int mi3d_entropy_loss(const float* logits, int N, int C, int64_t V, const int64_t* labels, const int64_t* ignore_index, int mode,
                      float weight, const float* grad_scale, float* loss_out, float* dlogits, int flags, void* workspace,
                      size_t workspace_bytes, void* stream) {
    const char* name = "mi3d_entropy_loss";
    MI3D_CHECK_ARG(logits && loss_out, "%s: null pointer (logits or loss_out)", name);
    MI3D_CHECK_ARG(N >= 1 && N <= 65535 && V >= 1, "%s: N in [1, 65535] and V >= 1 expected, got %d and %lld", name, N, (long long)V);
    MI3D_CHECK_ARG(C >= 2 && C <= MAXC, "%s: 2 to %d logit channels (ln 1 = 0 divides nothing), got %d", name, MAXC, C);
    MI3D_CHECK_ARG(mode == MI3D_ENT_ALL || mode == MI3D_ENT_COUNTED || mode == MI3D_ENT_IGNORED, "%s: unknown mode %d", name, mode);
    MI3D_CHECK_ARG((labels != nullptr) == (ignore_index != nullptr), "%s: labels and ignore_index come together or not at all", name);
    MI3D_CHECK_ARG(mode == MI3D_ENT_ALL || labels, "%s: mode %d selects by label: labels and ignore_index are required", name, mode);
    MI3D_CHECK_ARG(weight == weight && weight - weight == 0.f, "%s: weight %g is not finite", name, (double)weight);
    MI3D_CHECK_ARG((flags & ~(MI3D_ENT_ADD_LOSS | MI3D_ENT_ADD_GRAD)) == 0, "%s: unknown flags 0x%x", name, flags);
    MI3D_CHECK_ARG(dlogits || !(flags & MI3D_ENT_ADD_GRAD), "%s: MI3D_ENT_ADD_GRAD without dlogits", name);
    MI3D_CHECK_ARG(((uintptr_t)logits | (uintptr_t)loss_out | (uintptr_t)dlogits | (uintptr_t)grad_scale) % 4 == 0 && (uintptr_t)labels % 8 == 0,
                   "%s: a float pointer is not 4-byte or labels not 8-byte aligned", name);
    MI3D_CHECK_ARG(workspace && (uintptr_t)workspace % 8 == 0, "%s: the workspace must be a non-null, 8-byte aligned pointer", name);
    const size_t needed = mi3d_entropy_loss_workspace_bytes(N, V);
    MI3D_CHECK_ARG(workspace_bytes >= needed, "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, needed);
    const bool masked = mode != MI3D_ENT_ALL;          // mode ALL with labels given: they are not read
    const bool v4 = V % 4 == 0 && ((uintptr_t)logits | (uintptr_t)dlogits | (uintptr_t)(masked ? labels : nullptr)) % 16 == 0;
    const int64_t blocks = blocks_per_sample(N, V / (v4 ? 4 : 1));
    const double w_over_nvl = (double)weight / ((double)N * (double)V * log((double)C));
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)blocks, (unsigned)N);
    double* partial = static_cast<double*>(workspace);
    launch_classes(C, v4, masked, dlogits != nullptr, (flags & MI3D_ENT_ADD_GRAD) != 0, grid, s, logits, masked ? labels : nullptr,
                   (long long)(ignore_index ? *ignore_index : 0), mode == MI3D_ENT_IGNORED, V, (float)w_over_nvl, grad_scale, dlogits, partial);
    MI3D_LAUNCH_CHECK();
    entropy_finish_kernel<<<1, BLK, 0, s>>>(partial, (int64_t)N * blocks, w_over_nvl, (flags & MI3D_ENT_ADD_LOSS) != 0, loss_out);
    MI3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
