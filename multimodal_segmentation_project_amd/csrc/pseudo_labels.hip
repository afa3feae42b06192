// pseudo_labels.hip — self-training targets from a prediction: the uint8 label map and the float32 confidence map of
// segment.predict_labels_ensemble / predict_labels_sliding become the int64 target of the masked loss (head_loss.hip, MASK),
//     target[n][v] = (label < C && conf >= thr[label]) ? label : ignore_index
// plus, per sample, the voxels kept per class and the voxels ignored.  Contract: include/mi3d.h mi3d_pseudo_labels.
//
// One streaming pass, HBM-bound: 1 + 4 bytes read and 8 written per voxel.  grid = (blocks, N).  VV = 4: a thread owns four
// consecutive voxels of one sample -- the labels are one 4-byte load, the confidences one 16-byte load, the targets two 16-byte
// stores next to each other (load_labels' pattern in head_loss.hip, mirrored).  VV = 1 is the same per-voxel code for V % 4 != 0
// or pointers that are not aligned.  A NaN confidence fails `>=` and is ignored.
// The table is integer adds only: per-thread counters -> wave sums -> LDS -> ONE 64-bit integer atomic per block and column onto
// the table the launcher cleared on the same stream.  Integer addition commutes, so the table is exact and the same on every run.
#include "../../include/mi3d.h"
#include "ops.h"

namespace {
constexpr int BLK = 256;
constexpr int MAXC = MI3D_MAX_CLASSES;
constexpr int PSEUDO_BLOCKS = 2048;      // in all: eight 256-thread blocks per CU, as the other streaming label passes
struct Thresholds { float t[MAXC]; };

template <int VV>
__global__ __launch_bounds__(BLK) void pseudo_labels_kernel(const uint8_t* __restrict__ labels, const float* __restrict__ conf, int64_t V,
                                                            int C, Thresholds thr, long long ign, int64_t* __restrict__ target,
                                                            unsigned long long* __restrict__ table) {
    __shared__ unsigned red[BLK / 64][MAXC + 1];
    const int n = blockIdx.y;
    const uint8_t* ln = labels + (int64_t)n * V;
    const float* cn = conf + (int64_t)n * V;
    int64_t* tn = target + (int64_t)n * V;
    unsigned cnt[MAXC + 1];                  // kept per class, then ignored; a thread sees < 2^32 voxels
#pragma unroll
    for (int c = 0; c <= MAXC; c++) cnt[c] = 0;
    const int64_t ngrp = V / VV;
    // one group per thread and trip: a second group in flight per thread (loads of both issued first) was built and timed at 192^3
    // and changed nothing (46.3 us against 46.4 us for the call), so the plain walk stays
    for (int64_t grp = (int64_t)blockIdx.x * BLK + threadIdx.x; grp < ngrp; grp += (int64_t)gridDim.x * BLK) {
        const int64_t v0 = grp * VV;
        unsigned lab[VV];
        float cf[VV];
        if constexpr (VV == 4) {
            const unsigned w = *reinterpret_cast<const unsigned*>(ln + v0);
            const float4 f = *reinterpret_cast<const float4*>(cn + v0);
            lab[0] = w & 255u; lab[1] = (w >> 8) & 255u; lab[2] = (w >> 16) & 255u; lab[3] = w >> 24;
            cf[0] = f.x; cf[1] = f.y; cf[2] = f.z; cf[3] = f.w;
        } else {
            lab[0] = ln[v0];
            cf[0] = cn[v0];
        }
        long long o[VV];
#pragma unroll
        for (int k = 0; k < VV; k++) {
            float th = 0.f;
            bool known = false;              // label < C
#pragma unroll
            for (int c = 0; c < MAXC; c++) {
                const bool is = c < C && lab[k] == (unsigned)c;
                th = is ? thr.t[c] : th;
                known = known || is;
            }
            const bool keep = known && cf[k] >= th;
            o[k] = keep ? (long long)lab[k] : ign;
#pragma unroll
            for (int c = 0; c < MAXC; c++) cnt[c] += (keep && lab[k] == (unsigned)c) ? 1u : 0u;
            cnt[MAXC] += keep ? 0u : 1u;
        }
        if constexpr (VV == 4) {
            *reinterpret_cast<longlong2*>(tn + v0) = longlong2{o[0], o[1]};
            *reinterpret_cast<longlong2*>(tn + v0 + 2) = longlong2{o[2], o[3]};
        } else tn[v0] = o[0];
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c <= MAXC; c++) {
        unsigned s = cnt[c];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) red[wave][c] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x <= C) {             // columns 0 .. C - 1: kept per class; column C: ignored
        const int src = (int)threadIdx.x < C ? (int)threadIdx.x : MAXC;
        unsigned long long s = 0;
#pragma unroll
        for (int wv = 0; wv < BLK / 64; wv++) s += red[wv][src];
        if (s) atomicAdd(table + (int64_t)n * (C + 1) + threadIdx.x, s);
    }
}
}  // namespace

int pseudo_labels(const uint8_t* labels, const float* conf, int N, int64_t V, int C, const float* thresholds, int64_t ignore_index,
                  int64_t* target, int64_t* table, hipStream_t s) {
    MI3D_CHECK_ARG(C >= 1 && C <= MAXC, "pseudo_labels: %d classes unsupported (max %d)", C, MAXC);
    MI3D_CHECK_ARG(N >= 1 && N <= 65535 && V >= 1, "pseudo_labels: bad batch %d or volume %lld", N, (long long)V);
    Thresholds thr;
    for (int c = 0; c < MAXC; c++) thr.t[c] = c < C ? thresholds[c] : 0.f;
    MI3D_HIP(hipMemsetAsync(table, 0, (size_t)N * (C + 1) * sizeof(int64_t), s));
    const bool v4 = V % 4 == 0 && (uintptr_t)labels % 4 == 0 && (uintptr_t)conf % 16 == 0 && (uintptr_t)target % 16 == 0;
    const int64_t want = (V / (v4 ? 4 : 1) + BLK - 1) / BLK, cap = PSEUDO_BLOCKS / N < 1 ? 1 : PSEUDO_BLOCKS / N;
    dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)N);
    unsigned long long* tb = reinterpret_cast<unsigned long long*>(table);
    if (v4) pseudo_labels_kernel<4><<<grid, BLK, 0, s>>>(labels, conf, V, C, thr, (long long)ignore_index, target, tb);
    else pseudo_labels_kernel<1><<<grid, BLK, 0, s>>>(labels, conf, V, C, thr, (long long)ignore_index, target, tb);
    MI3D_LAUNCH_CHECK();
    return 0;
}
