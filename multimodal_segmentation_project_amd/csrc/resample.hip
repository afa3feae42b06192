// resample.hip — the resampling that puts a decoded scan on the training grid, on the GPU: what the reference's offline
// scripts do with four scipy.ndimage.zoom calls per scan (scripts/resampling/amos_ct_resample.py:56-70,93-97; the same
// calls in chaos_resample.py:53,63,83,87 and resample_totalseg_ras_mri.py:57,65,92,94).
//   zoom3_cubic    zoom(order=3, mode='nearest', prefilter=False): 4x4x4 cubic B-spline taps, edge-clamped, fp64 sums
//   zoom3_nearest  zoom(order=0, mode='nearest'): a per-axis index gather
// Every per-axis quantity (tap indices, already clamped; the four float64 weights; the nearest index) comes from tables the
// host builds in float64 (resample.py axis_table), so the tap choice is scipy's bit for bit; the kernels do no floor, no
// division on coordinates and no polynomial.  Direct form: each thread gathers its taps through L1/L2, no LDS, no atomics.
#include "ops.h"
#include "../../include/mi3d.h"

namespace {
constexpr int BLK = 256;
constexpr int CW = 4;      // cubic: consecutive W outputs per thread (one 16-byte store)
constexpr int NWV = 2;     // nearest: consecutive int64 W outputs per thread (one 16-byte store)

struct CubicRow {          // one output index of one axis; layout shared with resample.py (_ROW)
    int32_t idx[4];        // input indices of the four taps, clamped to [0, n_in - 1]
    double w[4];           // cubic B-spline weights, >= 0, sum 1
};
static_assert(sizeof(CubicRow) == 48, "table row layout");

// grid: x over (oh, group of CW outputs along W), y = od.  Sum over (kd, kh) of wd*wh * (sum over kw of x*ww), all fp64.
template <bool VEC>
__global__ __launch_bounds__(BLK) void zoom3_cubic_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                          int Ho, int Wo, int WQ, const CubicRow* __restrict__ td,
                                                          const CubicRow* __restrict__ th, const CubicRow* __restrict__ tw,
                                                          int ct, float lo, float hi) {
    const int q = blockIdx.x * BLK + threadIdx.x;
    if (q >= Ho * WQ) return;
    const int oh = q / WQ, ow0 = (q - oh * WQ) * CW, od = blockIdx.y;
    const CubicRow rd = td[od], rh = th[oh];
    CubicRow rw[CW];
#pragma unroll
    for (int j = 0; j < CW; j++) rw[j] = tw[min(ow0 + j, Wo - 1)];       // tail lanes recompute the last column, never store it
    double acc[CW];
#pragma unroll
    for (int j = 0; j < CW; j++) acc[j] = 0.0;
#pragma unroll
    for (int kd = 0; kd < 4; kd++) {
#pragma unroll
        for (int kh = 0; kh < 4; kh++) {
            const float* row = in + ((int64_t)rd.idx[kd] * H + rh.idx[kh]) * W;
            const double wdh = rd.w[kd] * rh.w[kh];
#pragma unroll
            for (int j = 0; j < CW; j++) {
                double s = (double)row[rw[j].idx[0]] * rw[j].w[0];
                s += (double)row[rw[j].idx[1]] * rw[j].w[1];
                s += (double)row[rw[j].idx[2]] * rw[j].w[2];
                s += (double)row[rw[j].idx[3]] * rw[j].w[3];
                acc[j] += wdh * s;
            }
        }
    }
    float v[CW];
#pragma unroll
    for (int j = 0; j < CW; j++) {
        v[j] = (float)acc[j];                                             // the one rounding to fp32
        if (ct) v[j] = ct_window_f32(v[j], lo, hi);
    }
    float* o = out + ((int64_t)od * Ho + oh) * Wo + ow0;
    if constexpr (VEC) {
        f32x4 a = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(o) = a;
    } else {
#pragma unroll
        for (int j = 0; j < CW; j++)
            if (ow0 + j < Wo) o[j] = v[j];
    }
}

template <bool VEC>
__global__ __launch_bounds__(BLK) void zoom3_nearest_kernel(const int64_t* __restrict__ in, int64_t* __restrict__ out, int H, int W,
                                                            int Ho, int Wo, int WQ, const int32_t* __restrict__ td,
                                                            const int32_t* __restrict__ th, const int32_t* __restrict__ tw) {
    const int q = blockIdx.x * BLK + threadIdx.x;
    if (q >= Ho * WQ) return;
    const int oh = q / WQ, ow0 = (q - oh * WQ) * NWV, od = blockIdx.y;
    const int64_t* row = in + ((int64_t)td[od] * H + th[oh]) * W;
    int64_t* o = out + ((int64_t)od * Ho + oh) * Wo + ow0;
    if constexpr (VEC) {
        longlong2 a;
        a.x = row[tw[ow0]];
        a.y = row[tw[ow0 + 1]];
        *reinterpret_cast<longlong2*>(o) = a;
    } else {
#pragma unroll
        for (int j = 0; j < NWV; j++)
            if (ow0 + j < Wo) o[j] = row[tw[ow0 + j]];
    }
}

constexpr int MAX_SIDE = 65535;      // od rides in gridDim.y; in-plane indices stay far inside int32
inline bool dims_ok(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1 && D <= MAX_SIDE && H <= MAX_SIDE && W <= MAX_SIDE; }
}  // namespace

extern "C" {

size_t mi3d_zoom3_workspace_bytes(int D, int H, int W) {
    if (!dims_ok(D, H, W)) {
        mi3d_set_error("mi3d_zoom3_workspace_bytes: sides must be in [1, %d]", MAX_SIDE);
        return 0;
    }
    return (((size_t)D * H * W * sizeof(float)) + 255) & ~(size_t)255;
}

int mi3d_zoom3_cubic(const float* in, float* out, int D, int H, int W, int Do, int Ho, int Wo, const void* table_d, int rows_d,
                     const void* table_h, int rows_h, const void* table_w, int rows_w, int ct_window, float window_min,
                     float window_max, void* stream) {
    MI3D_CHECK_ARG(in && out && in != out && table_d && table_h && table_w, "mi3d_zoom3_cubic: null or aliased pointers");
    MI3D_CHECK_ARG(dims_ok(D, H, W) && dims_ok(Do, Ho, Wo), "mi3d_zoom3_cubic: sides must be in [1, %d]", MAX_SIDE);
    MI3D_CHECK_ARG(rows_d == Do && rows_h == Ho && rows_w == Wo,
                   "mi3d_zoom3_cubic: tables have (%d, %d, %d) rows, the output is (%d, %d, %d)", rows_d, rows_h, rows_w, Do, Ho, Wo);
    MI3D_CHECK_ARG((((uintptr_t)table_d | (uintptr_t)table_h | (uintptr_t)table_w) & 15) == 0,
                   "mi3d_zoom3_cubic: tables must be 16-byte aligned");
    MI3D_CHECK_ARG(!ct_window || window_max > window_min, "mi3d_zoom3_cubic: empty CT window");
    const int WQ = (Wo + CW - 1) / CW;
    MI3D_CHECK_ARG((int64_t)Ho * WQ < (int64_t)1 << 31, "mi3d_zoom3_cubic: output plane too large");
    dim3 grid((unsigned)(((int64_t)Ho * WQ + BLK - 1) / BLK), (unsigned)Do);
    const CubicRow *td = (const CubicRow*)table_d, *th = (const CubicRow*)table_h, *tw = (const CubicRow*)table_w;
    hipStream_t s = (hipStream_t)stream;
    if (Wo % CW == 0 && ((uintptr_t)out & 15) == 0)
        zoom3_cubic_kernel<true><<<grid, BLK, 0, s>>>(in, out, H, W, Ho, Wo, WQ, td, th, tw, ct_window, window_min, window_max);
    else
        zoom3_cubic_kernel<false><<<grid, BLK, 0, s>>>(in, out, H, W, Ho, Wo, WQ, td, th, tw, ct_window, window_min, window_max);
    MI3D_LAUNCH_CHECK();
    return 0;
}

int mi3d_zoom3_nearest_i64(const int64_t* in, int64_t* out, int D, int H, int W, int Do, int Ho, int Wo, const int32_t* index_d,
                           int rows_d, const int32_t* index_h, int rows_h, const int32_t* index_w, int rows_w, void* stream) {
    MI3D_CHECK_ARG(in && out && in != out && index_d && index_h && index_w, "mi3d_zoom3_nearest_i64: null or aliased pointers");
    MI3D_CHECK_ARG(dims_ok(D, H, W) && dims_ok(Do, Ho, Wo), "mi3d_zoom3_nearest_i64: sides must be in [1, %d]", MAX_SIDE);
    MI3D_CHECK_ARG(rows_d == Do && rows_h == Ho && rows_w == Wo,
                   "mi3d_zoom3_nearest_i64: tables have (%d, %d, %d) rows, the output is (%d, %d, %d)", rows_d, rows_h, rows_w, Do, Ho, Wo);
    const int WQ = (Wo + NWV - 1) / NWV;
    MI3D_CHECK_ARG((int64_t)Ho * WQ < (int64_t)1 << 31, "mi3d_zoom3_nearest_i64: output plane too large");
    dim3 grid((unsigned)(((int64_t)Ho * WQ + BLK - 1) / BLK), (unsigned)Do);
    hipStream_t s = (hipStream_t)stream;
    if (Wo % NWV == 0 && ((uintptr_t)out & 15) == 0)
        zoom3_nearest_kernel<true><<<grid, BLK, 0, s>>>(in, out, H, W, Ho, Wo, WQ, index_d, index_h, index_w);
    else
        zoom3_nearest_kernel<false><<<grid, BLK, 0, s>>>(in, out, H, W, Ho, Wo, WQ, index_d, index_h, index_w);
    MI3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
