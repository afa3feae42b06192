// resample.hip — the resampling that puts a decoded scan on the training grid, on the GPU: what the reference's offline
// scripts do with four scipy.ndimage.zoom calls per scan (scripts/resampling/amos_ct_resample.py:56-70,93-97; the same
// calls in chaos_resample.py:53,63,83,87 and resample_totalseg_ras_mri.py:57,65,92,94).
//   zoom3_cubic    zoom(order=3, mode='nearest', prefilter=False): 4x4x4 cubic B-spline taps, edge-clamped, fp64 sums
//   zoom3_nearest  zoom(order=0, mode='nearest'): a per-axis index gather
// Every per-axis quantity (tap indices, already clamped; the four float64 weights; the nearest index) comes from tables the
// host builds in float64 (resample.py axis_table), so the tap choice is scipy's bit for bit; the kernels do no floor, no
// division on coordinates and no polynomial.  Direct form: each thread gathers its taps through L1/L2, no LDS, no atomics.
#include <utility>

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

// Where a stored scan lies in memory, seen in RAS order (orientation.py axis_map): element strides of the RAS axes D, H, W.
// Flips are not here: the host tables already hold n - 1 - i for a flipped axis.
struct SrcStrides {
    int64_t d, h, w;
};

// grid: x over (oh, group of CW outputs along W), y = od.  Sum over (kd, kh) of wd*wh * (sum over kw of x*ww), all fp64.
// STRIDED = false is the contiguous float32 volume (st unused); STRIDED = true reads a stored scan of type S through st with the
// same taps, the same order of sums and the same conversions ((double) of an int16 is what (double)(float) of it is).
template <typename S, bool VEC, bool STRIDED>
__global__ __launch_bounds__(BLK) void zoom3_cubic_kernel(const S* __restrict__ in, float* __restrict__ out, int H, int W,
                                                          int Ho, int Wo, int WQ, const CubicRow* __restrict__ td,
                                                          const CubicRow* __restrict__ th, const CubicRow* __restrict__ tw,
                                                          int ct, float lo, float hi, SrcStrides st) {
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
            const S* row = STRIDED ? in + (rd.idx[kd] * st.d + rh.idx[kh] * st.h) : in + ((int64_t)rd.idx[kd] * H + rh.idx[kh]) * W;
            const int64_t sw = STRIDED ? st.w : 1;
            const double wdh = rd.w[kd] * rh.w[kh];
#pragma unroll
            for (int j = 0; j < CW; j++) {
                double s = (double)row[rw[j].idx[0] * sw] * rw[j].w[0];
                s += (double)row[rw[j].idx[1] * sw] * rw[j].w[1];
                s += (double)row[rw[j].idx[2] * sw] * rw[j].w[2];
                s += (double)row[rw[j].idx[3] * sw] * rw[j].w[3];
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

template <typename S, bool VEC, bool STRIDED>
__global__ __launch_bounds__(BLK) void zoom3_nearest_kernel(const S* __restrict__ in, int64_t* __restrict__ out, int H, int W,
                                                            int Ho, int Wo, int WQ, const int32_t* __restrict__ td,
                                                            const int32_t* __restrict__ th, const int32_t* __restrict__ tw,
                                                            SrcStrides st) {
    const int q = blockIdx.x * BLK + threadIdx.x;
    if (q >= Ho * WQ) return;
    const int oh = q / WQ, ow0 = (q - oh * WQ) * NWV, od = blockIdx.y;
    const S* row = STRIDED ? in + (td[od] * st.d + th[oh] * st.h) : in + ((int64_t)td[od] * H + th[oh]) * W;
    const int64_t sw = STRIDED ? st.w : 1;
    int64_t* o = out + ((int64_t)od * Ho + oh) * Wo + ow0;
    if constexpr (VEC) {
        longlong2 a;
        a.x = (int64_t)row[tw[ow0] * sw];
        a.y = (int64_t)row[tw[ow0 + 1] * sw];
        *reinterpret_cast<longlong2*>(o) = a;
    } else {
#pragma unroll
        for (int j = 0; j < NWV; j++)
            if (ow0 + j < Wo) o[j] = (int64_t)row[tw[ow0 + j] * sw];
    }
}

// ---- stored scans: reorientation to RAS, mask merge ------------------------------------------------------------------------
// RAS index i of a flipped axis is stored index n - 1 - i (torch has no negative strides, so the pointer never moves)
__device__ __forceinline__ int stored_index(int i, int n, int flipped) { return flipped ? n - 1 - i : i; }

// reorient_to_ras (amos_ct_resample.py:29-36) of a dense stored scan into a contiguous RAS volume, converted to T.
// Streaming form: lanes along the destination W, 16 / sizeof(T) outputs per thread.  It is correct for every stride triple and
// is the route when W is also the stored-fastest axis (a copy, reversed when W is flipped) or no axis has stride 1 with a side > 1.
template <typename S, typename T, bool VEC>
__global__ __launch_bounds__(BLK) void reorient3_stream_kernel(const S* __restrict__ in, T* __restrict__ out, int D, int H, int W,
                                                               int WQ, SrcStrides st, int flips) {
    constexpr int NV = 16 / (int)sizeof(T);
    const int q = blockIdx.x * BLK + threadIdx.x;
    if (q >= H * WQ) return;
    const int h = q / WQ, w0 = (q - h * WQ) * NV, d = blockIdx.y;
    const S* row = in + (stored_index(d, D, flips & 1) * st.d + stored_index(h, H, flips & 2) * st.h);
    T* o = out + ((int64_t)d * H + h) * W + w0;
    if constexpr (VEC) {
        typedef __attribute__((ext_vector_type(NV))) T vec_t;
        vec_t a;
#pragma unroll
        for (int j = 0; j < NV; j++) a[j] = (T)row[stored_index(w0 + j, W, flips & 4) * st.w];
        *reinterpret_cast<vec_t*>(o) = a;
    } else {
#pragma unroll
        for (int j = 0; j < NV; j++)
            if (w0 + j < W) o[j] = (T)row[stored_index(w0 + j, W, flips & 4) * st.w];
    }
}

// Tiled form, for a stored-fastest axis F that is the RAS D or H: a TILE x TILE tile of the (F, W) plane goes through LDS, loaded
// with lanes along F (coalesced in the source, ascending or descending) and stored with lanes along W (coalesced in the
// destination).  Pitch TILE + 1: the transposed read tile[tx][c] of 4-byte T hits bank (tx * 33 + c) % 32 = (tx + c) % 32, one lane
// per bank in each 32-lane half; 8-byte T reads dwords tx * 66 + 2c (+1) of 64 banks, again all distinct in a half.
// The two halves of a 64-lane wave read columns c and c + 1, i.e. banks offset by one: if the LDS serves a 4-byte read for all 64
// lanes in one pass that is a 2-way conflict.  Its cost has not been measured; it is small next to the HBM time of the copy.
// grid: x over (tile of F, tile of W), y = g, the third axis.  of / og: destination strides of F and g.
constexpr int TILE = 32, TROWS = BLK / TILE;
template <typename S, typename T>
__global__ __launch_bounds__(BLK) void reorient3_tile_kernel(const S* __restrict__ in, T* __restrict__ out, int nF, int nG, int nW,
                                                             int tilesW, int64_t sF, int64_t sG, int64_t sW, int flipF, int flipG,
                                                             int flipW, int64_t of, int64_t og) {
    __shared__ T tile[TILE][TILE + 1];
    const int tx = threadIdx.x % TILE, ty = threadIdx.x / TILE;
    const int tf = blockIdx.x / tilesW, f0 = tf * TILE, w0 = (blockIdx.x - tf * tilesW) * TILE, g = blockIdx.y;
    const S* src = in + stored_index(g, nG, flipG) * sG;
    if (f0 + tx < nF) {
        const S* col = src + stored_index(f0 + tx, nF, flipF) * sF;
#pragma unroll
        for (int r = ty; r < TILE; r += TROWS)
            if (w0 + r < nW) tile[r][tx] = (T)col[stored_index(w0 + r, nW, flipW) * sW];
    }
    __syncthreads();
    if (w0 + tx < nW) {
        T* dst = out + g * og + w0 + tx;
#pragma unroll
        for (int r = ty; r < TILE; r += TROWS)
            if (f0 + r < nF) dst[(f0 + r) * of] = tile[tx][r];
    }
}

// The TotalSegmentator mask merge (resample_totalseg_ras_mri.py:77-96) as one gather: per output voxel the composed order-0
// source voxel is read from every mask in list order, and the last mask that is > 0 there gives the value.
constexpr int MAX_MASKS = MI3D_MAX_MASKS;
struct MaskArgs {          // by value in the kernel arguments
    const void* mask[MAX_MASKS];
    int64_t value[MAX_MASKS];
    int n;
};
template <typename S, bool VEC>
__global__ __launch_bounds__(BLK) void merge_masks3_kernel(MaskArgs m, int64_t* __restrict__ out, int Ho, int Wo, int WQ,
                                                           const int32_t* __restrict__ td, const int32_t* __restrict__ th,
                                                           const int32_t* __restrict__ tw, SrcStrides st) {
    const int q = blockIdx.x * BLK + threadIdx.x;
    if (q >= Ho * WQ) return;
    const int oh = q / WQ, ow0 = (q - oh * WQ) * NWV, od = blockIdx.y;
    const int64_t row = td[od] * st.d + th[oh] * st.h;
    int64_t v[NWV];
#pragma unroll
    for (int j = 0; j < NWV; j++) {
        v[j] = 0;
        const int64_t off = row + tw[min(ow0 + j, Wo - 1)] * st.w;      // a tail lane rereads the last column, never stores it
#pragma unroll
        for (int k = 0; k < MAX_MASKS; k++)
            if (k < m.n && static_cast<const S*>(m.mask[k])[off] > (S)0) v[j] = m.value[k];
    }
    int64_t* o = out + ((int64_t)od * Ho + oh) * Wo + ow0;
    if constexpr (VEC) {
        longlong2 a;
        a.x = v[0];
        a.y = v[1];
        *reinterpret_cast<longlong2*>(o) = a;
    } else {
#pragma unroll
        for (int j = 0; j < NWV; j++)
            if (ow0 + j < Wo) o[j] = v[j];
    }
}

// Labels from the training grid back onto a scan as stored: the order-0 gather out[s][m][f] = grid[tS[s]][tM[m]][tF[f]] with the
// DESTINATION strided.  The launcher sorts the stored tensor's three axes by stride: F is fastest in memory, then M, then S, so
// the kernel walks the output in memory order whatever the orientation; each axis brings its table (one grid index per
// destination index, already reversed for a flipped axis) and the grid's stride along it (gS, gM, gF: a permutation of
// Hg * Wg, Wg, 1).  grid: x over (m, piece of the row along F), y = s.  The two slow-axis indices are read once per thread, the
// fastest-axis index per element.  Pieces are cut where the row's bytes are 16-byte aligned: piece 0 is the (possibly empty)
// head up to the first aligned byte, every later piece 16 bytes in one store, the last one the scalar tail; a fastest axis
// that is not dense (oF != 1: no side > 1 has stride 1) is stored a byte at a time.
// For F = the grid's W the 16 reads of a thread are neighbouring bytes; for F = D or H they are 16 different lines, shared with
// the neighbouring rows.
constexpr int RW = 16;
__global__ __launch_bounds__(BLK) void restore_labels3_kernel(const uint8_t* __restrict__ grid, uint8_t* __restrict__ out, int nM,
                                                              int nF, int FQ, const int32_t* __restrict__ tS,
                                                              const int32_t* __restrict__ tM, const int32_t* __restrict__ tF,
                                                              int64_t gS, int64_t gM, int64_t gF, int64_t oS, int64_t oM, int64_t oF) {
    const int q = blockIdx.x * BLK + threadIdx.x;
    if (q >= nM * FQ) return;
    const int m = q / FQ, piece = q - m * FQ, s = blockIdx.y;
    uint8_t* o = out + (s * oS + m * oM);
    const int head = oF == 1 ? (int)((RW - (reinterpret_cast<uintptr_t>(o) & (RW - 1))) & (RW - 1)) : 0;
    const int f0 = piece == 0 ? 0 : head + (piece - 1) * RW;
    const int f1 = min(piece == 0 ? head : f0 + RW, nF);
    if (f0 >= f1) return;
    const uint8_t* row = grid + (tS[s] * gS + tM[m] * gM);
    if (f1 - f0 == RW && oF == 1) {
        uint32_t a[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            a[j] = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) a[j] |= (uint32_t)row[tF[f0 + 4 * j + b] * gF] << (8 * b);
        }
        *reinterpret_cast<uint4*>(o + f0) = uint4{a[0], a[1], a[2], a[3]};
    } else {
        for (int f = f0; f < f1; f++) o[f * oF] = row[tF[f] * gF];
    }
}

constexpr int MAX_SIDE = 65535;      // od rides in gridDim.y; in-plane indices stay far inside int32
inline bool dims_ok(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1 && D <= MAX_SIDE && H <= MAX_SIDE && W <= MAX_SIDE; }

// a stored scan's strides: positive (any value where the side is 1), and the last element's offset inside int64 with room to spare
// (that the last element's offset lies inside the caller's buffer is the caller's to guarantee: include/mi3d.h; resample.py
// passes dense tensors only)
inline bool strides_ok(int64_t sd, int64_t sh, int64_t sw) {
    const int64_t lim = (int64_t)1 << 44;      // 65535^3 < 2^48 elements; a dense tensor's largest stride is < 2^32
    return sd >= 1 && sh >= 1 && sw >= 1 && sd < lim && sh < lim && sw < lim;
}

template <typename S, typename T>
int reorient3_launch(const S* in, T* out, int D, int H, int W, int64_t sd, int64_t sh, int64_t sw, int flips, hipStream_t s) {
    constexpr int NV = 16 / (int)sizeof(T);
    // the stored-fastest axis, where it is not W: D or H with stride 1 and more than one element
    const int fast = (sw == 1 || W == 1) ? 2 : (sh == 1 && H > 1) ? 1 : (sd == 1 && D > 1) ? 0 : 2;
    if (fast == 2) {
        const int WQ = (W + NV - 1) / NV;
        MI3D_CHECK_ARG((int64_t)H * WQ < (int64_t)1 << 31, "mi3d_reorient3: plane too large");
        dim3 grid((unsigned)(((int64_t)H * WQ + BLK - 1) / BLK), (unsigned)D);
        const SrcStrides st{sd, sh, sw};
        if (W % NV == 0 && ((uintptr_t)out & 15) == 0)
            reorient3_stream_kernel<S, T, true><<<grid, BLK, 0, s>>>(in, out, D, H, W, WQ, st, flips);
        else
            reorient3_stream_kernel<S, T, false><<<grid, BLK, 0, s>>>(in, out, D, H, W, WQ, st, flips);
    } else {
        const int nF = fast == 1 ? H : D, nG = fast == 1 ? D : H;
        const int tilesW = (W + TILE - 1) / TILE, tilesF = (nF + TILE - 1) / TILE;
        dim3 grid((unsigned)(tilesF * tilesW), (unsigned)nG);
        if (fast == 1)
            reorient3_tile_kernel<S, T><<<grid, BLK, 0, s>>>(in, out, nF, nG, W, tilesW, sh, sd, sw, flips & 2, flips & 1, flips & 4,
                                                             (int64_t)W, (int64_t)H * W);
        else
            reorient3_tile_kernel<S, T><<<grid, BLK, 0, s>>>(in, out, nF, nG, W, tilesW, sd, sh, sw, flips & 1, flips & 2, flips & 4,
                                                             (int64_t)H * W, (int64_t)W);
    }
    MI3D_LAUNCH_CHECK();
    return 0;
}
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
        zoom3_cubic_kernel<float, true, false><<<grid, BLK, 0, s>>>(in, out, H, W, Ho, Wo, WQ, td, th, tw, ct_window, window_min, window_max, SrcStrides{});
    else
        zoom3_cubic_kernel<float, false, false><<<grid, BLK, 0, s>>>(in, out, H, W, Ho, Wo, WQ, td, th, tw, ct_window, window_min, window_max, SrcStrides{});
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
        zoom3_nearest_kernel<int64_t, true, false><<<grid, BLK, 0, s>>>(in, out, H, W, Ho, Wo, WQ, index_d, index_h, index_w, SrcStrides{});
    else
        zoom3_nearest_kernel<int64_t, false, false><<<grid, BLK, 0, s>>>(in, out, H, W, Ho, Wo, WQ, index_d, index_h, index_w, SrcStrides{});
    MI3D_LAUNCH_CHECK();
    return 0;
}

int mi3d_reorient3(const void* in, int src_dtype, void* out, int out_i64, int D, int H, int W, int64_t stride_d, int64_t stride_h,
                   int64_t stride_w, int flip_mask, void* stream) {
    MI3D_CHECK_ARG(in && out && in != out, "mi3d_reorient3: null or aliased pointers");
    MI3D_CHECK_ARG(dims_ok(D, H, W), "mi3d_reorient3: sides must be in [1, %d]", MAX_SIDE);
    MI3D_CHECK_ARG(strides_ok(stride_d, stride_h, stride_w), "mi3d_reorient3: strides must be positive element counts");
    MI3D_CHECK_ARG(flip_mask >= 0 && flip_mask <= 7, "mi3d_reorient3: flip_mask %d outside 0..7", flip_mask);
    hipStream_t s = (hipStream_t)stream;
#define MI3D_REORIENT(S, T) return reorient3_launch<S, T>((const S*)in, (T*)out, D, H, W, stride_d, stride_h, stride_w, flip_mask, s)
    if (!out_i64) {
        if (src_dtype == MI3D_SRC_U8) MI3D_REORIENT(uint8_t, float);
        if (src_dtype == MI3D_SRC_I16) MI3D_REORIENT(int16_t, float);
        if (src_dtype == MI3D_SRC_F32) MI3D_REORIENT(float, float);
        MI3D_CHECK_ARG(false, "mi3d_reorient3: a float32 volume is made from uint8, int16 or float32, not dtype code %d", src_dtype);
    }
    if (src_dtype == MI3D_SRC_U8) MI3D_REORIENT(uint8_t, int64_t);
    if (src_dtype == MI3D_SRC_I16) MI3D_REORIENT(int16_t, int64_t);
    if (src_dtype == MI3D_SRC_I64) MI3D_REORIENT(int64_t, int64_t);
#undef MI3D_REORIENT
    MI3D_CHECK_ARG(false, "mi3d_reorient3: an int64 volume is made from uint8, int16 or int64, not dtype code %d", src_dtype);
}

int mi3d_zoom3_cubic_src(const void* in, int src_dtype, int64_t stride_d, int64_t stride_h, int64_t stride_w, float* out, int D,
                         int H, int W, int Do, int Ho, int Wo, const void* table_d, int rows_d, const void* table_h, int rows_h,
                         const void* table_w, int rows_w, int ct_window, float window_min, float window_max, void* stream) {
    MI3D_CHECK_ARG(in && out && in != (const void*)out && table_d && table_h && table_w, "mi3d_zoom3_cubic_src: null or aliased pointers");
    MI3D_CHECK_ARG(dims_ok(D, H, W) && dims_ok(Do, Ho, Wo), "mi3d_zoom3_cubic_src: sides must be in [1, %d]", MAX_SIDE);
    MI3D_CHECK_ARG(strides_ok(stride_d, stride_h, stride_w), "mi3d_zoom3_cubic_src: strides must be positive element counts");
    MI3D_CHECK_ARG(rows_d == Do && rows_h == Ho && rows_w == Wo,
                   "mi3d_zoom3_cubic_src: tables have (%d, %d, %d) rows, the output is (%d, %d, %d)", rows_d, rows_h, rows_w, Do, Ho, Wo);
    MI3D_CHECK_ARG((((uintptr_t)table_d | (uintptr_t)table_h | (uintptr_t)table_w) & 15) == 0,
                   "mi3d_zoom3_cubic_src: tables must be 16-byte aligned");
    MI3D_CHECK_ARG(!ct_window || window_max > window_min, "mi3d_zoom3_cubic_src: empty CT window");
    MI3D_CHECK_ARG(src_dtype == MI3D_SRC_U8 || src_dtype == MI3D_SRC_I16 || src_dtype == MI3D_SRC_F32,
                   "mi3d_zoom3_cubic_src: the source is uint8, int16 or float32, not dtype code %d", src_dtype);
    const int WQ = (Wo + CW - 1) / CW;
    MI3D_CHECK_ARG((int64_t)Ho * WQ < (int64_t)1 << 31, "mi3d_zoom3_cubic_src: output plane too large");
    dim3 grid((unsigned)(((int64_t)Ho * WQ + BLK - 1) / BLK), (unsigned)Do);
    const CubicRow *td = (const CubicRow*)table_d, *th = (const CubicRow*)table_h, *tw = (const CubicRow*)table_w;
    const SrcStrides st{stride_d, stride_h, stride_w};
    hipStream_t s = (hipStream_t)stream;
    const bool vec = Wo % CW == 0 && ((uintptr_t)out & 15) == 0;
#define MI3D_CUBIC_SRC(S)                                                                                                       \
    do {                                                                                                                        \
        if (vec)                                                                                                                \
            zoom3_cubic_kernel<S, true, true><<<grid, BLK, 0, s>>>((const S*)in, out, H, W, Ho, Wo, WQ, td, th, tw, ct_window,   \
                                                                   window_min, window_max, st);                                 \
        else                                                                                                                    \
            zoom3_cubic_kernel<S, false, true><<<grid, BLK, 0, s>>>((const S*)in, out, H, W, Ho, Wo, WQ, td, th, tw, ct_window,  \
                                                                    window_min, window_max, st);                                \
    } while (0)
    if (src_dtype == MI3D_SRC_U8) MI3D_CUBIC_SRC(uint8_t);
    else if (src_dtype == MI3D_SRC_I16) MI3D_CUBIC_SRC(int16_t);
    else MI3D_CUBIC_SRC(float);
#undef MI3D_CUBIC_SRC
    MI3D_LAUNCH_CHECK();
    return 0;
}

int mi3d_zoom3_nearest_src(const void* in, int src_dtype, int64_t stride_d, int64_t stride_h, int64_t stride_w, int64_t* out, int D,
                           int H, int W, int Do, int Ho, int Wo, const int32_t* index_d, int rows_d, const int32_t* index_h,
                           int rows_h, const int32_t* index_w, int rows_w, void* stream) {
    MI3D_CHECK_ARG(in && out && in != (const void*)out && index_d && index_h && index_w, "mi3d_zoom3_nearest_src: null or aliased pointers");
    MI3D_CHECK_ARG(dims_ok(D, H, W) && dims_ok(Do, Ho, Wo), "mi3d_zoom3_nearest_src: sides must be in [1, %d]", MAX_SIDE);
    MI3D_CHECK_ARG(strides_ok(stride_d, stride_h, stride_w), "mi3d_zoom3_nearest_src: strides must be positive element counts");
    MI3D_CHECK_ARG(rows_d == Do && rows_h == Ho && rows_w == Wo,
                   "mi3d_zoom3_nearest_src: tables have (%d, %d, %d) rows, the output is (%d, %d, %d)", rows_d, rows_h, rows_w, Do, Ho, Wo);
    MI3D_CHECK_ARG(src_dtype == MI3D_SRC_U8 || src_dtype == MI3D_SRC_I16 || src_dtype == MI3D_SRC_I64,
                   "mi3d_zoom3_nearest_src: the source is uint8, int16 or int64, not dtype code %d", src_dtype);
    const int WQ = (Wo + NWV - 1) / NWV;
    MI3D_CHECK_ARG((int64_t)Ho * WQ < (int64_t)1 << 31, "mi3d_zoom3_nearest_src: output plane too large");
    dim3 grid((unsigned)(((int64_t)Ho * WQ + BLK - 1) / BLK), (unsigned)Do);
    const SrcStrides st{stride_d, stride_h, stride_w};
    hipStream_t s = (hipStream_t)stream;
    const bool vec = Wo % NWV == 0 && ((uintptr_t)out & 15) == 0;
#define MI3D_NEAREST_SRC(S)                                                                                                      \
    do {                                                                                                                         \
        if (vec)                                                                                                                 \
            zoom3_nearest_kernel<S, true, true><<<grid, BLK, 0, s>>>((const S*)in, out, H, W, Ho, Wo, WQ, index_d, index_h, index_w, st);  \
        else                                                                                                                     \
            zoom3_nearest_kernel<S, false, true><<<grid, BLK, 0, s>>>((const S*)in, out, H, W, Ho, Wo, WQ, index_d, index_h, index_w, st); \
    } while (0)
    if (src_dtype == MI3D_SRC_U8) MI3D_NEAREST_SRC(uint8_t);
    else if (src_dtype == MI3D_SRC_I16) MI3D_NEAREST_SRC(int16_t);
    else MI3D_NEAREST_SRC(int64_t);
#undef MI3D_NEAREST_SRC
    MI3D_LAUNCH_CHECK();
    return 0;
}

int mi3d_merge_masks3(const mi3d_mask_list* masks, int src_dtype, int64_t stride_d, int64_t stride_h, int64_t stride_w, int64_t* out,
                      int D, int H, int W, int Do, int Ho, int Wo, const int32_t* index_d, int rows_d, const int32_t* index_h,
                      int rows_h, const int32_t* index_w, int rows_w, void* stream) {
    MI3D_CHECK_ARG(masks && out && index_d && index_h && index_w, "mi3d_merge_masks3: null pointers");
    MI3D_CHECK_ARG(masks->n >= 0 && masks->n <= MAX_MASKS, "mi3d_merge_masks3: %d masks, at most %d fit one launch", masks->n, MAX_MASKS);
    MI3D_CHECK_ARG(dims_ok(D, H, W) && dims_ok(Do, Ho, Wo), "mi3d_merge_masks3: sides must be in [1, %d]", MAX_SIDE);
    MI3D_CHECK_ARG(strides_ok(stride_d, stride_h, stride_w), "mi3d_merge_masks3: strides must be positive element counts");
    MI3D_CHECK_ARG(rows_d == Do && rows_h == Ho && rows_w == Wo,
                   "mi3d_merge_masks3: tables have (%d, %d, %d) rows, the output is (%d, %d, %d)", rows_d, rows_h, rows_w, Do, Ho, Wo);
    MI3D_CHECK_ARG(src_dtype == MI3D_SRC_U8 || src_dtype == MI3D_SRC_F32,
                   "mi3d_merge_masks3: masks are uint8 or float32, not dtype code %d", src_dtype);
    MaskArgs m{};
    m.n = masks->n;
    for (int k = 0; k < masks->n; k++) {
        MI3D_CHECK_ARG(masks->mask[k] && masks->mask[k] != (const void*)out, "mi3d_merge_masks3: mask %d is null or is the output", k);
        m.mask[k] = masks->mask[k];
        m.value[k] = masks->value[k];
    }
    const int WQ = (Wo + NWV - 1) / NWV;
    MI3D_CHECK_ARG((int64_t)Ho * WQ < (int64_t)1 << 31, "mi3d_merge_masks3: output plane too large");
    dim3 grid((unsigned)(((int64_t)Ho * WQ + BLK - 1) / BLK), (unsigned)Do);
    const SrcStrides st{stride_d, stride_h, stride_w};
    hipStream_t s = (hipStream_t)stream;
    const bool vec = Wo % NWV == 0 && ((uintptr_t)out & 15) == 0;
    if (src_dtype == MI3D_SRC_U8) {
        if (vec) merge_masks3_kernel<uint8_t, true><<<grid, BLK, 0, s>>>(m, out, Ho, Wo, WQ, index_d, index_h, index_w, st);
        else merge_masks3_kernel<uint8_t, false><<<grid, BLK, 0, s>>>(m, out, Ho, Wo, WQ, index_d, index_h, index_w, st);
    } else {
        if (vec) merge_masks3_kernel<float, true><<<grid, BLK, 0, s>>>(m, out, Ho, Wo, WQ, index_d, index_h, index_w, st);
        else merge_masks3_kernel<float, false><<<grid, BLK, 0, s>>>(m, out, Ho, Wo, WQ, index_d, index_h, index_w, st);
    }
    MI3D_LAUNCH_CHECK();
    return 0;
}

int mi3d_restore_labels3(const uint8_t* grid, int Dg, int Hg, int Wg, uint8_t* out, int D, int H, int W, int64_t stride_d,
                         int64_t stride_h, int64_t stride_w, const int32_t* index_d, const int32_t* index_h, const int32_t* index_w,
                         void* stream) {
    MI3D_CHECK_ARG(grid && out && grid != out && index_d && index_h && index_w, "mi3d_restore_labels3: null or aliased pointers");
    MI3D_CHECK_ARG(dims_ok(Dg, Hg, Wg) && dims_ok(D, H, W), "mi3d_restore_labels3: sides must be in [1, %d]", MAX_SIDE);
    MI3D_CHECK_ARG(strides_ok(stride_d, stride_h, stride_w), "mi3d_restore_labels3: strides must be positive element counts");
    // the destination's axes by increasing stride, an axis of one element last among equals: a[0] = F, a[1] = M, a[2] = S
    struct Axis { int n; int64_t os, gs; const int32_t* t; };
    Axis a[3] = {{D, stride_d, (int64_t)Hg * Wg, index_d}, {H, stride_h, (int64_t)Wg, index_h}, {W, stride_w, 1, index_w}};
    auto before = [](const Axis& x, const Axis& y) { return (x.n > 1) != (y.n > 1) ? x.n > 1 : x.os < y.os; };
    if (before(a[1], a[0])) std::swap(a[0], a[1]);
    if (before(a[2], a[1])) std::swap(a[1], a[2]);
    if (before(a[1], a[0])) std::swap(a[0], a[1]);
    const Axis &F = a[0], &M = a[1], &S = a[2];
    const int FQ = 1 + (F.n + RW - 1) / RW;
    MI3D_CHECK_ARG((int64_t)M.n * FQ < (int64_t)1 << 31, "mi3d_restore_labels3: output plane too large");
    dim3 grd((unsigned)(((int64_t)M.n * FQ + BLK - 1) / BLK), (unsigned)S.n);
    restore_labels3_kernel<<<grd, BLK, 0, (hipStream_t)stream>>>(grid, out, M.n, F.n, FQ, S.t, M.t, F.t, S.gs, M.gs, F.gs, S.os, M.os,
                                                                 F.n > 1 ? F.os : 1);
    MI3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
