// resample.hip — the resampling that puts a decoded scan on the training grid, on the GPU: what the reference's offline
// scripts do with four scipy.ndimage.zoom calls per scan (scripts/resampling/amos_ct_resample.py:56-70,93-97; the same
// calls in chaos_resample.py:53,63,83,87 and resample_totalseg_ras_mri.py:57,65,92,94).
//   zoom3_cubic    zoom(order=3, mode='nearest', prefilter=False): 4x4x4 cubic B-spline taps, edge-clamped, fp64 sums
//   zoom3_nearest  zoom(order=0, mode='nearest'): a per-axis index gather
// Every per-axis quantity (tap indices, already clamped; the four float64 weights; the nearest index) comes from tables the
// host builds in float64 (resample.py axis_table), so the tap choice is scipy's bit for bit; the kernels do no floor, no
// division on coordinates and no polynomial.  Direct form: each thread gathers its taps through L1/L2, no LDS, no atomics.
//
// The kernels that write contiguous rows (cubic, nearest, mask merge, streamed reorient) share one walk:
//   row_slot     grid x over (output row oh, group of NV consecutive W outputs from ow0), y = od; NV * sizeof(T) = 16
//   tail_col     a lane past the row's end reads what the last column reads (index min(ow0 + j, Wo - 1)) and is never stored
//   store_group  VEC: one 16-byte store (the launcher saw Wo % NV == 0 and an aligned output); else scalar stores of ow0 + j < Wo
//   src_row      STRIDED = false: a contiguous volume (st unused); true: a stored scan read through its RAS element strides
// Both STRIDED forms gather the same taps and sum them in the same order, so they give the same bits.
#include <type_traits>
#include <utility>

#include "volume.h"

namespace {
constexpr int BLK = 256;
constexpr int CW = 4;      // cubic: float outputs per thread
constexpr int NWV = 2;     // nearest, merge: int64 outputs per thread

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

template <int NV>
__device__ __forceinline__ bool row_slot(int Ho, int WQ, int& oh, int& ow0, int& od) {
    const int q = blockIdx.x * BLK + threadIdx.x;
    if (q >= Ho * WQ) return false;
    oh = q / WQ, ow0 = (q - oh * WQ) * NV, od = blockIdx.y;
    return true;
}

template <bool VEC>      // VEC: the launcher saw Wo % NV == 0, no lane is past the end
__device__ __forceinline__ int tail_col(int ow, int Wo) { return VEC ? ow : min(ow, Wo - 1); }

template <typename T, int NV, bool VEC>
__device__ __forceinline__ void store_group(T* o, const T (&v)[NV], int ow0, int Wo) {
    static_assert(NV * sizeof(T) == 16, "one 16-byte store");
    if constexpr (VEC) {
        typedef __attribute__((ext_vector_type(NV))) T vec_t;
        vec_t a;
#pragma unroll
        for (int j = 0; j < NV; j++) a[j] = v[j];
        *reinterpret_cast<vec_t*>(o) = a;
    } else {
#pragma unroll
        for (int j = 0; j < NV; j++)
            if (ow0 + j < Wo) o[j] = v[j];
    }
}

template <bool STRIDED, typename S>
__device__ __forceinline__ const S* src_row(const S* in, int id, int ih, int H, int W, SrcStrides st) {
    return STRIDED ? in + (id * st.d + ih * st.h) : in + ((int64_t)id * H + ih) * W;
}
template <bool STRIDED>
__device__ __forceinline__ int64_t src_sw(SrcStrides st) { return STRIDED ? st.w : 1; }

// Sum over (kd, kh) of wd*wh * (sum over kw of x*ww), all fp64.  A stored scan of type S converts as the float32 copy of it would:
// (double) of an int16 is what (double)(float) of it is.
template <typename S, bool VEC, bool STRIDED>
__global__ __launch_bounds__(BLK) void zoom3_cubic_kernel(const S* __restrict__ in, float* __restrict__ out, int H, int W,
                                                          int Ho, int Wo, int WQ, const CubicRow* __restrict__ td,
                                                          const CubicRow* __restrict__ th, const CubicRow* __restrict__ tw,
                                                          int ct, float lo, float hi, SrcStrides st) {
    int oh, ow0, od;
    if (!row_slot<CW>(Ho, WQ, oh, ow0, od)) return;
    const CubicRow rd = td[od], rh = th[oh];
    CubicRow rw[CW];
#pragma unroll
    for (int j = 0; j < CW; j++) rw[j] = tw[tail_col<false>(ow0 + j, Wo)];      // clamped in the vector form too: without, <uint8, VEC> takes 15 more AGPRs
    double acc[CW];
#pragma unroll
    for (int j = 0; j < CW; j++) acc[j] = 0.0;
#pragma unroll
    for (int kd = 0; kd < 4; kd++) {
#pragma unroll
        for (int kh = 0; kh < 4; kh++) {
            const S* row = src_row<STRIDED>(in, rd.idx[kd], rh.idx[kh], H, W, st);
            const int64_t sw = src_sw<STRIDED>(st);
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
    store_group<float, CW, VEC>(out + ((int64_t)od * Ho + oh) * Wo + ow0, v, ow0, Wo);
}

template <typename S, bool VEC, bool STRIDED>
__global__ __launch_bounds__(BLK) void zoom3_nearest_kernel(const S* __restrict__ in, int64_t* __restrict__ out, int H, int W,
                                                            int Ho, int Wo, int WQ, const int32_t* __restrict__ td,
                                                            const int32_t* __restrict__ th, const int32_t* __restrict__ tw,
                                                            SrcStrides st) {
    int oh, ow0, od;
    if (!row_slot<NWV>(Ho, WQ, oh, ow0, od)) return;
    const S* row = src_row<STRIDED>(in, td[od], th[oh], H, W, st);
    const int64_t sw = src_sw<STRIDED>(st);
    int64_t v[NWV];
#pragma unroll
    for (int j = 0; j < NWV; j++) v[j] = (int64_t)row[tw[tail_col<VEC>(ow0 + j, Wo)] * sw];
    store_group<int64_t, NWV, VEC>(out + ((int64_t)od * Ho + oh) * Wo + ow0, v, ow0, Wo);
}

// ---- stored scans: reorientation to RAS, mask merge ------------------------------------------------------------------------
// RAS index i of a flipped axis is stored index n - 1 - i (torch has no negative strides, so the pointer never moves)
__device__ __forceinline__ int stored_index(int i, int n, int flipped) { return flipped ? n - 1 - i : i; }

// reorient_to_ras (amos_ct_resample.py:29-36) of a dense stored scan into a contiguous RAS volume, converted to T.
// Streaming form: lanes along the destination W.  It is correct for every stride triple and is the route when W is also the
// stored-fastest axis (a copy, reversed when W is flipped) or no axis has stride 1 with a side > 1.
template <typename S, typename T, bool VEC>
__global__ __launch_bounds__(BLK) void reorient3_stream_kernel(const S* __restrict__ in, T* __restrict__ out, int D, int H, int W,
                                                               int WQ, SrcStrides st, int flips) {
    constexpr int NV = 16 / (int)sizeof(T);
    int h, w0, d;
    if (!row_slot<NV>(H, WQ, h, w0, d)) return;
    const S* row = in + (stored_index(d, D, flips & 1) * st.d + stored_index(h, H, flips & 2) * st.h);
    T v[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) v[j] = (T)row[stored_index(tail_col<VEC>(w0 + j, W), W, flips & 4) * st.w];
    store_group<T, NV, VEC>(out + ((int64_t)d * H + h) * W + w0, v, w0, W);
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
    int oh, ow0, od;
    if (!row_slot<NWV>(Ho, WQ, oh, ow0, od)) return;
    const int64_t row = td[od] * st.d + th[oh] * st.h;
    int64_t v[NWV];
#pragma unroll
    for (int j = 0; j < NWV; j++) {
        v[j] = 0;
        const int64_t off = row + tw[tail_col<VEC>(ow0 + j, Wo)] * st.w;
#pragma unroll
        for (int k = 0; k < MAX_MASKS; k++)
            if (k < m.n && static_cast<const S*>(m.mask[k])[off] > (S)0) v[j] = m.value[k];
    }
    store_group<int64_t, NWV, VEC>(out + ((int64_t)od * Ho + oh) * Wo + ow0, v, ow0, Wo);
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

// The soft way back: float32 votes (C, Dg, Hg, Wg) on the training grid -> the label of the trilinearly zoomed votes on the scan as
// stored (contract: include/mi3d.h mi3d_restore_votes3).  F / M / S are the destination's axes by stride, as in
// restore_labels3_kernel, and the output is written in memory order whatever the orientation.  FA / MA say which grid axis (0 = D,
// 1 = H, 2 = W) F and M are: they decide which table a row comes from and which way the lanes run (below), never the arithmetic,
// which is always in grid-axis order, W innermost, then H, then D, so the layout cannot move a bit.
struct LerpRow {           // one destination index of one axis; layout shared with resample.py (_ROW1) and mi3d_lerp_row
    int32_t idx[2];        // grid indices of the two taps floor(c), floor(c) + 1, each clamped to [0, n_grid - 1]
    double w[2];           // 1 - t and t
};
static_assert(sizeof(LerpRow) == 24 && sizeof(mi3d_lerp_row) == 24, "table row layout");

struct Tap {               // a row with its indices turned into element offsets along its grid axis
    int64_t o0, o1;
    double w0, w1;
};
__device__ __forceinline__ Tap tap_of(const LerpRow& r, int64_t gs) { return Tap{r.idx[0] * gs, r.idx[1] * gs, r.w[0], r.w[1]}; }

// v_k of one output voxel: eight taps through L1 / L2, fp64.  Contraction is switched off with the pragma (not the __dmul_rn /
// __dadd_rn intrinsics): every product and every sum below is rounded on its own, no fused multiply-add, as the numpy model does.
__device__ __forceinline__ double lerp3(const float* __restrict__ p, const Tap& d, const Tap& h, const Tap& w) {
#pragma clang fp contract(off)
    const float* p00 = p + (d.o0 + h.o0);
    const float* p01 = p + (d.o0 + h.o1);
    const float* p10 = p + (d.o1 + h.o0);
    const float* p11 = p + (d.o1 + h.o1);
    const double r00 = (double)p00[w.o0] * w.w0 + (double)p00[w.o1] * w.w1;
    const double r01 = (double)p01[w.o0] * w.w0 + (double)p01[w.o1] * w.w1;
    const double r10 = (double)p10[w.o0] * w.w0 + (double)p10[w.o1] * w.w1;
    const double r11 = (double)p11[w.o0] * w.w0 + (double)p11[w.o1] * w.w1;
    const double s0 = r00 * h.w0 + r01 * h.w1;
    const double s1 = r10 * h.w0 + r11 * h.w1;
    return s0 * d.w0 + s1 * d.w1;
}
// the tap of grid axis A among those of the destination's S, M and F axes
template <int A, int FA, int MA>
__device__ __forceinline__ const Tap& axis_tap(const Tap& s, const Tap& m, const Tap& f) {
    if constexpr (A == FA) return f;
    else if constexpr (A == MA) return m;
    else return s;
}
template <int FA, int MA>
__device__ __forceinline__ double vote_at(const float* __restrict__ p, const Tap& s, const Tap& m, const Tap& f) {
    return lerp3(p, axis_tap<0, FA, MA>(s, m, f), axis_tap<1, FA, MA>(s, m, f), axis_tap<2, FA, MA>(s, m, f));
}

// A group is VG = 4 outputs of one thread.  The classes are outermost: one running (best value, best label) per output, so the
// first maximum under a strict `>` from class 0 falls out and the register count does not depend on C; 32 independent taps are in
// flight.  With 16 outputs in one class loop the compiler keeps 16 rows and 128 taps live: 256 VGPRs + 136 to 256 AGPRs, one wave
// per SIMD, and over 1 KB of scratch per lane when bounded to 128 registers; in groups of four it is 128 to 156 VGPRs, no scratch.
constexpr int VG = 4;
template <int FA, int MA>
__device__ __forceinline__ void vote_group(const float* __restrict__ votes, int C, int64_t cs, const Tap& ts, const Tap& tm,
                                           const Tap (&tf)[VG], double (&best)[VG], int (&lab)[VG]) {
#pragma unroll
    for (int j = 0; j < VG; j++) best[j] = vote_at<FA, MA>(votes, ts, tm, tf[j]), lab[j] = 0;
    for (int k = 1; k < C; k++) {
        const float* p = votes + k * cs;
#pragma unroll
        for (int j = 0; j < VG; j++) {
            const double v = vote_at<FA, MA>(p, ts, tm, tf[j]);
            if (v > best[j]) best[j] = v, lab[j] = k;
        }
    }
}

// Which thread does what.  Only the grid's W axis is contiguous in the votes, so the lanes of a wave run along the destination axis
// that IS the grid's W, whichever of F, M, S that is (LA): neighbouring lanes then read neighbouring taps.
//   F is W (LA = 0): x over (m, t), y = s; a row along F is cut in VG quarters of Q = ceil(nF / VG) and thread t owns f = t + j * Q,
//                    j = 0 .. 3: consecutive lanes store consecutive bytes (and floats of the confidence), no head and no tail
//   M is W (LA = 1): x over (piece, m), y = s, lanes along m; every lane owns a 16-byte piece of its own row, cut as the order-0
//                    kernel cuts it (head to the first aligned byte, whole pieces in one store each, scalar tail)
//   S is W (LA = 2): x over (piece, s), y = m, lanes along s; pieces as for LA = 1
// Measured on 4 x 192^3 -> 512 x 512 x 100 with lanes along 16-byte pieces of F in EVERY layout, as the order-0 kernel has them:
// 0.88 ms C-ordered, 2.05 ms F-ordered (every lane of a load in a line of its own), against 0.61 / 0.74 ms for interpolate + argmax
// in torch.  That form is not in the tree, so those figures cannot be measured again from it; the rows of the form built are in
// profiles/restore_soft_timing.txt.  A fastest axis that is not dense (oF != 1 with nF > 1) is stored an element at a time; it can
// come through the C entry only, resample.py admits dense layouts.
constexpr int votes_lane_axis(int FA, int MA) { return FA == 2 ? 0 : MA == 2 ? 1 : 2; }
template <int FA, int MA, bool CONF>
__global__ __launch_bounds__(BLK) void restore_votes3_kernel(const float* __restrict__ votes, int C, int64_t cs, uint8_t* __restrict__ out,
                                                             float* __restrict__ conf, int nI, int nO, int nF,
                                                             const LerpRow* __restrict__ tS, const LerpRow* __restrict__ tM,
                                                             const LerpRow* __restrict__ tF, int64_t gS, int64_t gM, int64_t gF,
                                                             int64_t oS, int64_t oM, int64_t oF) {
    constexpr int LA = votes_lane_axis(FA, MA);
    const int q = blockIdx.x * BLK + threadIdx.x;
    if (q >= nI * nO) return;
    const int ou = q / nI, in = q - ou * nI, y = blockIdx.y;
    const int m = LA == 0 ? ou : LA == 1 ? in : y, s = LA == 2 ? in : y;
    const int64_t orow = s * oS + m * oM;
    uint8_t* o = out + orow;
    const Tap ts = tap_of(tS[s], gS), tm = tap_of(tM[m], gM);
    Tap tf[VG];
    double best[VG];
    int lab[VG];
    if constexpr (LA == 0) {
#pragma unroll
        for (int j = 0; j < VG; j++) tf[j] = tap_of(tF[min(in + j * nI, nF - 1)], gF);          // past the end: the last row, never stored
        vote_group<FA, MA>(votes, C, cs, ts, tm, tf, best, lab);
#pragma unroll
        for (int j = 0; j < VG; j++) {
            const int f = in + j * nI;
            if (f < nF) {
                o[f * oF] = (uint8_t)lab[j];
                if constexpr (CONF) conf[orow + f * oF] = (float)best[j];          // (float): the one rounding to fp32
            }
        }
    } else {
        const int piece = ou;
        const int head = oF == 1 ? (int)((RW - (reinterpret_cast<uintptr_t>(o) & (RW - 1))) & (RW - 1)) : 0;
        const int f0 = piece == 0 ? 0 : head + (piece - 1) * RW;
        const int f1 = min(piece == 0 ? head : f0 + RW, nF);
        if (f0 >= f1) return;
        const bool whole = f1 - f0 == RW && oF == 1;
        float* c = CONF ? conf + (orow + f0) : nullptr;
        const bool cvec = whole && (reinterpret_cast<uintptr_t>(c) & 15) == 0;
        uint32_t a[RW / VG];
#pragma unroll
        for (int g = 0; g < RW / VG; g++) {
            if (f0 + VG * g >= f1) break;
#pragma unroll
            for (int j = 0; j < VG; j++) tf[j] = tap_of(tF[min(f0 + VG * g + j, nF - 1)], gF);
            vote_group<FA, MA>(votes, C, cs, ts, tm, tf, best, lab);
            a[g] = (uint32_t)lab[0] | (uint32_t)lab[1] << 8 | (uint32_t)lab[2] << 16 | (uint32_t)lab[3] << 24;
            if (!whole) {
#pragma unroll
                for (int j = 0; j < VG; j++) {
                    const int f = f0 + VG * g + j;
                    if (f < f1) {
                        o[f * oF] = (uint8_t)lab[j];
                        if constexpr (CONF) conf[orow + f * oF] = (float)best[j];
                    }
                }
            } else if constexpr (CONF) {
                if (cvec) {
                    reinterpret_cast<float4*>(c)[g] = float4{(float)best[0], (float)best[1], (float)best[2], (float)best[3]};
                } else {
#pragma unroll
                    for (int j = 0; j < VG; j++) c[VG * g + j] = (float)best[j];
                }
            }
        }
        if (whole) *reinterpret_cast<uint4*>(o + f0) = uint4{a[0], a[1], a[2], a[3]};
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
struct Dims {
    int d, h, w;
    bool ok() const { return sides_ok(d, h, w); }          // od rides in gridDim.y
};

// The argument check of every entry; `ptrs` is the entry's own null / alias test.  rows: the tables' row counts, which must be
// the sides of `out`.  st: a stored scan's strides (strides_ok; that the offset lies inside the caller's buffer is the caller's to
// guarantee: include/mi3d.h).  tabs16: three tables that must be 16-byte aligned.
int check_args(const char* name, bool ptrs, Dims in, Dims out, const int* rows, const SrcStrides* st = nullptr,
               const void* const* tabs16 = nullptr) {
    MI3D_CHECK_ARG(ptrs, "%s: null or aliased pointers", name);
    MI3D_CHECK_ARG(in.ok() && out.ok(), "%s: sides must be in [1, %d]", name, MAX_SIDE);
    MI3D_CHECK_ARG(!st || strides_ok(st->d, st->h, st->w), "%s: strides must be positive element counts", name);
    MI3D_CHECK_ARG(!rows || (rows[0] == out.d && rows[1] == out.h && rows[2] == out.w),
                   "%s: tables have (%d, %d, %d) rows, the output is (%d, %d, %d)", name, rows ? rows[0] : 0, rows ? rows[1] : 0,
                   rows ? rows[2] : 0, out.d, out.h, out.w);
    MI3D_CHECK_ARG(!tabs16 || (((uintptr_t)tabs16[0] | (uintptr_t)tabs16[1] | (uintptr_t)tabs16[2]) & 15) == 0,
                   "%s: tables must be 16-byte aligned", name);
    return 0;
}

// The launch shape of row_slot / store_group for NV outputs per thread
struct RowGrid {
    int WQ;
    dim3 grid;
    bool vec;
};
int row_grid(const char* name, Dims o, int NV, const void* out, RowGrid& g) {
    g.WQ = (o.w + NV - 1) / NV;
    MI3D_CHECK_ARG((int64_t)o.h * g.WQ < (int64_t)1 << 31, "%s: output plane too large", name);
    g.grid = dim3((unsigned)(((int64_t)o.h * g.WQ + BLK - 1) / BLK), (unsigned)o.d);
    g.vec = o.w % NV == 0 && aligned16(out);
    return 0;
}

// every axis with more than one element has the stride of a contiguous (D, H, W) volume
bool dense_ras(Dims n, SrcStrides st) {
    return (n.d == 1 || st.d == (int64_t)n.h * n.w) && (n.h == 1 || st.h == n.w) && (n.w == 1 || st.w == 1);
}

// One launcher per zoom family, behind the contiguous and the _src entry alike.  A float32 (cubic) / int64 (nearest) source with
// dense RAS strides takes the STRIDED = false instantiation: the same bits, without the stride arithmetic.
int cubic_launch(const char* name, const void* in, int src_dtype, SrcStrides st, float* out, Dims n, Dims o, const void* const (&tab)[3],
                 const int (&rows)[3], int ct, float lo, float hi, void* stream) {
    MI3D_TRY(check_args(name, in && out && in != (const void*)out && tab[0] && tab[1] && tab[2], n, o, rows, &st, tab));
    MI3D_CHECK_ARG(!ct || hi > lo, "%s: empty CT window", name);
    RowGrid g;
    MI3D_TRY(row_grid(name, o, CW, out, g));
    const bool known = dispatch_src(src_dtype, Types<uint8_t, int16_t, float>(), [&](auto tag) {
        using S = decltype(tag);
        auto launch = [&](auto kernel) {
            kernel<<<g.grid, BLK, 0, (hipStream_t)stream>>>((const S*)in, out, n.h, n.w, o.h, o.w, g.WQ, (const CubicRow*)tab[0],
                                                            (const CubicRow*)tab[1], (const CubicRow*)tab[2], ct, lo, hi, st);
        };
        if constexpr (std::is_same<S, float>::value)
            if (dense_ras(n, st)) return launch(g.vec ? zoom3_cubic_kernel<S, true, false> : zoom3_cubic_kernel<S, false, false>);
        launch(g.vec ? zoom3_cubic_kernel<S, true, true> : zoom3_cubic_kernel<S, false, true>);
    });
    MI3D_CHECK_ARG(known, "%s: the source is uint8, int16 or float32, not dtype code %d", name, src_dtype);
    MI3D_LAUNCH_CHECK();
    return 0;
}

int nearest_launch(const char* name, const void* in, int src_dtype, SrcStrides st, int64_t* out, Dims n, Dims o,
                   const int32_t* const (&tab)[3], const int (&rows)[3], void* stream) {
    MI3D_TRY(check_args(name, in && out && in != (const void*)out && tab[0] && tab[1] && tab[2], n, o, rows, &st));
    RowGrid g;
    MI3D_TRY(row_grid(name, o, NWV, out, g));
    const bool known = dispatch_src(src_dtype, Types<uint8_t, int16_t, int64_t>(), [&](auto tag) {
        using S = decltype(tag);
        auto launch = [&](auto kernel) {
            kernel<<<g.grid, BLK, 0, (hipStream_t)stream>>>((const S*)in, out, n.h, n.w, o.h, o.w, g.WQ, tab[0], tab[1], tab[2], st);
        };
        if constexpr (std::is_same<S, int64_t>::value)
            if (dense_ras(n, st)) return launch(g.vec ? zoom3_nearest_kernel<S, true, false> : zoom3_nearest_kernel<S, false, false>);
        launch(g.vec ? zoom3_nearest_kernel<S, true, true> : zoom3_nearest_kernel<S, false, true>);
    });
    MI3D_CHECK_ARG(known, "%s: the source is uint8, int16 or int64, not dtype code %d", name, src_dtype);
    MI3D_LAUNCH_CHECK();
    return 0;
}

template <typename S, typename T>
int reorient3_launch(const S* in, T* out, Dims n, SrcStrides st, int flips, hipStream_t s) {
    // the stored-fastest axis, where it is not W: D or H with stride 1 and more than one element
    const int fast = (st.w == 1 || n.w == 1) ? 2 : (st.h == 1 && n.h > 1) ? 1 : (st.d == 1 && n.d > 1) ? 0 : 2;
    if (fast == 2) {
        RowGrid g;
        MI3D_TRY(row_grid("mi3d_reorient3", n, 16 / (int)sizeof(T), out, g));
        auto kernel = g.vec ? reorient3_stream_kernel<S, T, true> : reorient3_stream_kernel<S, T, false>;
        kernel<<<g.grid, BLK, 0, s>>>(in, out, n.d, n.h, n.w, g.WQ, st, flips);
    } else {
        const int nF = fast == 1 ? n.h : n.d, nG = fast == 1 ? n.d : n.h;
        const int tilesW = (n.w + TILE - 1) / TILE, tilesF = (nF + TILE - 1) / TILE;
        dim3 grid((unsigned)(tilesF * tilesW), (unsigned)nG);
        if (fast == 1)
            reorient3_tile_kernel<S, T><<<grid, BLK, 0, s>>>(in, out, nF, nG, n.w, tilesW, st.h, st.d, st.w, flips & 2, flips & 1, flips & 4,
                                                             (int64_t)n.w, (int64_t)n.h * n.w);
        else
            reorient3_tile_kernel<S, T><<<grid, BLK, 0, s>>>(in, out, nF, nG, n.w, tilesW, st.d, st.h, st.w, flips & 1, flips & 2, flips & 4,
                                                             (int64_t)n.h * n.w, (int64_t)n.w);
    }
    MI3D_LAUNCH_CHECK();
    return 0;
}

// The walk of the two restore kernels over a destination seen in RAS order: its axes by increasing stride, an axis of one element
// last among equals: a[0] = F, a[1] = M, a[2] = S; each with its side, destination stride, the grid's stride along it, its table
// and which grid axis it is (0 = D, 1 = H, 2 = W).  pieces(): the 16-byte pieces of a row along F, the head included.
template <typename T>
struct RestoreWalk {
    struct Axis { int n; int64_t os, gs; const T* t; int ga; };
    Axis a[3];
    int pieces() const { return 1 + (a[0].n + RW - 1) / RW; }
    RestoreWalk(Dims g, Dims n, SrcStrides st, const T* td, const T* th, const T* tw)
        : a{{n.d, st.d, (int64_t)g.h * g.w, td, 0}, {n.h, st.h, (int64_t)g.w, th, 1}, {n.w, st.w, 1, tw, 2}} {
        auto before = [](const Axis& x, const Axis& y) { return (x.n > 1) != (y.n > 1) ? x.n > 1 : x.os < y.os; };
        if (before(a[1], a[0])) std::swap(a[0], a[1]);
        if (before(a[2], a[1])) std::swap(a[1], a[2]);
        if (before(a[1], a[0])) std::swap(a[0], a[1]);
    }
};
// the launch shape: x over nO * nI threads, the lanes along the nI axis, y the third axis
int walk_grid(const char* name, int nI, int nO, int ny, dim3& grid) {
    MI3D_CHECK_ARG((int64_t)nI * nO < (int64_t)1 << 31, "%s: output plane too large", name);
    grid = dim3((unsigned)(((int64_t)nI * nO + BLK - 1) / BLK), (unsigned)ny);
    return 0;
}
}  // namespace

extern "C" {

size_t mi3d_zoom3_workspace_bytes(int D, int H, int W) {
    if (!Dims{D, H, W}.ok()) {
        mi3d_set_error("mi3d_zoom3_workspace_bytes: sides must be in [1, %d]", MAX_SIDE);
        return 0;
    }
    return (((size_t)D * H * W * sizeof(float)) + 255) & ~(size_t)255;
}

int mi3d_zoom3_cubic(const float* in, float* out, int D, int H, int W, int Do, int Ho, int Wo, const void* table_d, int rows_d,
                     const void* table_h, int rows_h, const void* table_w, int rows_w, int ct_window, float window_min,
                     float window_max, void* stream) {
    return cubic_launch("mi3d_zoom3_cubic", in, MI3D_SRC_F32, {(int64_t)H * W, W, 1}, out, {D, H, W}, {Do, Ho, Wo},
                        {table_d, table_h, table_w}, {rows_d, rows_h, rows_w}, ct_window, window_min, window_max, stream);
}

int mi3d_zoom3_cubic_src(const void* in, int src_dtype, int64_t stride_d, int64_t stride_h, int64_t stride_w, float* out, int D,
                         int H, int W, int Do, int Ho, int Wo, const void* table_d, int rows_d, const void* table_h, int rows_h,
                         const void* table_w, int rows_w, int ct_window, float window_min, float window_max, void* stream) {
    return cubic_launch("mi3d_zoom3_cubic_src", in, src_dtype, {stride_d, stride_h, stride_w}, out, {D, H, W}, {Do, Ho, Wo},
                        {table_d, table_h, table_w}, {rows_d, rows_h, rows_w}, ct_window, window_min, window_max, stream);
}

int mi3d_zoom3_nearest_i64(const int64_t* in, int64_t* out, int D, int H, int W, int Do, int Ho, int Wo, const int32_t* index_d,
                           int rows_d, const int32_t* index_h, int rows_h, const int32_t* index_w, int rows_w, void* stream) {
    return nearest_launch("mi3d_zoom3_nearest_i64", in, MI3D_SRC_I64, {(int64_t)H * W, W, 1}, out, {D, H, W}, {Do, Ho, Wo},
                          {index_d, index_h, index_w}, {rows_d, rows_h, rows_w}, stream);
}

int mi3d_zoom3_nearest_src(const void* in, int src_dtype, int64_t stride_d, int64_t stride_h, int64_t stride_w, int64_t* out, int D,
                           int H, int W, int Do, int Ho, int Wo, const int32_t* index_d, int rows_d, const int32_t* index_h,
                           int rows_h, const int32_t* index_w, int rows_w, void* stream) {
    return nearest_launch("mi3d_zoom3_nearest_src", in, src_dtype, {stride_d, stride_h, stride_w}, out, {D, H, W}, {Do, Ho, Wo},
                          {index_d, index_h, index_w}, {rows_d, rows_h, rows_w}, stream);
}

int mi3d_reorient3(const void* in, int src_dtype, void* out, int out_i64, int D, int H, int W, int64_t stride_d, int64_t stride_h,
                   int64_t stride_w, int flip_mask, void* stream) {
    const Dims n{D, H, W};
    const SrcStrides st{stride_d, stride_h, stride_w};
    MI3D_TRY(check_args("mi3d_reorient3", in && out && in != out, n, n, nullptr, &st));
    MI3D_CHECK_ARG(flip_mask >= 0 && flip_mask <= 7, "mi3d_reorient3: flip_mask %d outside 0..7", flip_mask);
    int rc = 0;
    auto run = [&](auto dst, auto sources) {
        return dispatch_src(src_dtype, sources, [&](auto tag) {
            rc = reorient3_launch((const decltype(tag)*)in, (decltype(dst)*)out, n, st, flip_mask, (hipStream_t)stream);
        });
    };
    const bool known = out_i64 ? run(int64_t(), Types<uint8_t, int16_t, int64_t>()) : run(float(), Types<uint8_t, int16_t, float>());
    MI3D_CHECK_ARG(known, "mi3d_reorient3: %s volume is made from uint8, int16 or %s, not dtype code %d",
                   out_i64 ? "an int64" : "a float32", out_i64 ? "int64" : "float32", src_dtype);
    return rc;
}

int mi3d_merge_masks3(const mi3d_mask_list* masks, int src_dtype, int64_t stride_d, int64_t stride_h, int64_t stride_w, int64_t* out,
                      int D, int H, int W, int Do, int Ho, int Wo, const int32_t* index_d, int rows_d, const int32_t* index_h,
                      int rows_h, const int32_t* index_w, int rows_w, void* stream) {
    const char* name = "mi3d_merge_masks3";
    const Dims o{Do, Ho, Wo};
    const SrcStrides st{stride_d, stride_h, stride_w};
    const int rows[3] = {rows_d, rows_h, rows_w};
    MI3D_TRY(check_args(name, masks && out && index_d && index_h && index_w, {D, H, W}, o, rows, &st));
    MI3D_CHECK_ARG(masks->n >= 0 && masks->n <= MAX_MASKS, "%s: %d masks, at most %d fit one launch", name, masks->n, MAX_MASKS);
    MaskArgs m{};
    m.n = masks->n;
    for (int k = 0; k < masks->n; k++) {
        MI3D_CHECK_ARG(masks->mask[k] && masks->mask[k] != (const void*)out, "%s: mask %d is null or is the output", name, k);
        m.mask[k] = masks->mask[k];
        m.value[k] = masks->value[k];
    }
    RowGrid g;
    MI3D_TRY(row_grid(name, o, NWV, out, g));
    const bool known = dispatch_src(src_dtype, Types<uint8_t, float>(), [&](auto tag) {
        using S = decltype(tag);
        auto kernel = g.vec ? merge_masks3_kernel<S, true> : merge_masks3_kernel<S, false>;
        kernel<<<g.grid, BLK, 0, (hipStream_t)stream>>>(m, out, Ho, Wo, g.WQ, index_d, index_h, index_w, st);
    });
    MI3D_CHECK_ARG(known, "%s: masks are uint8 or float32, not dtype code %d", name, src_dtype);
    MI3D_LAUNCH_CHECK();
    return 0;
}

int mi3d_restore_labels3(const uint8_t* grid, int Dg, int Hg, int Wg, uint8_t* out, int D, int H, int W, int64_t stride_d,
                         int64_t stride_h, int64_t stride_w, const int32_t* index_d, const int32_t* index_h, const int32_t* index_w,
                         void* stream) {
    const SrcStrides st{stride_d, stride_h, stride_w};
    MI3D_TRY(check_args("mi3d_restore_labels3", grid && out && grid != out && index_d && index_h && index_w, {Dg, Hg, Wg}, {D, H, W},
                        nullptr, &st));
    const RestoreWalk<int32_t> k({Dg, Hg, Wg}, {D, H, W}, st, index_d, index_h, index_w);
    const auto &F = k.a[0], &M = k.a[1], &S = k.a[2];
    dim3 grd;
    MI3D_TRY(walk_grid("mi3d_restore_labels3", k.pieces(), M.n, S.n, grd));
    restore_labels3_kernel<<<grd, BLK, 0, (hipStream_t)stream>>>(grid, out, M.n, F.n, k.pieces(), S.t, M.t, F.t, S.gs, M.gs, F.gs, S.os, M.os,
                                                                 F.n > 1 ? F.os : 1);
    MI3D_LAUNCH_CHECK();
    return 0;
}

int mi3d_restore_votes3(const float* votes, int C, int Dg, int Hg, int Wg, uint8_t* out, float* confidence, int D, int H, int W,
                        int64_t stride_d, int64_t stride_h, int64_t stride_w, const mi3d_lerp_row* rows_d, const mi3d_lerp_row* rows_h,
                        const mi3d_lerp_row* rows_w, void* stream) {
    const char* name = "mi3d_restore_votes3";
    const SrcStrides st{stride_d, stride_h, stride_w};
    const void *v = votes, *o = out, *c = confidence;
    MI3D_TRY(check_args(name, v && o && v != o && v != c && o != c && rows_d && rows_h && rows_w, {Dg, Hg, Wg}, {D, H, W}, nullptr, &st));
    MI3D_CHECK_ARG(C >= 2 && C <= 8, "%s: %d classes, 2 to 8 are supported (the range of the head kernels)", name, C);
    const RestoreWalk<LerpRow> k({Dg, Hg, Wg}, {D, H, W}, st, (const LerpRow*)rows_d, (const LerpRow*)rows_h, (const LerpRow*)rows_w);
    const auto &F = k.a[0], &M = k.a[1], &S = k.a[2];
    const int lane = votes_lane_axis(F.ga, M.ga);
    const int nI = lane == 0 ? (F.n + VG - 1) / VG : lane == 1 ? M.n : S.n, nO = lane == 0 ? M.n : k.pieces();
    dim3 grd;
    MI3D_TRY(walk_grid(name, nI, nO, lane == 2 ? M.n : S.n, grd));
    const int64_t cs = (int64_t)Dg * Hg * Wg;
    auto launch = [&](auto kernel) {
        kernel<<<grd, BLK, 0, (hipStream_t)stream>>>(votes, C, cs, out, confidence, nI, nO, F.n, S.t, M.t, F.t, S.gs, M.gs, F.gs, S.os,
                                                        M.os, F.n > 1 ? F.os : 1);
    };
    auto pick = [&](auto fa, auto ma) {
        constexpr int FA = decltype(fa)::value, MA = decltype(ma)::value;
        launch(confidence ? restore_votes3_kernel<FA, MA, true> : restore_votes3_kernel<FA, MA, false>);
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    switch (F.ga * 3 + M.ga) {
        case 1: pick(I0(), I1()); break;
        case 2: pick(I0(), I2()); break;
        case 3: pick(I1(), I0()); break;
        case 5: pick(I1(), I2()); break;
        case 6: pick(I2(), I0()); break;
        default: pick(I2(), I1()); break;
    }
    MI3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
