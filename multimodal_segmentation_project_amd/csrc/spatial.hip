// spatial.hip — spatial augmentation of one (C, D, H, W) sample on the GPU: the reference's random_flip (np.flip over axes 1, 2, 3,
// utils/dataloader.py:207-213) and random_rotate (scipy.ndimage.rotate(reshape=False, mode='nearest') in one plane, order=1 for
// the image and order=0 for the label, :215-221) as ONE gather pass over image and label.
//   plane_rows_kernel    the plane is (D, H): a whole W-row shares its source rows and weights; 16 bytes per access
//                        (scalar route for W % 4 != 0).  INTERP = false is the pure flip: a copy with reversed indices, no fp64
//   plane_gather_kernel  W is in the plane, (D, W) or (H, W): one output voxel per lane, consecutive lanes on consecutive W
// The coordinate is scipy's, operation by operation, in IEEE double with contraction OFF: (o0*M[i][0] + o1*M[i][1]) + off[i],
// clamped to [0, n-1]; the label reads floor(cc + 0.5); the image blends the 2x2 taps in double and rounds once to fp32.
// A flipped axis reverses the SOURCE index after the mapping, so the pass equals rotate(flip(x)) bit for bit.
// Every source index is inside the volume by construction (clamped coordinate, upper tap min(f + 1, n - 1)).
#include "ops.h"
#include "../../include/mi3d.h"

namespace {
constexpr int BLK = 256;
constexpr int VW = 4;      // rows kernel: consecutive W outputs per thread (one 16-byte image store, two 16-byte label stores)

struct PlaneMap { double m00, m01, m10, m11, off0, off1; };

// products first, then their sum, then the offset; each operation rounded on its own (hipcc would contract to FMA by default)
__device__ __forceinline__ double plane_coord(int o0, int o1, double ma, double mb, double off, int n) {
#pragma clang fp contract(off)
    const double cc = ((double)o0 * ma + (double)o1 * mb) + off;
    return fmin(fmax(cc, 0.0), (double)(n - 1));
}

__device__ __forceinline__ int flipped(int i, int n, bool flip) { return flip ? n - 1 - i : i; }

__device__ __forceinline__ int nearest_index(double cc, int n, bool flip) { return flipped((int)floor(cc + 0.5), n, flip); }

struct Taps { int lo, hi; double t; };      // source indices of the two taps of one axis (already flipped) and the upper one's weight
__device__ __forceinline__ Taps linear_taps(double cc, int n, bool flip) {
    const double f = floor(cc);
    const int lo = (int)f;
    Taps r;
    r.t = cc - f;
    r.lo = flipped(lo, n, flip);
    r.hi = flipped(min(lo + 1, n - 1), n, flip);
    return r;
}

struct Weights { double w00, w01, w10, w11; };
__device__ __forceinline__ Weights tap_weights(double t0, double t1) {
#pragma clang fp contract(off)
    const double a0 = 1.0 - t0, a1 = 1.0 - t1;
    Weights w = {a0 * a1, a0 * t1, t0 * a1, t0 * t1};
    return w;
}
// order (f0,f1), (f0,f1+1), (f0+1,f1), (f0+1,f1+1); products and sums as written, one rounding to fp32
__device__ __forceinline__ float blend(const Weights& w, float v00, float v01, float v10, float v11) {
#pragma clang fp contract(off)
    double s = w.w00 * (double)v00;
    s = s + w.w01 * (double)v01;
    s = s + w.w10 * (double)v10;
    s = s + w.w11 * (double)v11;
    return (float)s;
}

struct Voxel { int c, od, oh, ow; };
__device__ __forceinline__ Voxel decode(int64_t q, int D, int H, int WQ) {      // q over (c, od, oh, index along W), W fastest
    Voxel v;
    int64_t r = q / WQ;
    v.ow = (int)(q - r * WQ);
    v.oh = (int)(r % H);
    r /= H;
    v.od = (int)(r % D);
    v.c = (int)(r / D);
    return v;
}

// One thread: VW consecutive W outputs of row (c, od, oh).  VEC needs W % VW == 0 and 16-byte aligned bases.
template <bool VEC, bool INTERP>
__global__ __launch_bounds__(BLK) void plane_rows_kernel(const float* __restrict__ img_in, float* __restrict__ img_out,
                                                         const int64_t* __restrict__ lab_in, int64_t* __restrict__ lab_out, int D, int H,
                                                         int W, int WQ, PlaneMap m, int flip_mask, int64_t total) {
    const int64_t q = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (q >= total) return;
    const Voxel v = decode(q, D, H, WQ);
    const bool fd = flip_mask & 1, fh = flip_mask & 2, fw = flip_mask & 4;
    const int w0 = v.ow * VW;
    const int sw0 = fw ? W - VW - w0 : w0;                     // VEC: first source column of the 16-byte group
    const int64_t plane0 = (int64_t)v.c * D;
    auto row = [&](int d, int h) { return ((plane0 + d) * H + h) * W; };
    const int64_t orow = row(v.od, v.oh);
    double cc0 = 0.0, cc1 = 0.0;
    if constexpr (INTERP) {
        cc0 = plane_coord(v.od, v.oh, m.m00, m.m01, m.off0, D);
        cc1 = plane_coord(v.od, v.oh, m.m10, m.m11, m.off1, H);
    }
    if (lab_in) {
        const int sd = INTERP ? nearest_index(cc0, D, fd) : flipped(v.od, D, fd);
        const int sh = INTERP ? nearest_index(cc1, H, fh) : flipped(v.oh, H, fh);
        const int64_t* src = lab_in + row(sd, sh);
        int64_t* dst = lab_out + orow + w0;
        if constexpr (VEC) {
            const longlong2 a = *reinterpret_cast<const longlong2*>(src + sw0), b = *reinterpret_cast<const longlong2*>(src + sw0 + 2);
            longlong2 o0, o1;
            if (fw) { o0.x = b.y; o0.y = b.x; o1.x = a.y; o1.y = a.x; } else { o0 = a; o1 = b; }
            *reinterpret_cast<longlong2*>(dst) = o0;
            *reinterpret_cast<longlong2*>(dst + 2) = o1;
        } else {
#pragma unroll
            for (int j = 0; j < VW; j++)
                if (w0 + j < W) dst[j] = src[flipped(w0 + j, W, fw)];
        }
    }
    if (img_in) {
        float* dst = img_out + orow + w0;
        if constexpr (INTERP) {
            const Taps t0 = linear_taps(cc0, D, fd), t1 = linear_taps(cc1, H, fh);
            const Weights wt = tap_weights(t0.t, t1.t);
            const float *r00 = img_in + row(t0.lo, t1.lo), *r01 = img_in + row(t0.lo, t1.hi);
            const float *r10 = img_in + row(t0.hi, t1.lo), *r11 = img_in + row(t0.hi, t1.hi);
            if constexpr (VEC) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(r00 + sw0), b = *reinterpret_cast<const f32x4*>(r01 + sw0);
                const f32x4 c = *reinterpret_cast<const f32x4*>(r10 + sw0), d = *reinterpret_cast<const f32x4*>(r11 + sw0);
                f32x4 o;
#pragma unroll
                for (int j = 0; j < VW; j++) {
                    const int k = fw ? VW - 1 - j : j;
                    o[j] = blend(wt, a[k], b[k], c[k], d[k]);
                }
                *reinterpret_cast<f32x4*>(dst) = o;
            } else {
#pragma unroll
                for (int j = 0; j < VW; j++)
                    if (w0 + j < W) {
                        const int sw = flipped(w0 + j, W, fw);
                        dst[j] = blend(wt, r00[sw], r01[sw], r10[sw], r11[sw]);
                    }
            }
        } else {
            const float* src = img_in + row(flipped(v.od, D, fd), flipped(v.oh, H, fh));
            if constexpr (VEC) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(src + sw0);
                f32x4 o;
#pragma unroll
                for (int j = 0; j < VW; j++) o[j] = a[fw ? VW - 1 - j : j];
                *reinterpret_cast<f32x4*>(dst) = o;
            } else {
#pragma unroll
                for (int j = 0; j < VW; j++)
                    if (w0 + j < W) dst[j] = src[flipped(w0 + j, W, fw)];
            }
        }
    }
}

// One thread: one output voxel; the plane is (D, W) (AX0_D) or (H, W).  The output index is q itself.
template <bool AX0_D>
__global__ __launch_bounds__(BLK) void plane_gather_kernel(const float* __restrict__ img_in, float* __restrict__ img_out,
                                                           const int64_t* __restrict__ lab_in, int64_t* __restrict__ lab_out, int D, int H,
                                                           int W, PlaneMap m, int flip_mask, int64_t total) {
    const int64_t q = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (q >= total) return;
    const Voxel v = decode(q, D, H, W);
    const bool fd = flip_mask & 1, fh = flip_mask & 2, fw = flip_mask & 4;
    const int o0 = AX0_D ? v.od : v.oh, n0 = AX0_D ? D : H;
    const bool f0 = AX0_D ? fd : fh;
    const int across = AX0_D ? flipped(v.oh, H, fh) : flipped(v.od, D, fd);     // source index on the axis outside the plane
    const int64_t plane0 = (int64_t)v.c * D;
    auto row = [&](int i0) { return AX0_D ? ((plane0 + i0) * H + across) * W : ((plane0 + across) * H + i0) * W; };
    const double cc0 = plane_coord(o0, v.ow, m.m00, m.m01, m.off0, n0);
    const double cc1 = plane_coord(o0, v.ow, m.m10, m.m11, m.off1, W);
    if (lab_in) lab_out[q] = lab_in[row(nearest_index(cc0, n0, f0)) + nearest_index(cc1, W, fw)];
    if (img_in) {
        const Taps t0 = linear_taps(cc0, n0, f0), t1 = linear_taps(cc1, W, fw);
        const float *lo = img_in + row(t0.lo), *hi = img_in + row(t0.hi);
        img_out[q] = blend(tap_weights(t0.t, t1.t), lo[t1.lo], lo[t1.hi], hi[t1.lo], hi[t1.hi]);
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

int plane_affine(const float* img_in, float* img_out, const int64_t* lab_in, int64_t* lab_out, int C, int D, int H, int W, int ax0,
                 int ax1, const double* matrix, const double* offset, int flip_mask, hipStream_t s) {
    MI3D_CHECK_ARG(matrix && offset, "mi3d_plane_affine: null matrix or offset");
    MI3D_CHECK_ARG(!img_in == !img_out && !lab_in == !lab_out && (img_in || lab_in),
                   "mi3d_plane_affine: the image pair, the label pair or both, each with its input AND its output");
    MI3D_CHECK_ARG((!img_in || img_in != img_out) && (!lab_in || lab_in != lab_out), "mi3d_plane_affine: input and output alias");
    MI3D_CHECK_ARG(C >= 1 && D >= 1 && H >= 1 && W >= 1, "mi3d_plane_affine: sizes must be positive, got (%d, %d, %d, %d)", C, D, H, W);
    MI3D_CHECK_ARG((int64_t)C * D <= INT32_MAX && (int64_t)H * W <= INT32_MAX && (int64_t)C * D * ((int64_t)H * W) <= INT32_MAX,
                   "mi3d_plane_affine: more than 2^31 - 1 voxels");
    const int64_t n = (int64_t)C * D * H * W;
    MI3D_CHECK_ARG(1 <= ax0 && ax0 < ax1 && ax1 <= 3, "mi3d_plane_affine: axes (%d, %d) are not 1 <= ax0 < ax1 <= 3 of (C, D, H, W)", ax0, ax1);
    MI3D_CHECK_ARG(flip_mask >= 0 && flip_mask <= 7, "mi3d_plane_affine: flip_mask %d has bits beyond axes 1..3", flip_mask);
    const PlaneMap m = {matrix[0], matrix[1], matrix[2], matrix[3], offset[0], offset[1]};
    const bool identity = m.m00 == 1.0 && m.m01 == 0.0 && m.m10 == 0.0 && m.m11 == 1.0 && m.off0 == 0.0 && m.off1 == 0.0;
    auto blocks = [](int64_t total) { return (unsigned)((total + BLK - 1) / BLK); };
    if (identity || (ax0 == 1 && ax1 == 2)) {
        const int WQ = (W + VW - 1) / VW;
        const int64_t total = (int64_t)C * D * H * WQ;
        const bool vec = W % VW == 0 && al16(img_in) && al16(img_out) && al16(lab_in) && al16(lab_out);
#define MI3D_ROWS(VEC, INTERP) \
    plane_rows_kernel<VEC, INTERP><<<blocks(total), BLK, 0, s>>>(img_in, img_out, lab_in, lab_out, D, H, W, WQ, m, flip_mask, total)
        if (identity) { if (vec) MI3D_ROWS(true, false); else MI3D_ROWS(false, false); }
        else { if (vec) MI3D_ROWS(true, true); else MI3D_ROWS(false, true); }
#undef MI3D_ROWS
    } else if (ax0 == 1) {
        plane_gather_kernel<true><<<blocks(n), BLK, 0, s>>>(img_in, img_out, lab_in, lab_out, D, H, W, m, flip_mask, n);
    } else {
        plane_gather_kernel<false><<<blocks(n), BLK, 0, s>>>(img_in, img_out, lab_in, lab_out, D, H, W, m, flip_mask, n);
    }
    MI3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int mi3d_plane_affine(const float* img_in, float* img_out, const int64_t* lab_in, int64_t* lab_out, int C, int D, int H, int W,
                                 int ax0, int ax1, const double* matrix, const double* offset, int flip_mask, void* stream) {
    return plane_affine(img_in, img_out, lab_in, lab_out, C, D, H, W, ax0, ax1, matrix, offset, flip_mask, (hipStream_t)stream);
}
