// warp.hip — the 3-D affine + elastic spatial augmentation of one (C, D, H, W) sample on the GPU: the MONAI RandAffined /
// Rand3DElasticd block that the reference's combined_transform() lists and leaves commented out (utils/dataloader.py:227-248),
// as ONE smoothed random displacement field and ONE gather that reads image and label through the same coordinates.
//   field_w_kernel      noise from the counter hash (never stored), smoothed along W: a wave stages the 64 + 2R noise values of its
//                       piece of a row in LDS once and convolves from there
//   field_axis_kernel   the H pass and the D pass: lanes along W, every tap read is a coalesced row piece
//   warp3_kernel        four consecutive output W per thread; one field read and one coordinate computation serve every channel of
//                       image and label; 16-byte stores (scalar route for Wo % 4 != 0 or unaligned pointers, same bits)
// Contract and arithmetic: include/mi3d.h mi3d_elastic_field / mi3d_warp3 / mi3d_warp3_at.  All coordinate and interpolation arithmetic is IEEE
// double with contraction OFF, operation by operation as written there.  Every source index is inside the volume by construction:
// "outside" (not 0 <= s <= n - 1, so a NaN is outside) is decided on the coordinate, then it is clamped to [0, n - 1] (a NaN clamps to 0) and the upper tap is
// min(f + 1, n - 1); a smoothing tap beyond the volume is skipped, not read.
#include "ops.h"
#include "rng.h"
#include "../../include/mi3d.h"

namespace {
constexpr int BLK = 256;
constexpr int VW = 4;          // gather: consecutive W outputs per thread
constexpr int FW = 64;         // W pass: outputs per wave
constexpr int MAXR = MI3D_ELASTIC_MAX_RADIUS;

struct TapTable { int R; double g[2 * MAXR + 1]; };      // g[j + R] weighs the source at offset j, j = -R..R

// an exact dyadic in [-1, 1): the top 24 bits of the hash of (seed, component * V + voxel) as a signed multiple of 2^-23
__device__ __forceinline__ float field_noise(uint64_t seed_mixed, uint64_t idx) {
    const uint64_t k = mix64a(seed_mixed ^ idx) >> 40;
    return (float)((int)k - (1 << 23)) * (1.f / 8388608.f);
}

// sum over j = -R..R of g[j] * read(j) for the taps with 0 <= i + j < n, in ascending j, each product and sum rounded on its own.  A
// tap beyond the volume is neither read nor added.  (Issuing eight reads ahead of their sums, with selects for the skipped taps,
// measured 18-26 % slower at 192^3: profiles/warp_timing.txt.)
template <typename Read>
__device__ __forceinline__ double tap_sum(const TapTable& tp, int i, int n, Read read) {
    const int R = tp.R;
    double s = 0.0;
    for (int j = -R; j <= R; j++) {
#pragma clang fp contract(off)
        if (i + j >= 0 && i + j < n) s = s + tp.g[j + R] * (double)read(j);
    }
    return s;
}

// One wave: FW consecutive outputs of one row (a, d, h) of the (3, D, H, W) field.  row * W is a * V + the row's first voxel index.
__global__ __launch_bounds__(BLK) void field_w_kernel(float* __restrict__ out, int W, uint64_t seed_mixed, TapTable tp, int nchunk,
                                                      int64_t items) {
    __shared__ float s_n[BLK / 64][FW + 2 * MAXR];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, R = tp.R;
    const int64_t item = (int64_t)blockIdx.x * (BLK / 64) + wave;
    const bool live = item < items;
    const int64_t row = live ? item / nchunk : 0;
    const int w0 = live ? (int)(item - row * nchunk) * FW : 0;
    if (live)
        for (int i = lane; i < FW + 2 * R; i += 64) {
            const int w = w0 - R + i;
            if (w >= 0 && w < W) s_n[wave][i] = field_noise(seed_mixed, (uint64_t)(row * W + w));
        }
    __syncthreads();
    const int w = w0 + lane;
    if (!live || w >= W) return;
    out[row * W + w] = (float)tap_sum(tp, w, W, [&](int j) { return s_n[wave][lane + R + j]; });
}

// One thread: one voxel of the (3, D, H, W) field, smoothed along H (ALONG_H) or along D.  q is the voxel's index in src and dst.
template <bool ALONG_H>
__global__ __launch_bounds__(BLK) void field_axis_kernel(const float* __restrict__ src, float* __restrict__ dst, int D, int H, int W,
                                                         TapTable tp, int64_t total) {
    const int64_t q = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (q >= total) return;
    const int64_t r = q / W;
    const int i = ALONG_H ? (int)(r % H) : (int)((r / H) % D), n = ALONG_H ? H : D;
    const int64_t stride = ALONG_H ? W : (int64_t)H * W;
    dst[q] = (float)tap_sum(tp, i, n, [&](int j) { return src[q + j * stride]; });
}

struct WarpMap {
    double m[9], off[3], half_o[3], t[3], mag;      // off[a] = (n_a - 1) / 2 + t_a;  half_o[a] = (no_a - 1) / 2;  t: the translation
    int n[3], no[3];
};

// where one output voxel reads: the taps of the image (indices and upper weights per axis), the label's voxel, and whether the
// sampling point lies outside the input
struct Site { int lo[3], hi[3]; double t[3]; int lab; bool outside; };

__device__ __forceinline__ Site site_of(const WarpMap& m, const double (&off)[3], int od, int oh, int ow, float ud, float uh, float uw,
                                        bool has_field) {
#pragma clang fp contract(off)
    double p[3] = {(double)od - m.half_o[0], (double)oh - m.half_o[1], (double)ow - m.half_o[2]};
    if (has_field) {
        p[0] = p[0] + m.mag * (double)ud;
        p[1] = p[1] + m.mag * (double)uh;
        p[2] = p[2] + m.mag * (double)uw;
    }
    Site st;
    st.outside = false;
    int lab[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double s = ((m.m[3 * a] * p[0] + m.m[3 * a + 1] * p[1]) + m.m[3 * a + 2] * p[2]) + off[a];
        const double top = (double)(m.n[a] - 1);
        st.outside = st.outside || !(s >= 0.0 && s <= top);      // a NaN is outside
        s = fmin(fmax(s, 0.0), top);                      // inside [0, n - 1] from here on, whatever s was
        const double f = floor(s);
        st.lo[a] = (int)f;
        st.hi[a] = min(st.lo[a] + 1, m.n[a] - 1);
        st.t[a] = s - f;
        lab[a] = (int)floor(s + 0.5);
    }
    st.lab = (lab[0] * m.n[1] + lab[1]) * m.n[2] + lab[2];
    return st;
}

__device__ __forceinline__ double lerp_d(double lo, double hi, double t) {
#pragma clang fp contract(off)
    return lo * (1.0 - t) + hi * t;
}

// W level on the four (d, h) rows, then H, then D; one rounding to float32
__device__ __forceinline__ float trilinear(const float* __restrict__ x, const WarpMap& m, const Site& st) {
    const int HW = m.n[1] * m.n[2];
    const float *r00 = x + (int64_t)st.lo[0] * HW + st.lo[1] * m.n[2], *r01 = x + (int64_t)st.lo[0] * HW + st.hi[1] * m.n[2];
    const float *r10 = x + (int64_t)st.hi[0] * HW + st.lo[1] * m.n[2], *r11 = x + (int64_t)st.hi[0] * HW + st.hi[1] * m.n[2];
    const int a = st.lo[2], b = st.hi[2];
    const double w00 = lerp_d((double)r00[a], (double)r00[b], st.t[2]), w01 = lerp_d((double)r01[a], (double)r01[b], st.t[2]);
    const double w10 = lerp_d((double)r10[a], (double)r10[b], st.t[2]), w11 = lerp_d((double)r11[a], (double)r11[b], st.t[2]);
    return (float)lerp_d(lerp_d(w00, w01, st.t[1]), lerp_d(w10, w11, st.t[1]), st.t[0]);
}

// One thread: VW consecutive W outputs of output row (od, oh), every channel.  VEC needs Wo % VW == 0 and 16-byte aligned field and
// output bases.  start: NULL, or three device ints, the window's first voxel: the offset is then (start_a + (no_a - 1) / 2) + t_a,
// formed here in that order, instead of the host's (n_a - 1) / 2 + t_a.
template <bool VEC>
__global__ __launch_bounds__(BLK) void warp3_kernel(const float* __restrict__ img_in, float* __restrict__ img_out,
                                                    const int64_t* __restrict__ lab_in, int64_t* __restrict__ lab_out,
                                                    const float* __restrict__ field, const int32_t* __restrict__ start, int C, WarpMap m,
                                                    int WQ, int img_zeros, int lab_zeros, int64_t total) {
    const int64_t q = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (q >= total) return;
    const int64_t r = q / WQ;
    const int w0 = (int)(q - r * WQ) * VW, oh = (int)(r % m.no[1]), od = (int)(r / m.no[1]);
    const int Wo = m.no[2];
    const int64_t Vo = (int64_t)m.no[0] * m.no[1] * Wo, Vi = (int64_t)m.n[0] * m.n[1] * m.n[2];
    const int64_t orow = ((int64_t)od * m.no[1] + oh) * Wo + w0;
    float u[3][VW] = {};
    if (field) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float* f = field + a * Vo + orow;
            if constexpr (VEC) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(f);
#pragma unroll
                for (int j = 0; j < VW; j++) u[a][j] = v[j];
            } else {
#pragma unroll
                for (int j = 0; j < VW; j++)
                    if (w0 + j < Wo) u[a][j] = f[j];
            }
        }
    }
    double off[3] = {m.off[0], m.off[1], m.off[2]};
    if (start) {
#pragma clang fp contract(off)
#pragma unroll
        for (int a = 0; a < 3; a++) off[a] = ((double)start[a] + m.half_o[a]) + m.t[a];
    }
    Site st[VW];
#pragma unroll
    for (int j = 0; j < VW; j++) st[j] = site_of(m, off, od, oh, w0 + j, u[0][j], u[1][j], u[2][j], field != nullptr);
    for (int c = 0; c < C; c++) {
        if (lab_in) {
            const int64_t* src = lab_in + c * Vi;
            int64_t* dst = lab_out + c * Vo + orow;
            int64_t v[VW];
#pragma unroll
            for (int j = 0; j < VW; j++) v[j] = (VEC || w0 + j < Wo) && !(lab_zeros && st[j].outside) ? src[st[j].lab] : 0;
            if constexpr (VEC) {
                longlong2 a, b;
                a.x = v[0]; a.y = v[1]; b.x = v[2]; b.y = v[3];
                *reinterpret_cast<longlong2*>(dst) = a;
                *reinterpret_cast<longlong2*>(dst + 2) = b;
            } else {
#pragma unroll
                for (int j = 0; j < VW; j++)
                    if (w0 + j < Wo) dst[j] = v[j];
            }
        }
        if (img_in) {
            const float* src = img_in + c * Vi;
            float* dst = img_out + c * Vo + orow;
            f32x4 v;
#pragma unroll
            for (int j = 0; j < VW; j++) v[j] = (VEC || w0 + j < Wo) && !(img_zeros && st[j].outside) ? trilinear(src, m, st[j]) : 0.f;
            if constexpr (VEC) {
                *reinterpret_cast<f32x4*>(dst) = v;
            } else {
#pragma unroll
                for (int j = 0; j < VW; j++)
                    if (w0 + j < Wo) dst[j] = v[j];
            }
        }
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned blocks_of(int64_t total, int per) { return (unsigned)((total + per - 1) / per); }
inline bool fits_i32(int64_t a, int64_t b, int64_t c, int64_t d) { return a * b <= INT32_MAX && c * d <= INT32_MAX && a * b * (c * d) <= INT32_MAX; }
}  // namespace

size_t elastic_ws_bytes(int D, int H, int W) {
    if (D < 1 || H < 1 || W < 1) return 0;
    return (size_t)3 * D * H * W * sizeof(float);
}

int elastic_field(float* field, int D, int H, int W, uint64_t seed, const double* taps, int radius, void* ws, size_t ws_bytes,
                  hipStream_t s) {
    MI3D_CHECK_ARG(field && taps && ws, "mi3d_elastic_field: null field, taps or workspace");
    MI3D_CHECK_ARG(D >= 1 && H >= 1 && W >= 1, "mi3d_elastic_field: sizes must be positive, got (%d, %d, %d)", D, H, W);
    MI3D_CHECK_ARG(fits_i32(3, D, H, W), "mi3d_elastic_field: more than 2^31 - 1 field values");
    MI3D_CHECK_ARG(radius >= 0 && radius <= MAXR, "mi3d_elastic_field: tap radius %d is outside 0..%d (MI3D_ELASTIC_MAX_RADIUS)", radius,
                   MAXR);
    MI3D_CHECK_ARG(ws_bytes >= elastic_ws_bytes(D, H, W) && al16(ws), "mi3d_elastic_field: workspace too small or not 16-byte aligned");
    MI3D_CHECK_ARG((void*)field != ws, "mi3d_elastic_field: field and workspace alias");
    TapTable tp = {};
    tp.R = radius;
    for (int j = 0; j <= 2 * radius; j++) tp.g[j] = taps[j];
    float* tmp = (float*)ws;
    const int64_t total = (int64_t)3 * D * H * W;
    const int nchunk = (W + FW - 1) / FW;
    const int64_t items = (int64_t)3 * D * H * nchunk;
    field_w_kernel<<<blocks_of(items, BLK / 64), BLK, 0, s>>>(field, W, mix64a(seed), tp, nchunk, items);
    MI3D_LAUNCH_CHECK();
    field_axis_kernel<true><<<blocks_of(total, BLK), BLK, 0, s>>>(field, tmp, D, H, W, tp, total);
    MI3D_LAUNCH_CHECK();
    field_axis_kernel<false><<<blocks_of(total, BLK), BLK, 0, s>>>(tmp, field, D, H, W, tp, total);
    MI3D_LAUNCH_CHECK();
    return 0;
}

int warp3(const float* img_in, float* img_out, const int64_t* lab_in, int64_t* lab_out, int C, int D, int H, int W, int Do, int Ho,
          int Wo, const double* matrix, const double* translate, const float* field, double magnitude, int image_padding,
          int label_padding, const int32_t* start, hipStream_t s) {
    MI3D_CHECK_ARG(matrix && translate, "mi3d_warp3: null matrix or translation");
    MI3D_CHECK_ARG(!img_in == !img_out && !lab_in == !lab_out && (img_in || lab_in),
                   "mi3d_warp3: the image pair, the label pair or both, each with its input AND its output");
    MI3D_CHECK_ARG((!img_in || img_in != img_out) && (!lab_in || lab_in != lab_out), "mi3d_warp3: input and output alias");
    MI3D_CHECK_ARG(C >= 1 && D >= 1 && H >= 1 && W >= 1 && Do >= 1 && Ho >= 1 && Wo >= 1,
                   "mi3d_warp3: sizes must be positive, got (%d, %d, %d, %d) -> (%d, %d, %d)", C, D, H, W, Do, Ho, Wo);
    MI3D_CHECK_ARG(fits_i32(C, D, H, W) && fits_i32(C, Do, Ho, Wo) && fits_i32(3, Do, Ho, Wo), "mi3d_warp3: more than 2^31 - 1 voxels");
    MI3D_CHECK_ARG((image_padding == MI3D_PAD_BORDER || image_padding == MI3D_PAD_ZEROS) &&
                       (label_padding == MI3D_PAD_BORDER || label_padding == MI3D_PAD_ZEROS),
                   "mi3d_warp3: padding modes (%d, %d) are not MI3D_PAD_BORDER or MI3D_PAD_ZEROS", image_padding, label_padding);
    WarpMap m;
    const int n[3] = {D, H, W}, no[3] = {Do, Ho, Wo};
    for (int i = 0; i < 9; i++) m.m[i] = matrix[i];
    for (int a = 0; a < 3; a++) {
        m.n[a] = n[a];
        m.no[a] = no[a];
        m.half_o[a] = (double)(no[a] - 1) / 2.0;
        m.off[a] = (double)(n[a] - 1) / 2.0 + translate[a];
        m.t[a] = translate[a];
    }
    m.mag = magnitude;
    const int WQ = (Wo + VW - 1) / VW;
    const int64_t total = (int64_t)Do * Ho * WQ;
    const bool vec = Wo % VW == 0 && al16(img_out) && al16(lab_out) && al16(field);
    if (vec)
        warp3_kernel<true><<<blocks_of(total, BLK), BLK, 0, s>>>(img_in, img_out, lab_in, lab_out, field, start, C, m, WQ,
                                                                  image_padding == MI3D_PAD_ZEROS, label_padding == MI3D_PAD_ZEROS, total);
    else
        warp3_kernel<false><<<blocks_of(total, BLK), BLK, 0, s>>>(img_in, img_out, lab_in, lab_out, field, start, C, m, WQ,
                                                                   image_padding == MI3D_PAD_ZEROS, label_padding == MI3D_PAD_ZEROS, total);
    MI3D_LAUNCH_CHECK();
    return 0;
}

extern "C" {
size_t mi3d_elastic_workspace_bytes(int D, int H, int W) { return elastic_ws_bytes(D, H, W); }

int mi3d_elastic_field(float* field, int D, int H, int W, uint64_t seed, const double* taps, int radius, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return elastic_field(field, D, H, W, seed, taps, radius, workspace, workspace_bytes, (hipStream_t)stream);
}

int mi3d_warp3(const float* img_in, float* img_out, const int64_t* lab_in, int64_t* lab_out, int C, int D, int H, int W, int Do, int Ho,
               int Wo, const double* matrix, const double* translate, const float* field, double magnitude, int image_padding,
               int label_padding, void* stream) {
    return mi3d_warp3_at(img_in, img_out, lab_in, lab_out, C, D, H, W, Do, Ho, Wo, matrix, translate, field, magnitude, image_padding,
                         label_padding, nullptr, stream);
}

int mi3d_warp3_at(const float* img_in, float* img_out, const int64_t* lab_in, int64_t* lab_out, int C, int D, int H, int W, int Do,
                  int Ho, int Wo, const double* matrix, const double* translate, const float* field, double magnitude,
                  int image_padding, int label_padding, const int32_t* start, void* stream) {
    return warp3(img_in, img_out, lab_in, lab_out, C, D, H, W, Do, Ho, Wo, matrix, translate, field, magnitude, image_padding,
                 label_padding, start, (hipStream_t)stream);
}
}  // extern "C"
