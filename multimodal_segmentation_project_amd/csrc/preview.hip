// preview.hip — the preview figure of the reference's test loop, on the GPU: what visualize_prediction (test_model.py:66-193)
// and the slider of visualize_nifti.py:29-52 compute from whole host copies of the image, the label and the prediction.
//   foreground_profiles  np.sum(label > 0, axis=others) for all three axes in one read (find_best_slice, test_model.py:75-82)
//   best_slices          np.argmax of each profile, n // 2 where the maximum is 0 (test_model.py:85-89)
//   slice_minmax         overlay.min() / overlay.max() of a slice (test_model.py:110), per slice
//   overlay_render       create_overlay (test_model.py:103-125 = visualize_nifti.py:29-52) and np.rot90 per output pixel
// Volumes are dense 3-D arrays seen through element strides, as in resample.hip.  The two kernels that read a whole volume
// (profiles, the stack's min/max along the stored-fastest axis) walk it in memory order: the launcher sorts the axes by stride
// into F (fastest), M, S, whichever logical axes those are.  The render kernel reads the sources through signed 2-D views, so
// np.rot90 costs nothing, and lays its lanes along whichever of the output's two axes the image is stored faster in.
// Everything accumulated across workgroups is an integer or a min/max: atomics in any order give the same bits.
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "volume.h"

namespace {
constexpr int BLK = 256, NW = BLK / 64;
constexpr int TARGET_BLOCKS = 1024;  // four workgroups per CU: where a launcher may choose, it makes about this many
typedef unsigned long long u64;

struct Dims {
    int n[3];
    bool ok() const { return sides_ok(n[0], n[1], n[2]); }          // a slice index rides in gridDim.y
};
struct Strides {
    int64_t s[3];
    bool ok() const { return strides_ok(s[0], s[1], s[2]); }
};

// the three axes by increasing stride, an axis of one element last among equals: o[0] = F, o[1] = M, o[2] = S
void sort_axes(Dims n, Strides st, int (&o)[3]) {
    o[0] = 0, o[1] = 1, o[2] = 2;
    auto before = [&](int x, int y) { return (n.n[x] > 1) != (n.n[y] > 1) ? n.n[x] > 1 : st.s[x] < st.s[y]; };
    if (before(o[1], o[0])) std::swap(o[0], o[1]);
    if (before(o[2], o[1])) std::swap(o[1], o[2]);
    if (before(o[1], o[0])) std::swap(o[0], o[1]);
}

// ---- foreground profiles ----------------------------------------------------------------------------------------------------
// One workgroup reads MT rows (along M) of one F chunk in SG consecutive S slices.  A wave's 64 lanes are LF lanes along F (V
// elements each, one 16-byte load where V > 1) times LM = 64 / LF rows, so a short row still fills the wave; ITER row groups per
// wave are loaded before any is counted.  Counts along F: V register columns per lane, kept over all SG slices, then summed over
// the lanes that share a column (shuffles over the LM rows, LDS atomics over the waves).  Counts along M: a popcount per lane,
// summed over the row's LF lanes by shuffles and kept over the slices in the row's own LDS word.  Count of an S slice: the wave
// sums, one LDS word per slice.  At the end one 64-bit integer global atomic per non-zero LDS counter: the more slices a
// workgroup walks, the fewer atomics meet on one address (a 512 x 512 x 100 C-ordered label has only 100 F counters).
constexpr int ITER = 4;
constexpr int COLS = 64 * 16;                 // LF * V <= 64 lanes * 16 bytes
constexpr int ROWS = NW * 64 * ITER;          // MT <= NW * LM * ITER, LM <= 64
constexpr int MAX_SG = 64;

template <typename T, int V>
__global__ __launch_bounds__(BLK) void foreground_profiles_kernel(const T* __restrict__ lab, u64* __restrict__ cS, u64* __restrict__ cM,
                                                                  u64* __restrict__ cF, int nS, int nM, int nF, int64_t sS, int64_t sM,
                                                                  int64_t sF, int lgLF, int fChunks, int SG) {
    __shared__ int colcnt[COLS], rowcnt[ROWS], total[MAX_SG];
    const int LF = 1 << lgLF, LM = 64 >> lgLF, MT = NW * LM * ITER;
    for (int t = threadIdx.x; t < LF * V; t += BLK) colcnt[t] = 0;
    for (int t = threadIdx.x; t < MT; t += BLK) rowcnt[t] = 0;
    if (threadIdx.x < MAX_SG) total[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lf = lane & (LF - 1), lm = lane >> lgLF;
    const int mt = blockIdx.x / fChunks, fc = blockIdx.x - mt * fChunks;
    const int s0 = blockIdx.y * SG, s1 = min(s0 + SG, nS);
    const int m0 = mt * MT, f0 = (fc * LF + lf) * V;
    int col[V];
#pragma unroll
    for (int j = 0; j < V; j++) col[j] = 0;
    for (int s = s0; s < s1; s++) {
        const T* base = lab + (s * sS + f0 * sF);
        T vals[ITER][V];
#pragma unroll
        for (int it = 0; it < ITER; it++) {
            const int m = m0 + (it * NW + wave) * LM + lm;
#pragma unroll
            for (int j = 0; j < V; j++) vals[it][j] = 0;
            if (m < nM && f0 < nF) {           // V > 1: the launcher saw nF % V == 0 and 16-byte aligned rows
                if constexpr (V > 1) {
                    const uint4 q = *reinterpret_cast<const uint4*>(base + m * sM);
                    __builtin_memcpy(&vals[it][0], &q, 16);
                } else {
                    vals[it][0] = base[m * sM];
                }
            }
        }
        int mine = 0;
#pragma unroll
        for (int it = 0; it < ITER; it++) {
            int c = 0;
#pragma unroll
            for (int j = 0; j < V; j++) {
                const int fg = vals[it][j] > (T)0;
                col[j] += fg, c += fg;
            }
            mine += c;
            for (int off = 1; off < LF; off <<= 1) c += __shfl_xor(c, off, 64);
            if (lf == 0 && c) rowcnt[(it * NW + wave) * LM + lm] += c;      // one owner per row of the tile, the same in every slice
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
        if (lane == 0 && mine) atomicAdd(&total[s - s0], mine);
    }
    for (int off = LF; off < 64; off <<= 1) {
#pragma unroll
        for (int j = 0; j < V; j++) col[j] += __shfl_xor(col[j], off, 64);
    }
    if (lm == 0) {
#pragma unroll
        for (int j = 0; j < V; j++)
            if (col[j]) atomicAdd(&colcnt[lf * V + j], col[j]);
    }
    __syncthreads();
    const int fb = fc * LF * V;
    for (int t = threadIdx.x; t < LF * V; t += BLK)
        if (fb + t < nF && colcnt[t]) atomicAdd(cF + fb + t, (u64)colcnt[t]);
    for (int t = threadIdx.x; t < MT; t += BLK)
        if (m0 + t < nM && rowcnt[t]) atomicAdd(cM + m0 + t, (u64)rowcnt[t]);
    if (threadIdx.x < s1 - s0 && total[threadIdx.x]) atomicAdd(cS + s0 + threadIdx.x, (u64)total[threadIdx.x]);
}

// np.argmax + the n // 2 fallback; one workgroup per axis.  Candidates are ordered (count descending, index ascending), a total
// order, so the reduction tree's shape does not matter.
__global__ __launch_bounds__(BLK) void best_slices_kernel(const int64_t* __restrict__ counts, int nD, int nH, int nW,
                                                          int32_t* __restrict__ best) {
    __shared__ int64_t bc[NW];
    __shared__ int bi[NW];
    const int a = blockIdx.x, n = a == 0 ? nD : a == 1 ? nH : nW;
    const int64_t* c = counts + (a == 0 ? 0 : a == 1 ? nD : nD + nH);
    int64_t mc = -1;
    int mi = 0;
    for (int i = threadIdx.x; i < n; i += BLK) {
        const int64_t v = c[i];
        if (v > mc) mc = v, mi = i;          // ascending i: the first maximum of this thread's indices
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t oc = __shfl_xor(mc, off, 64);
        const int oi = __shfl_xor(mi, off, 64);
        if (oc > mc || (oc == mc && oi < mi)) mc = oc, mi = oi;
    }
    if ((threadIdx.x & 63) == 0) bc[threadIdx.x >> 6] = mc, bi[threadIdx.x >> 6] = mi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NW; w++)
            if (bc[w] > mc || (bc[w] == mc && bi[w] < mi)) mc = bc[w], mi = bi[w];
        best[a] = mc > 0 ? mi : n / 2;
    }
}

// ---- per-slice minimum and maximum ---------------------------------------------------------------------------------------------
// A slice's pair lives in two 32-bit keys that a ZEROED word already holds the identity of: key(v) maps the float order onto the
// unsigned order and is never 0 for a finite v; word 0 takes atomicMax(key(max)), word 1 atomicMax(~key(min)).
__device__ __forceinline__ uint32_t order_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ float image_at(const void* img, int code, int64_t off) {
    return code == MI3D_SRC_F32 ? static_cast<const float*>(img)[off] : (float)static_cast<const int16_t*>(img)[off];
}

// workgroup minimum / maximum -> the slot's two keys (thread 0); every thread of the workgroup calls it
__device__ __forceinline__ void block_minmax_to_keys(float mn, float mx, uint32_t* keys) {
    __shared__ float smn[NW], smx[NW];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float a = __shfl_xor(mn, off, 64), b = __shfl_xor(mx, off, 64);
        mn = a < mn ? a : mn, mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) smn[threadIdx.x >> 6] = mn, smx[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NW; w++) mn = smn[w] < mn ? smn[w] : mn, mx = smx[w] > mx ? smx[w] : mx;
        atomicMax(keys, order_key(mx));
        atomicMax(keys + 1, ~order_key(mn));
    }
}

// The plane of one slice: `outer` rows of `inner` elements, inner the remaining axis with the smaller stride.
struct Plane {
    int axis, n, inner, outer;          // the sliced axis, its side, the plane's sides
    int64_t sk, si, so;                 // element strides of the slice index, of inner, of outer
};
struct Planes {
    Plane p[3];
};
constexpr int PER = 8;                  // elements per thread of the plane kernel

// mode MI3D_PREVIEW_STACK: slot y = slice y of p[0].axis; MI3D_PREVIEW_ONE: the slice index[0] (or k) of p[0].axis, slot 0;
// MI3D_PREVIEW_THREE: y = axis, its slice index[y], slot y.  An index from device memory is clamped to the axis.
__device__ __forceinline__ int slice_of(int mode, int y, const int32_t* index, int k, int n) {
    const int v = mode == MI3D_PREVIEW_STACK ? y : index ? index[mode == MI3D_PREVIEW_THREE ? y : 0] : k;
    return min(max(v, 0), n - 1);
}

__global__ __launch_bounds__(BLK) void slice_minmax_plane_kernel(const void* __restrict__ img, int code, Planes pl, int mode,
                                                                 const int32_t* __restrict__ index, int k, uint32_t* __restrict__ keys) {
    const Plane p = pl.p[mode == MI3D_PREVIEW_THREE ? blockIdx.y : 0];
    const int64_t cells = (int64_t)p.inner * p.outer, q0 = (int64_t)blockIdx.x * (BLK * PER) + threadIdx.x;
    if ((int64_t)blockIdx.x * (BLK * PER) >= cells) return;          // the grid is sized for the largest of three planes
    const int64_t base = slice_of(mode, blockIdx.y, index, k, p.n) * p.sk;
    float v[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int64_t qq = min(q0 + j * BLK, cells - 1);          // past the slice's end: its last cell again
        const int64_t o = qq / p.inner, i = qq - o * p.inner;
        v[j] = image_at(img, code, base + o * p.so + i * p.si);
    }
    float mn = v[0], mx = v[0];
#pragma unroll
    for (int j = 1; j < PER; j++) mn = v[j] < mn ? v[j] : mn, mx = v[j] > mx ? v[j] : mx;
    block_minmax_to_keys(mn, mx, keys + 2 * blockIdx.y);
}

// The stack along the stored-fastest axis: a wave's lanes lie along F and every lane keeps the pair of ITS slice in registers.  A
// workgroup takes `rpb` rows (row s * nM + m is the F line of (s, m)), its four waves every fourth of them, LUN loads in flight
// per lane; the waves meet in LDS and the workgroup adds two atomics per slice of its chunk.
constexpr int LUN = 4;
__global__ __launch_bounds__(BLK) void slice_minmax_lane_kernel(const void* __restrict__ img, int code, int nF, int nM, int64_t rows,
                                                                int rpb, int64_t sF, int64_t sM, int64_t sS, uint32_t* __restrict__ keys) {
    __shared__ float smn[NW][64], smx[NW][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.x * 64 + lane;
    const int64_t r0 = (int64_t)blockIdx.y * rpb, r1 = min(r0 + rpb, rows);
    const int64_t col = min(f, nF - 1) * sF;          // a lane past the end reads the last slice and publishes nothing
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t r = r0 + wave; r < r1; r += NW * LUN) {
        float v[LUN];
#pragma unroll
        for (int u = 0; u < LUN; u++) {
            const int64_t rr = min(r + u * NW, r1 - 1);          // past the chunk's end: its last row again
            const int64_t si = rr / nM, mi = rr - si * nM;
            v[u] = image_at(img, code, col + si * sS + mi * sM);
        }
#pragma unroll
        for (int u = 0; u < LUN; u++) mn = v[u] < mn ? v[u] : mn, mx = v[u] > mx ? v[u] : mx;
    }
    smn[wave][lane] = mn, smx[wave][lane] = mx;
    __syncthreads();
    if (wave == 0 && f < nF) {          // wave 0 has read row r0, so the pair is finite
        for (int w = 1; w < NW; w++) mn = smn[w][lane] < mn ? smn[w][lane] : mn, mx = smx[w][lane] > mx ? smx[w][lane] : mx;
        atomicMax(keys + 2 * f, order_key(mx));
        atomicMax(keys + 2 * f + 1, ~order_key(mn));
    }
}

// ---- overlay render ----------------------------------------------------------------------------------------------------------------
// create_overlay for one pixel, in IEEE double, every operation rounded on its own (a subtraction, a subtraction, a division:
// nothing to contract): grey (v - min) / (max - min) of the slice's own pair, 0 / 0 = NaN on a flat slice, overwritten by the
// colour of label 1, 2 or 3 (test_model.py:110-123); any other label keeps the grey.
__device__ __forceinline__ void overlay_pixel(double v, int64_t label, double mn, double mx, double (&rgb)[3]) {
    const double g = (v - mn) / (mx - mn);
    rgb[0] = rgb[1] = rgb[2] = g;
    if (label == 1) rgb[0] = 1.0, rgb[1] = 0.0, rgb[2] = 0.0;
    if (label == 2) rgb[0] = 1.0, rgb[1] = 0.65, rgb[2] = 0.0;
    if (label == 3) rgb[0] = 0.0, rgb[1] = 0.5, rgb[2] = 0.0;
}
// float64: the reference's bits; float32: one rounding of them; uint8: (255 * value).astype(np.uint8), truncation, NaN -> 0
template <typename O> __device__ __forceinline__ O overlay_cast(double x) {
    if constexpr (std::is_same<O, uint8_t>::value) {
        const double t = 255.0 * x;
        return t != t ? (uint8_t)0 : (uint8_t)(int)t;
    } else {
        return (O)x;
    }
}
__device__ __forceinline__ int64_t label_at(const void* lab, int code, int64_t off) {
    return code == MI3D_SRC_I64 ? static_cast<const int64_t*>(lab)[off] : (int64_t)static_cast<const uint8_t*>(lab)[off];
}

// Output pixel (r, c) of slice k reads source element k * sk + base + r * sr + c * sc: sr / sc are the strides of the slice's two
// axes, or for np.rot90 (out[i][j] = slice[j][B - 1 - i]) sc = stride of the slice's first axis, sr = -stride of its second and
// base = (B - 1) * that stride.
struct View {
    int64_t sk, base, sr, sc;
};
struct Panel {                          // one launch row y: a slice of `axis` drawn as R x C pixels
    int axis, n, R, C;
    int by_rows;                        // consecutive lanes take consecutive r (the image is stored faster along r), else c groups
    View img, lab, prd;
    float* raw;                         // (R, C) float32 or null
    void* gt;                           // (R, C, 3), or for the stack (n, R, C, 3)
    void* pr;                           // (R, C, 3) from prd, or null
};
struct Panels {
    Panel p[3];
};

// G pixels = 48 bytes of output per thread.  VEC: the launcher saw C % G == 0 and 16-byte aligned outputs -> three 16-byte stores.
template <typename O, bool VEC>
__device__ __forceinline__ void store_pixels(O* out, const double (&rgb)[48 / (3 * sizeof(O))][3], int c0, int C) {
    constexpr int G = 48 / (3 * (int)sizeof(O));
    if constexpr (VEC) {
        O packed[3 * G];
#pragma unroll
        for (int j = 0; j < G; j++)
#pragma unroll
            for (int ch = 0; ch < 3; ch++) packed[3 * j + ch] = overlay_cast<O>(rgb[j][ch]);
        uint4 q[3];
        __builtin_memcpy(q, packed, 48);
#pragma unroll
        for (int t = 0; t < 3; t++) reinterpret_cast<uint4*>(out)[t] = q[t];
    } else {
#pragma unroll
        for (int j = 0; j < G; j++)
            if (c0 + j < C)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) out[3 * j + ch] = overlay_cast<O>(rgb[j][ch]);
    }
}

// grid: x over (r, group of G pixels along c), y = launch row (a slice of the stack, or a view of the panel set)
template <typename O, bool VEC>
__global__ __launch_bounds__(BLK) void overlay_render_kernel(const void* __restrict__ img, int img_code, const void* __restrict__ lab,
                                                             int lab_code, const void* __restrict__ prd, int prd_code, Panels ps, int mode,
                                                             const int32_t* __restrict__ index, int k, const uint32_t* __restrict__ keys) {
    constexpr int G = 48 / (3 * (int)sizeof(O));
    const Panel p = ps.p[mode == MI3D_PREVIEW_THREE ? blockIdx.y : 0];
    const int CG = (p.C + G - 1) / G;
    const int64_t q = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (q >= (int64_t)p.R * CG) return;
    // by_rows: each of a thread's G loads is coalesced across the wave and its 48 output bytes lie a row apart from its
    // neighbours'; otherwise the stores are coalesced and the loads are G elements of one source row.  Same pixels, same bits.
    const int r = p.by_rows ? (int)(q % p.R) : (int)(q / CG);
    const int c0 = (p.by_rows ? (int)(q / p.R) : (int)(q - (int64_t)r * CG)) * G;
    const int ks = slice_of(mode, blockIdx.y, index, k, p.n);
    const double mx = (double)key_value(keys[2 * blockIdx.y]), mn = (double)key_value(~keys[2 * blockIdx.y + 1]);
    const int64_t oi = ks * p.img.sk + p.img.base + r * p.img.sr, ol = ks * p.lab.sk + p.lab.base + r * p.lab.sr;
    const int64_t op = ks * p.prd.sk + p.prd.base + r * p.prd.sr;
    const int64_t pix = (mode == MI3D_PREVIEW_STACK ? (int64_t)blockIdx.y * p.R * p.C : 0) + (int64_t)r * p.C + c0;
    float v[G];
    double rgb[G][3];
#pragma unroll
    for (int j = 0; j < G; j++) {
        const int c = VEC ? c0 + j : min(c0 + j, p.C - 1);          // a lane past the row's end reads the last column, stores nothing
        v[j] = image_at(img, img_code, oi + c * p.img.sc);
        overlay_pixel((double)v[j], label_at(lab, lab_code, ol + c * p.lab.sc), mn, mx, rgb[j]);
    }
    store_pixels<O, VEC>(static_cast<O*>(p.gt) + 3 * pix, rgb, c0, p.C);
    if (p.raw) {
#pragma unroll
        for (int j = 0; j < G; j++)
            if (c0 + j < p.C) p.raw[pix + j] = v[j];
    }
    if (p.pr) {
#pragma unroll
        for (int j = 0; j < G; j++) {
            const int c = VEC ? c0 + j : min(c0 + j, p.C - 1);
            overlay_pixel((double)v[j], label_at(prd, prd_code, op + c * p.prd.sc), mn, mx, rgb[j]);
        }
        store_pixels<O, VEC>(static_cast<O*>(p.pr) + 3 * pix, rgb, c0, p.C);
    }
}

// The stack where the image is not stored fastest along the output's c: along the slice axis (a C-ordered volume sliced along its
// last axis) or along r (a Fortran-ordered scan sliced along its last).  Neighbouring pixels of an output row then lie far
// apart in the source, so a workgroup first loads a tile of KT positions of that fast axis X x CT pixels along c with its lanes
// along X (coalesced), parks image values and colour codes in LDS, and then writes CT pixels = 4 x 48 bytes for each of the KT
// positions with the per-pixel function above.  CT = 4 G: every thread loads G voxels and stores G pixels.  grid: x over (tile
// of X, tile of c), y = the third axis (r where X is the slice axis, the slice where X is r).
constexpr int KT = 64;
template <typename O, bool VEC>
__global__ __launch_bounds__(BLK) void overlay_stack_tile_kernel(const void* __restrict__ img, int img_code, const void* __restrict__ lab,
                                                                 int lab_code, Panel p, int x_is_r, int cTiles,
                                                                 const uint32_t* __restrict__ keys) {
    constexpr int G = 48 / (3 * (int)sizeof(O)), CT = 4 * G;
    __shared__ float simg[CT][KT + 1];
    __shared__ uint8_t slab[CT][KT + 4];          // the label where it is 1, 2 or 3, else 0: all the colour needs
    const int xt = blockIdx.x / cTiles, c00 = (blockIdx.x - xt * cTiles) * CT, x0 = xt * KT, y = blockIdx.y;
    const int nX = x_is_r ? p.R : p.n;
    {
        const int xx = threadIdx.x & (KT - 1), x = x0 + xx;
        const int k = x_is_r ? y : x, r = x_is_r ? x : y;
#pragma unroll
        for (int j = 0; j < G; j++) {
            const int cc = (threadIdx.x >> 6) + NW * j, c = c00 + cc;
            if (x < nX && c < p.C) {
                simg[cc][xx] = image_at(img, img_code, k * p.img.sk + p.img.base + r * p.img.sr + c * p.img.sc);
                const int64_t l = label_at(lab, lab_code, k * p.lab.sk + p.lab.base + r * p.lab.sr + c * p.lab.sc);
                slab[cc][xx] = l >= 1 && l <= 3 ? (uint8_t)l : (uint8_t)0;
            }
        }
    }
    __syncthreads();
    const int xx = threadIdx.x >> 2, x = x0 + xx, c0 = c00 + (threadIdx.x & 3) * G;
    if (x >= nX || c0 >= p.C) return;
    const int k = x_is_r ? y : x, r = x_is_r ? x : y;
    const double mx = (double)key_value(keys[2 * k]), mn = (double)key_value(~keys[2 * k + 1]);
    double rgb[G][3];
#pragma unroll
    for (int j = 0; j < G; j++) {
        const int cc = min(c0 + j, p.C - 1) - c00;          // past the row's end: the last column again, never stored
        overlay_pixel((double)simg[cc][xx], (int64_t)slab[cc][xx], mn, mx, rgb[j]);
    }
    store_pixels<O, VEC>(static_cast<O*>(p.gt) + 3 * (((int64_t)k * p.R + r) * p.C + c0), rgb, c0, p.C);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
int check_volume(const char* name, const void* p, Dims n, Strides st) {
    MI3D_CHECK_ARG(p, "%s: null pointer", name);
    MI3D_CHECK_ARG(n.ok(), "%s: sides must be in [1, %d]", name, MAX_SIDE);
    MI3D_CHECK_ARG(st.ok(), "%s: strides must be positive element counts", name);
    return 0;
}
int check_mode(const char* name, int axis, int mode, const int32_t* index, int k, Dims n) {
    MI3D_CHECK_ARG(mode == MI3D_PREVIEW_STACK || mode == MI3D_PREVIEW_ONE || mode == MI3D_PREVIEW_THREE, "%s: unknown mode %d", name, mode);
    if (mode == MI3D_PREVIEW_THREE) {
        MI3D_CHECK_ARG(index, "%s: the three slice indices are read from device memory", name);
        return 0;
    }
    MI3D_CHECK_ARG(axis >= 0 && axis <= 2, "%s: axis %d outside 0..2", name, axis);
    MI3D_CHECK_ARG(mode != MI3D_PREVIEW_ONE || index || (k >= 0 && k < n.n[axis]), "%s: slice %d outside the axis of %d", name, k,
                   n.n[axis]);
    return 0;
}

// the slice of `axis` as a 2-D array in the reference's order: its first axis a, its second axis b
void slice_axes(int axis, int& a, int& b) { a = axis == 0 ? 1 : 0, b = axis == 2 ? 1 : 2; }

Plane plane_of(int axis, Dims n, Strides st) {
    int a, b;
    slice_axes(axis, a, b);
    const bool a_inner = n.n[b] == 1 || (n.n[a] > 1 && st.s[a] < st.s[b]);
    const int in = a_inner ? a : b, out = a_inner ? b : a;
    return Plane{axis, n.n[axis], n.n[in], n.n[out], st.s[axis], st.s[in], st.s[out]};
}

View view_of(int axis, Dims n, Strides st, int rot90) {
    int a, b;
    slice_axes(axis, a, b);
    if (rot90) return View{st.s[axis], (int64_t)(n.n[b] - 1) * st.s[b], -st.s[b], st.s[a]};
    return View{st.s[axis], 0, st.s[a], st.s[b]};
}

// the launcher of mi3d_slice_minmax
int slice_minmax_launch(const char* name, const void* image, int image_dtype, int D, int H, int W, int64_t stride_d,
                        int64_t stride_h, int64_t stride_w, int axis, int mode, const int32_t* index, int k, uint32_t* keys,
                        void* stream) {
    const Dims n{{D, H, W}};
    const Strides st{{stride_d, stride_h, stride_w}};
    MI3D_TRY(check_volume(name, image, n, st));
    MI3D_CHECK_ARG(keys && ((uintptr_t)keys & 3) == 0, "%s: keys must be a 4-byte aligned device pointer", name);
    MI3D_CHECK_ARG(image_dtype == MI3D_SRC_F32 || image_dtype == MI3D_SRC_I16, "%s: the image is float32 or int16, not dtype code %d", name,
                   image_dtype);
    MI3D_TRY(check_mode(name, axis, mode, index, k, n));
    int o[3];
    sort_axes(n, st, o);
    if (mode == MI3D_PREVIEW_STACK && axis == o[0] && n.n[axis] > 1) {
        const int F = o[0], M = o[1], S = o[2];
        const int64_t rows = (int64_t)n.n[M] * n.n[S], chunks = (n.n[F] + 63) / 64;
        const int64_t want = std::max<int64_t>(NW * LUN, (rows * chunks + TARGET_BLOCKS - 1) / TARGET_BLOCKS);
        const int rpb = (int)((want + NW * LUN - 1) / (NW * LUN)) * (NW * LUN);
        dim3 grid((unsigned)chunks, (unsigned)((rows + rpb - 1) / rpb));
        slice_minmax_lane_kernel<<<grid, BLK, 0, (hipStream_t)stream>>>(image, image_dtype, n.n[F], n.n[M], rows, rpb, st.s[F], st.s[M],
                                                                        st.s[S], keys);
        MI3D_LAUNCH_CHECK();
        return 0;
    }
    Planes pl;
    int64_t cells = 0;
    for (int j = 0; j < 3; j++) {
        pl.p[j] = plane_of(mode == MI3D_PREVIEW_THREE ? j : axis, n, st);
        if (mode == MI3D_PREVIEW_THREE || j == 0) cells = std::max(cells, (int64_t)pl.p[j].inner * pl.p[j].outer);
    }
    const unsigned rows = mode == MI3D_PREVIEW_STACK ? (unsigned)n.n[axis] : mode == MI3D_PREVIEW_THREE ? 3u : 1u;
    dim3 grid((unsigned)((cells + BLK * PER - 1) / (BLK * PER)), rows);
    slice_minmax_plane_kernel<<<grid, BLK, 0, (hipStream_t)stream>>>(image, image_dtype, pl, mode, index, k, keys);
    MI3D_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" {

size_t mi3d_preview_workspace_bytes(int D, int H, int W) {
    if (!Dims{{D, H, W}}.ok()) {
        mi3d_set_error("mi3d_preview_workspace_bytes: sides must be in [1, %d]", MAX_SIDE);
        return 0;
    }
    const size_t side = (size_t)(D > H ? (D > W ? D : W) : (H > W ? H : W));
    return (((size_t)(D + H + W) * 8 + 16 + side * 8) + 255) & ~(size_t)255;
}

int mi3d_foreground_profiles(const void* label, int label_dtype, int D, int H, int W, int64_t stride_d, int64_t stride_h,
                             int64_t stride_w, int64_t* counts, void* stream) {
    const char* name = "mi3d_foreground_profiles";
    const Dims n{{D, H, W}};
    const Strides st{{stride_d, stride_h, stride_w}};
    MI3D_TRY(check_volume(name, label, n, st));
    MI3D_CHECK_ARG(counts && ((uintptr_t)counts & 7) == 0, "%s: counts must be an 8-byte aligned device pointer", name);
    MI3D_CHECK_ARG(label_dtype == MI3D_SRC_U8 || label_dtype == MI3D_SRC_I64, "%s: labels are uint8 or int64, not dtype code %d", name,
                   label_dtype);
    int o[3];
    sort_axes(n, st, o);
    const int F = o[0], M = o[1], S = o[2];
    const int nF = n.n[F], nM = n.n[M], nS = n.n[S];
    const int64_t sF = nF > 1 ? st.s[F] : 1, sM = st.s[M], sS = st.s[S];
    u64* c[3] = {(u64*)counts, (u64*)counts + D, (u64*)counts + D + H};
    const int esz = label_dtype == MI3D_SRC_U8 ? 1 : 8, VV = 16 / esz;
    const bool vec = sF == 1 && nF % VV == 0 && aligned16(label) && (nM == 1 || sM * esz % 16 == 0) && (nS == 1 || sS * esz % 16 == 0);
    const int V = vec ? VV : 1, lanes = (nF + V - 1) / V;
    int lgLF = 0;
    while (lgLF < 6 && (1 << lgLF) < lanes) lgLF++;
    const int LF = 1 << lgLF, MT = NW * (64 >> lgLF) * ITER;
    const int fChunks = (lanes + LF - 1) / LF, mTiles = (nM + MT - 1) / MT;
    MI3D_CHECK_ARG((int64_t)fChunks * mTiles < (int64_t)1 << 31, "%s: plane too large", name);
    // slices per workgroup: as many as leave about four workgroups per CU, at most MAX_SG
    const int64_t groups = std::min<int64_t>(nS, std::max<int64_t>((TARGET_BLOCKS + (int64_t)fChunks * mTiles - 1) / ((int64_t)fChunks * mTiles),
                                                                  (nS + MAX_SG - 1) / MAX_SG));
    const int SG = (int)((nS + groups - 1) / groups);
    dim3 grid((unsigned)(fChunks * mTiles), (unsigned)((nS + SG - 1) / SG));
    dispatch_src(label_dtype, LabelTypes(), [&](auto tag) {
        using T = decltype(tag);
        auto kernel = vec ? foreground_profiles_kernel<T, 16 / (int)sizeof(T)> : foreground_profiles_kernel<T, 1>;
        kernel<<<grid, BLK, 0, (hipStream_t)stream>>>((const T*)label, c[S], c[M], c[F], nS, nM, nF, sS, sM, sF, lgLF, fChunks, SG);
    });
    MI3D_LAUNCH_CHECK();
    return 0;
}

int mi3d_best_slices(const int64_t* counts, int D, int H, int W, int32_t* best, void* stream) {
    MI3D_CHECK_ARG(counts && best, "mi3d_best_slices: null pointer");
    MI3D_CHECK_ARG((Dims{{D, H, W}}.ok()), "mi3d_best_slices: sides must be in [1, %d]", MAX_SIDE);
    best_slices_kernel<<<3, BLK, 0, (hipStream_t)stream>>>(counts, D, H, W, best);
    MI3D_LAUNCH_CHECK();
    return 0;
}

int mi3d_slice_minmax(const void* image, int image_dtype, int D, int H, int W, int64_t stride_d, int64_t stride_h, int64_t stride_w,
                      int axis, int mode, const int32_t* index, int k, uint32_t* keys, void* stream) {
    return slice_minmax_launch("mi3d_slice_minmax", image, image_dtype, D, H, W, stride_d, stride_h, stride_w, axis, mode, index, k, keys,
                               stream);
}

int mi3d_overlay_render(const void* image, int image_dtype, const int64_t* image_strides, const void* label, int label_dtype,
                        const int64_t* label_strides, const void* pred, int pred_dtype, const int64_t* pred_strides, int D, int H, int W,
                        int axis, int mode, const int32_t* index, int k, int rot90, const uint32_t* keys, int out_dtype,
                        void* const* outs, void* stream) {
    const char* name = "mi3d_overlay_render";
    const Dims n{{D, H, W}};
    MI3D_CHECK_ARG(image_strides && label_strides && outs && keys, "%s: null pointer", name);
    const Strides si{{image_strides[0], image_strides[1], image_strides[2]}}, sl{{label_strides[0], label_strides[1], label_strides[2]}};
    MI3D_TRY(check_volume(name, image, n, si));
    MI3D_TRY(check_volume(name, label, n, sl));
    MI3D_CHECK_ARG(image_dtype == MI3D_SRC_F32 || image_dtype == MI3D_SRC_I16, "%s: the image is float32 or int16, not dtype code %d", name,
                   image_dtype);
    MI3D_CHECK_ARG(label_dtype == MI3D_SRC_U8 || label_dtype == MI3D_SRC_I64, "%s: labels are uint8 or int64, not dtype code %d", name,
                   label_dtype);
    MI3D_TRY(check_mode(name, axis, mode, index, k, n));
    MI3D_CHECK_ARG(out_dtype == MI3D_OVERLAY_F64 || out_dtype == MI3D_OVERLAY_F32 || out_dtype == MI3D_OVERLAY_U8,
                   "%s: unknown output dtype code %d", name, out_dtype);
    Strides sp = sl;
    if (mode == MI3D_PREVIEW_THREE) {
        MI3D_CHECK_ARG(pred_strides, "%s: the panel set needs a prediction", name);
        sp = Strides{{pred_strides[0], pred_strides[1], pred_strides[2]}};
        MI3D_TRY(check_volume(name, pred, n, sp));
        MI3D_CHECK_ARG(pred_dtype == MI3D_SRC_U8 || pred_dtype == MI3D_SRC_I64, "%s: predictions are uint8 or int64, not dtype code %d",
                       name, pred_dtype);
        MI3D_CHECK_ARG(rot90, "%s: the panel set is the rotated figure of test_model.py:127-179", name);
    } else {
        MI3D_CHECK_ARG(!pred, "%s: a prediction is drawn by the panel set only", name);
        pred = label, pred_dtype = label_dtype;
    }
    const int esz = out_dtype == MI3D_OVERLAY_F64 ? 8 : out_dtype == MI3D_OVERLAY_F32 ? 4 : 1, G = 16 / esz;
    const int views = mode == MI3D_PREVIEW_THREE ? 3 : 1;
    // figure order: row v = view of axis 2, 0, 1 (axial, sagittal, coronal); outs[3 v + {0, 1, 2}] = raw, ground truth, prediction.
    // Launch row y of the panel set is AXIS y (its keys and its index are slot y), so view v lands in p[axis of v].
    static const int view_axis[3] = {2, 0, 1};
    Panels ps{};
    bool vec = true;
    int64_t threads = 0;
    for (int v = 0; v < views; v++) {
        const int ax = views == 3 ? view_axis[v] : axis;
        int a, b;
        slice_axes(ax, a, b);
        Panel& p = ps.p[views == 3 ? ax : 0];
        p.axis = ax, p.n = n.n[ax];
        p.R = rot90 ? n.n[b] : n.n[a], p.C = rot90 ? n.n[a] : n.n[b];
        p.img = view_of(ax, n, si, rot90), p.lab = view_of(ax, n, sl, rot90), p.prd = view_of(ax, n, sp, rot90);
        if (views == 3) {
            p.raw = (float*)outs[3 * v], p.gt = outs[3 * v + 1], p.pr = outs[3 * v + 2];
            MI3D_CHECK_ARG(p.raw && p.gt && p.pr, "%s: null output", name);
            vec = vec && aligned16(p.pr);
        } else {
            p.gt = outs[0];
            MI3D_CHECK_ARG(p.gt, "%s: null output", name);
        }
        p.by_rows = p.R > 1 && std::llabs(p.img.sr) < std::llabs(p.img.sc);
        vec = vec && p.C % G == 0 && aligned16(p.gt);
        threads = std::max(threads, (int64_t)p.R * ((p.C + G - 1) / G));
    }
    MI3D_CHECK_ARG(threads < (int64_t)1 << 31, "%s: slice too large", name);
    if (mode == MI3D_PREVIEW_STACK) {
        // where does the image run fastest: along the slices, along r, or along c (then, or with no such axis, the kernel below)
        const Panel& p = ps.p[0];
        const int64_t big = (int64_t)1 << 62;
        const int64_t fk = p.n > 1 ? std::llabs(p.img.sk) : big, fr = p.R > 1 ? std::llabs(p.img.sr) : big;
        const int64_t fc = p.C > 1 ? std::llabs(p.img.sc) : big;
        if (std::min(fk, fr) < fc) {
            const int x_is_r = fr < fk, nX = x_is_r ? p.R : p.n, nY = x_is_r ? p.n : p.R;
            const int cTiles = (p.C + 4 * G - 1) / (4 * G), xTiles = (nX + KT - 1) / KT;
            MI3D_CHECK_ARG((int64_t)cTiles * xTiles < (int64_t)1 << 31, "%s: slice too large", name);
            dim3 tgrid((unsigned)(cTiles * xTiles), (unsigned)nY);
            auto tlaunch = [&](auto kernel) {
                kernel<<<tgrid, BLK, 0, (hipStream_t)stream>>>(image, image_dtype, label, label_dtype, p, x_is_r, cTiles, keys);
            };
            if (out_dtype == MI3D_OVERLAY_F64) tlaunch(vec ? overlay_stack_tile_kernel<double, true> : overlay_stack_tile_kernel<double, false>);
            else if (out_dtype == MI3D_OVERLAY_F32) tlaunch(vec ? overlay_stack_tile_kernel<float, true> : overlay_stack_tile_kernel<float, false>);
            else tlaunch(vec ? overlay_stack_tile_kernel<uint8_t, true> : overlay_stack_tile_kernel<uint8_t, false>);
            MI3D_LAUNCH_CHECK();
            return 0;
        }
    }
    const unsigned rows = mode == MI3D_PREVIEW_STACK ? (unsigned)n.n[axis] : (unsigned)views;
    dim3 grid((unsigned)((threads + BLK - 1) / BLK), rows);
    auto launch = [&](auto kernel) {
        kernel<<<grid, BLK, 0, (hipStream_t)stream>>>(image, image_dtype, label, label_dtype, pred, pred_dtype, ps, mode, index, k, keys);
    };
    if (out_dtype == MI3D_OVERLAY_F64) launch(vec ? overlay_render_kernel<double, true> : overlay_render_kernel<double, false>);
    else if (out_dtype == MI3D_OVERLAY_F32) launch(vec ? overlay_render_kernel<float, true> : overlay_render_kernel<float, false>);
    else launch(vec ? overlay_render_kernel<uint8_t, true> : overlay_render_kernel<uint8_t, false>);
    MI3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
