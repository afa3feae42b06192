// surface.hip — surface distances between two label maps: the exact Euclidean distance transform, and from it the Hausdorff
// distance, its percentile, the average symmetric surface distance and the surface Dice, per (sample, class); what a user does on
// the host with scipy.ndimage.binary_erosion and scipy.ndimage.distance_transform_edt(~F, sampling=spacing) per class and
// direction.  The reference computes no surface metric; scipy (the conventions of monai.metrics and medpy) is the contract.
//   surface pass   a voxel of a listed class with a neighbour outside the class or the volume     -> bytemap (class index + 1), counts
//   w pass         one wave per row, one ballot per 64 voxels, nearest feature by clz / ctz       -> g1 = fl((sw (w - w'))^2)
//   h pass, d pass one thread per voxel walks outwards along its line until the offset alone      -> g2, g3
//                  costs as much as the best candidate so far: min over h' of fl(g1[h'] + fl((sh (h - h'))^2))
//   query epilogue the d pass of mi3d_surface_distances runs at the other map's surface only and  -> compacted g3, max, counts
//                  leaves, per (sample, direction): the g3 values, their maximum, the counts within     within tolerance,
//                  each tolerance and per-workgroup sums of sqrt(g3) in fixed slots                      partial sums
//   select         one workgroup per (sample, direction): the partial sums in a fixed order, and a    -> table
//                  radix select (8 digits of 8 bits, histogram in LDS) of the two order statistics
//   signed maps    mi3d_signed_distance_maps: per (sample, listed class) the class mask and its inverse as the     -> phi, float32
//                  features of ONE sweep of the w and h passes (maps x 2 jobs); the last pass takes the d pass of
//                  the one direction a voxel needs, the root, the sign and the offset, and rounds to float32 once
// Everything in g is IEEE double with every operation rounded on its own (contraction is off in this file).  g3 is the
// minimum of the candidate expressions themselves, not the parabola a real-valued envelope picks: the outward walk of the h and d
// passes evaluates every candidate that can be smaller and stops at offset k only when fl((s k)^2) >= best; rounding is monotone
// and g >= 0, so fl(g + fl((s k')^2)) >= fl((s k)^2) >= best for every k' >= k: nothing skipped could have lowered the minimum.
// The walk is bounded by the line's length.  Near a feature it ends after about as many steps as the distance in voxels (the
// surfaces of a prediction and its target lie voxels apart); on a nearly empty mask it is the full O(L) per voxel.
// Non-negative doubles order as their bit patterns, so the maximum and the select use integer atomics only; the float sum goes
// through fixed slots and one fixed-order reduce: every output has the same bits on every run.  No workgroup waits on another and
// no loop is unbounded, so there is no status word.  Every launch is on the caller's stream, every buffer the caller's.
#include <cmath>

#include "volume.h"

#pragma clang fp contract(off)          // hipcc would fuse a product into the add that follows it

namespace {
constexpr int BLK = 256, NW = BLK / 64;
constexpr int MAXC = MI3D_COMPONENTS_MAX_CLASSES, MAXT = MI3D_SURFACE_MAX_TOLERANCES;
constexpr int COUNTS = MI3D_SURFACE_COUNT_COLUMNS, TABLE = MI3D_SURFACE_TABLE_COLUMNS;
typedef unsigned long long u64;

struct Tol {                         // fl(tau * tau) of every tolerance
    int n;
    double sq[MAXT];
};

__device__ __forceinline__ double inf() { return __longlong_as_double(0x7ff0000000000000ll); }
// fl(fl(s * k)^2): the squared offset of k voxels at spacing s
__device__ __forceinline__ double sq_offset(double s, int64_t k) {
    const double t = s * (double)k;
    return t * t;
}
__device__ __forceinline__ double min_nonneg(double a, double b) { return b < a ? b : a; }          // no NaN ever enters g

// ---- surface pass -----------------------------------------------------------------------------------------------------------------
// One thread per voxel.  out (N, V) bytes: j + 1 at a surface voxel of listed class j, else 0.  counts (may be NULL): the column of
// this map in the counts table, one integer atomic per (workgroup, class).  grid: x over voxels, y = sample.
template <typename T>
__global__ __launch_bounds__(BLK) void surface_kernel(const T* __restrict__ lab, Vol vol, Classes cl, int conn, uint8_t* __restrict__ out,
                                                      u64* __restrict__ counts) {
    __shared__ unsigned found[MAXC];
    if (threadIdx.x < MAXC) found[threadIdx.x] = 0;
    __syncthreads();
    const int64_t V = vol.V(), i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i < V) {
        lab += blockIdx.y * vol.sn;
        int d, h, w;
        vol.split(i, d, h, w);
        const int64_t v = (int64_t)lab[vol.offset(d, h, w)];
        const int c = class_index(cl, v);
        bool edge = false;
        if (c >= 0) {
            for (int o = 0; o < 27 && !edge; o++) {
                const int dd = o / 9 - 1, dh = o / 3 % 3 - 1, dw = o % 3 - 1, nz = nonzeros(dd, dh, dw);
                if (nz == 0 || nz > conn) continue;
                const int nd = d + dd, nh = h + dh, nw = w + dw;
                if (nd < 0 || nd >= vol.D || nh < 0 || nh >= vol.H || nw < 0 || nw >= vol.W)
                    edge = true;          // border_value = 0: outside the volume is outside the class
                else
                    edge = (int64_t)lab[vol.offset(nd, nh, nw)] != v;
            }
            if (edge) atomicAdd(&found[c], 1u);
        }
        out[blockIdx.y * V + i] = (uint8_t)(edge ? c + 1 : 0);
    }
    __syncthreads();
    if (counts && threadIdx.x < cl.n && found[threadIdx.x])
        atomicAdd(counts + ((int64_t)blockIdx.y * cl.n + threadIdx.x) * COUNTS, (u64)found[threadIdx.x]);
}

// the feature bytemap of mi3d_distance_transform: 1 where the mask is not 0
template <typename T>
__global__ __launch_bounds__(BLK) void nonzero_kernel(const T* __restrict__ mask, Vol vol, uint8_t* __restrict__ out) {
    const int64_t V = vol.V(), i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= V) return;
    int d, h, w;
    vol.split(i, d, h, w);
    out[blockIdx.y * V + i] = (uint8_t)(mask[blockIdx.y * vol.sn + vol.offset(d, h, w)] != 0);
}

// ---- w pass -----------------------------------------------------------------------------------------------------------------------
// One wave per row of W voxels, 64 at a time.  The input is binary, so g1 at w is the squared offset to the nearest feature of the
// row (the offset cost is monotone), +inf if the row has none.  Sweep 1 walks the words from the right and writes the cost to the
// nearest feature at or right of w; sweep 2 walks from the left and lowers it to the one at or left of w.  Within a word the
// nearest feature is a bit scan of the ballot; across words it is carried (wave-uniform).  A lane re-reads only what it wrote
// itself.  grid: x over rows / NW, y = sample, z = direction (feat0 / feat1).  g1 (jobs, V), job = sample * gridDim.z + z.
__global__ __launch_bounds__(BLK) void w_kernel(const uint8_t* __restrict__ feat0, const uint8_t* __restrict__ feat1, int match,
                                                int64_t rows, int W, double sw, double* __restrict__ g1) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * NW + (threadIdx.x >> 6);
    if (row >= rows) return;          // the whole wave leaves
    const int64_t V = rows * W, job = (int64_t)blockIdx.y * gridDim.z + blockIdx.z;
    const uint8_t* f = (blockIdx.z ? feat1 : feat0) + blockIdx.y * V + row * W;
    double* g = g1 + job * V + row * W;
    const int64_t words = ((int64_t)W + 63) / 64;
    int64_t carried = -1;
    for (int64_t k = words - 1; k >= 0; k--) {
        const int64_t w = k * 64 + lane;
        const u64 m = __ballot(w < W && f[w] == match);
        const u64 at_or_right = m & (~0ull << lane);
        const int64_t r = at_or_right ? k * 64 + __builtin_ctzll(at_or_right) : carried;
        if (w < W) g[w] = r < 0 ? inf() : sq_offset(sw, r - w);
        if (m) carried = k * 64 + __builtin_ctzll(m);
    }
    carried = -1;
    for (int64_t k = 0; k < words; k++) {
        const int64_t w = k * 64 + lane;
        const u64 m = __ballot(w < W && f[w] == match);
        const u64 at_or_left = m & (~0ull >> (63 - lane));
        const int64_t l = at_or_left ? k * 64 + 63 - __builtin_clzll(at_or_left) : carried;
        if (w < W && l >= 0) g[w] = min_nonneg(g[w], sq_offset(sw, w - l));
        if (m) carried = k * 64 + 63 - __builtin_clzll(m);
    }
}

// ---- h pass and d pass ------------------------------------------------------------------------------------------------------------
// out[x] = min over x' of fl(in[x'] + fl((s (x - x'))^2)) along one axis: `stride` elements between neighbours, L of them.  One
// thread per voxel, adjacent lanes on adjacent voxels of the innermost axis, so every load and store of a wave is one contiguous
// run; no transpose, no envelope to keep.  The walk and why it is exact: the head of the file.
__device__ __forceinline__ double line_min(const double* __restrict__ in, int64_t i, int64_t stride, int x, int L, double s) {
    double best = in[i];
    const int reach = x > L - 1 - x ? x : L - 1 - x;
    for (int k = 1; k <= reach; k++) {
        const double c = sq_offset(s, k);
        if (!(c < best)) break;
        if (k <= x) best = min_nonneg(best, in[i - k * stride] + c);
        if (k <= L - 1 - x) best = min_nonneg(best, in[i + k * stride] + c);
    }
    return best;
}

// grid: x over voxels, y = sample, z = direction.  in, out (jobs, V).
__global__ __launch_bounds__(BLK) void line_kernel(const double* __restrict__ in, double* __restrict__ out, int64_t V, int64_t stride, int L,
                                                   double s) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x, job = (int64_t)blockIdx.y * gridDim.z + blockIdx.z;
    if (i >= V) return;
    out[job * V + i] = line_min(in + job * V, i, stride, (int)(i / stride % L), L, s);
}

// The last pass of mi3d_surface_distances: g3 only where the other map has a surface voxel of the class (query0 / query1 by
// direction), and what the table needs from it.  list (jobs, V): the g3 values of the job's query voxels in any order (the select
// does not depend on it).  state (jobs, 2): [0] how many, [1] the bits of the largest g3.  partial (jobs, gridDim.x): this
// workgroup's sum of sqrt(g3), written by every workgroup.  counts: the row of the class in sample 0, rows `row_stride` apart.
__global__ __launch_bounds__(BLK) void query_kernel(const double* __restrict__ in, double* __restrict__ list, const uint8_t* __restrict__ query0,
                                                    const uint8_t* __restrict__ query1, int match, int64_t V, int64_t stride, int L, double s,
                                                    Tol tol, u64* __restrict__ state, double* __restrict__ partial, u64* __restrict__ counts,
                                                    int64_t row_stride) {
    __shared__ u64 top;
    __shared__ unsigned within[MAXT];
    __shared__ double wave_sum[NW];
    if (threadIdx.x == 0) top = 0;
    if (threadIdx.x < MAXT) within[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x, job = (int64_t)blockIdx.y * gridDim.z + blockIdx.z;
    double root = 0.0;
    if (i < V && (blockIdx.z ? query1 : query0)[blockIdx.y * V + i] == match) {
        const double g = line_min(in + job * V, i, stride, (int)(i / stride % L), L, s);
        const u64 at = atomicAdd(state + 2 * job, 1ull);          // < V: one per query voxel
        list[job * V + at] = g;
        atomicMax(&top, (u64)__double_as_longlong(g));
#pragma unroll
        for (int t = 0; t < MAXT; t++)
            if (t < tol.n && g <= tol.sq[t]) atomicAdd(&within[t], 1u);
        root = sqrt(g);
    }
    block_sum_fixed_put(root, wave_sum);
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[job * gridDim.x + blockIdx.x] = block_sum_fixed_get(wave_sum);
        if (top) atomicMax(state + 2 * job + 1, top);
    }
    if (threadIdx.x < tol.n && within[threadIdx.x])
        atomicAdd(counts + blockIdx.y * row_stride + 2 + blockIdx.z * MAXT + threadIdx.x, (u64)within[threadIdx.x]);
}

// ---- signed distance maps -----------------------------------------------------------------------------------------------------------
// The features of mi3d_signed_distance_maps, one thread per voxel: per (sample, listed class j) the class mask (inside) and its
// inverse (outside), each (N * n_classes, V) bytes, the feat0 / feat1 of the w pass with `match` 1.  grid: x over voxels, y = sample.
template <typename T>
__global__ __launch_bounds__(BLK) void class_masks_kernel(const T* __restrict__ lab, Vol vol, Classes cl, uint8_t* __restrict__ inside,
                                                          uint8_t* __restrict__ outside) {
    const int64_t V = vol.V(), i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= V) return;
    int d, h, w;
    vol.split(i, d, h, w);
    const int c = class_index(cl, (int64_t)lab[blockIdx.y * vol.sn + vol.offset(d, h, w)]);
#pragma unroll
    for (int j = 0; j < MAXC; j++)
        if (j < cl.n) {
            const int64_t at = ((int64_t)blockIdx.y * cl.n + j) * V + i;
            inside[at] = (uint8_t)(j == c), outside[at] = (uint8_t)(j != c);
        }
}

// The last pass of mi3d_signed_distance_maps: the d pass of the ONE direction a voxel needs (inside the class the distance to the
// outside, job 2 m + 1; outside it the distance to the class, job 2 m), its root, the sign and the offset, one rounding to float32.
// A distance of +inf (the class, or its complement, is empty in the sample) gives 0.  grid: x over voxels, y = map m = sample *
// n_classes + class.  in (2 maps, V), phi (maps, V).
__global__ __launch_bounds__(BLK) void signed_kernel(const double* __restrict__ in, const uint8_t* __restrict__ inside, int64_t V, int64_t stride,
                                                     int L, double s, double inner_offset, float* __restrict__ phi) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x, m = blockIdx.y;
    if (i >= V) return;
    const bool in_class = inside[m * V + i] != 0;
    const double g = line_min(in + (2 * m + (in_class ? 1 : 0)) * V, i, stride, (int)(i / stride % L), L, s);
    const double root = sqrt(g);
    const double v = g == inf() ? 0.0 : in_class ? 0.0 - (root - inner_offset) : root;          // 0 - x: a zero is +0
    phi[m * V + i] = (float)v;
}

// ---- select -----------------------------------------------------------------------------------------------------------------------
// One workgroup per (sample, direction).  The sum: thread t adds the partials t, t + 256, ... in that order, then the fixed tree.
// The order statistics of n values at lo = floor((n - 1) q) and hi = ceil((n - 1) q): eight passes over the list, most significant
// byte first; a pass counts, among the keys that share the prefix found so far, the next byte in an LDS histogram, and the byte
// whose cumulative count passes the rank extends the prefix.  After the last pass the prefix is the key of rank lo, `rank` its
// position among its equals and `equal` how many they are; hi = lo + 1 is the same key if it is still among them, else the
// smallest larger key (one more pass).  table: the row of the class in sample 0, rows `row_stride` apart.
__global__ __launch_bounds__(BLK) void select_kernel(const u64* __restrict__ list, int64_t V, const u64* __restrict__ state,
                                                     const double* __restrict__ partial, int64_t blocks, double q, double* __restrict__ table,
                                                     int64_t row_stride) {
    __shared__ unsigned hist[256];
    __shared__ double wave_sum[NW];
    __shared__ u64 above;
    const int64_t job = (int64_t)blockIdx.y * gridDim.z + blockIdx.z;
    const u64 n = state[2 * job];
    double* row = table + blockIdx.y * row_stride + blockIdx.z * 4;
    double sum = 0.0;
    for (int64_t b = threadIdx.x; b < blocks; b += BLK) sum = sum + partial[job * blocks + b];
    block_sum_fixed_put(sum, wave_sum);
    if (threadIdx.x == 0) above = ~0ull;
    __syncthreads();
    if (n == 0) {          // an empty direction
        if (threadIdx.x < 3) row[threadIdx.x] = inf();
        if (threadIdx.x == 3) row[3] = 0.0;
        return;
    }
    if (threadIdx.x == 0) {
        row[0] = __longlong_as_double((long long)state[2 * job + 1]);
        row[3] = block_sum_fixed_get(wave_sum);
    }
    list += job * V;
    const double at = (double)(n - 1) * q;
    const u64 lo = (u64)floor(at), hi = (u64)ceil(at);          // <= n - 1 as q <= 1
    u64 prefix = 0, rank = lo, equal = 0;
    for (int pass = 7; pass >= 0; pass--) {
        const int shift = pass * 8;
        const u64 decided = pass == 7 ? 0 : ~0ull << (shift + 8);
        hist[threadIdx.x] = 0;          // BLK == 256
        __syncthreads();
        for (u64 k = threadIdx.x; k < n; k += BLK) {
            const u64 key = list[k];
            if ((key & decided) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
        }
        __syncthreads();
        u64 below = 0;          // every thread does the same walk: rank < the keys under the prefix, so a byte is found
        int byte = 255;
        for (int b = 0; b < 256; b++) {
            const unsigned c = hist[b];
            if (rank < below + c) {
                byte = b;
                break;
            }
            below += c;
        }
        equal = hist[byte];
        rank -= below;
        prefix |= (u64)byte << shift;
        __syncthreads();
    }
    const u64 at_most = lo - rank + equal;          // keys <= the one of rank lo
    if (hi >= at_most) {
        u64 mine = ~0ull;
        for (u64 k = threadIdx.x; k < n; k += BLK) {
            const u64 key = list[k];
            if (key > prefix && key < mine) mine = key;
        }
        atomicMin(&above, mine);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        row[1] = __longlong_as_double((long long)prefix);
        row[2] = __longlong_as_double((long long)(hi >= at_most ? above : prefix));
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// the two surface bytemaps, two buffers of (sample, direction, voxel) doubles, the partial sums, the state words: the layout, once
struct Workspace {
    uint8_t *pred, *target;
    double *a, *b, *partial;
    u64* state;
    size_t bytes;
    Workspace(void* base, int N, int64_t V) {
        Arena ar{static_cast<char*>(base)};
        pred = ar.take<uint8_t>((size_t)N * V), target = ar.take<uint8_t>((size_t)N * V);
        a = ar.take<double>((size_t)N * V * 2), b = ar.take<double>((size_t)N * V * 2);
        partial = ar.take<double>((size_t)(2 * N * voxel_blocks(V))), state = ar.take<u64>((size_t)N * 4);
        bytes = ar.used;
    }
};

// mi3d_signed_distance_maps: the two feature bytemaps and two buffers of doubles, each per (map, direction, voxel)
struct SignedWorkspace {
    uint8_t *inside, *outside;
    double *a, *b;
    size_t bytes;
    SignedWorkspace(void* base, int64_t maps, int64_t V) {
        Arena ar{static_cast<char*>(base)};
        inside = ar.take<uint8_t>((size_t)maps * V), outside = ar.take<uint8_t>((size_t)maps * V);
        a = ar.take<double>((size_t)maps * V * 2), b = ar.take<double>((size_t)maps * V * 2);
        bytes = ar.used;
    }
};

int check_spacing(const char* name, const double* spacing) {
    MI3D_CHECK_ARG(spacing, "%s: null pointer (spacing)", name);
    for (int a = 0; a < 3; a++)
        MI3D_CHECK_ARG(std::isfinite(spacing[a]) && spacing[a] > 0.0, "%s: spacing %g of axis %d is not a positive finite number", name, spacing[a], a);
    return 0;
}
int surface_launch(const void* labels, int dtype, const Vol& vol, const Classes& cl, int conn, uint8_t* out, u64* counts, hipStream_t s) {
    dim3 grid((unsigned)voxel_blocks(vol.V()), (unsigned)vol.N);
    dispatch_src(dtype, LabelTypes(), [&](auto tag) { surface_kernel<<<grid, BLK, 0, s>>>((const decltype(tag)*)labels, vol, cl, conn, out, counts); });
    MI3D_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" {

size_t mi3d_surface_workspace_bytes(int N, int D, int H, int W, int n_classes) {
    const int64_t NV = total_voxels(N, D, H, W);
    if (NV == 0 || n_classes < 1 || n_classes > MAXC) {
        mi3d_set_error("mi3d_surface_workspace_bytes: N in [1, 65535], sides >= 1, D * H * W < 2^31 and 1 to %d classes expected", MAXC);
        return 0;
    }
    return Workspace(nullptr, N, NV / N).bytes;
}

int mi3d_distance_transform(const void* mask, int mask_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d, int64_t stride_h,
                            int64_t stride_w, const double* spacing, double* dist2_out, void* workspace, size_t workspace_bytes,
                            void* stream) {
    const char* name = "mi3d_distance_transform";
    MI3D_TRY(check_map(name, "mask", mask, mask_dtype, stride_n, stride_d, stride_h, stride_w));
    MI3D_TRY(check_sizes(name, N, D, H, W));
    MI3D_TRY(check_spacing(name, spacing));
    MI3D_CHECK_ARG(dist2_out && ((uintptr_t)dist2_out & 7) == 0, "%s: dist2_out must be a non-null, 8-byte aligned pointer", name);
    const Vol vol{N, D, H, W, stride_n, stride_d, stride_h, stride_w};
    const int64_t V = vol.V();
    const Workspace ws(workspace, N, V);
    MI3D_TRY(check_workspace(name, workspace, workspace_bytes, ws.bytes));
    hipStream_t s = (hipStream_t)stream;
    dim3 vgrid((unsigned)voxel_blocks(V), (unsigned)N), rgrid((unsigned)cdiv((int64_t)D * H, NW), (unsigned)N);
    dispatch_src(mask_dtype, LabelTypes(), [&](auto tag) { nonzero_kernel<<<vgrid, BLK, 0, s>>>((const decltype(tag)*)mask, vol, ws.pred); });
    MI3D_LAUNCH_CHECK();
    w_kernel<<<rgrid, BLK, 0, s>>>(ws.pred, ws.pred, 1, (int64_t)D * H, W, spacing[2], dist2_out);
    MI3D_LAUNCH_CHECK();
    line_kernel<<<vgrid, BLK, 0, s>>>(dist2_out, ws.a, V, W, H, spacing[1]);
    MI3D_LAUNCH_CHECK();
    line_kernel<<<vgrid, BLK, 0, s>>>(ws.a, dist2_out, V, (int64_t)H * W, D, spacing[0]);
    MI3D_LAUNCH_CHECK();
    return 0;
}

int mi3d_surface_mask(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d, int64_t stride_h,
                      int64_t stride_w, int connectivity, int class_value, uint8_t* surface_out, void* stream) {
    const char* name = "mi3d_surface_mask";
    MI3D_TRY(check_map(name, "labels", labels, label_dtype, stride_n, stride_d, stride_h, stride_w));
    MI3D_TRY(check_sizes(name, N, D, H, W));
    MI3D_TRY(check_connectivity(name, connectivity));
    MI3D_CHECK_ARG(surface_out, "%s: null pointer (surface_out)", name);
    Classes cl{};
    cl.n = 1, cl.value[0] = class_value;
    const Vol vol{N, D, H, W, stride_n, stride_d, stride_h, stride_w};
    return surface_launch(labels, label_dtype, vol, cl, connectivity, surface_out, nullptr, (hipStream_t)stream);
}

int mi3d_surface_distances(const void* pred, int pred_dtype, int64_t pred_stride_n, int64_t pred_stride_d, int64_t pred_stride_h,
                           int64_t pred_stride_w, const void* target, int target_dtype, int64_t target_stride_n, int64_t target_stride_d,
                           int64_t target_stride_h, int64_t target_stride_w, int N, int D, int H, int W, int connectivity, int n_classes,
                           const int32_t* class_values, const double* spacing, double q, int n_tol, const double* tol_mm,
                           int64_t* counts_out, double* table_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = "mi3d_surface_distances";
    MI3D_TRY(check_map(name, "pred", pred, pred_dtype, pred_stride_n, pred_stride_d, pred_stride_h, pred_stride_w));
    MI3D_TRY(check_map(name, "target", target, target_dtype, target_stride_n, target_stride_d, target_stride_h, target_stride_w));
    MI3D_TRY(check_sizes(name, N, D, H, W));
    MI3D_TRY(check_connectivity(name, connectivity));
    Classes cl{};
    MI3D_TRY(check_classes(name, n_classes, class_values, cl));
    MI3D_TRY(check_spacing(name, spacing));
    MI3D_CHECK_ARG(q >= 0.0 && q <= 1.0, "%s: q = %g is outside [0, 1]", name, q);
    MI3D_CHECK_ARG(n_tol >= 0 && n_tol <= MAXT, "%s: 0 to %d tolerances, got %d", name, MAXT, n_tol);
    MI3D_CHECK_ARG(n_tol == 0 || tol_mm, "%s: null pointer (tol_mm)", name);
    Tol tol{};
    tol.n = n_tol;
    for (int t = 0; t < n_tol; t++) {
        MI3D_CHECK_ARG(std::isfinite(tol_mm[t]) && tol_mm[t] >= 0.0, "%s: tolerance %g is not a finite number >= 0", name, tol_mm[t]);
        tol.sq[t] = tol_mm[t] * tol_mm[t];
    }
    MI3D_CHECK_ARG(counts_out && table_out && ((uintptr_t)counts_out & 7) == 0 && ((uintptr_t)table_out & 7) == 0,
                   "%s: counts_out and table_out must be non-null, 8-byte aligned pointers", name);
    const Vol pv{N, D, H, W, pred_stride_n, pred_stride_d, pred_stride_h, pred_stride_w};
    const Vol tv{N, D, H, W, target_stride_n, target_stride_d, target_stride_h, target_stride_w};
    const int64_t V = pv.V(), blocks = voxel_blocks(V);
    const Workspace ws(workspace, N, V);
    MI3D_TRY(check_workspace(name, workspace, workspace_bytes, ws.bytes));
    hipStream_t s = (hipStream_t)stream;
    u64* counts = (u64*)counts_out;
    MI3D_HIP(hipMemsetAsync(counts_out, 0, (size_t)N * n_classes * COUNTS * sizeof(int64_t), s));
    MI3D_TRY(surface_launch(pred, pred_dtype, pv, cl, connectivity, ws.pred, counts, s));
    MI3D_TRY(surface_launch(target, target_dtype, tv, cl, connectivity, ws.target, counts + 1, s));
    dim3 vgrid((unsigned)blocks, (unsigned)N, 2), rgrid((unsigned)cdiv((int64_t)D * H, NW), (unsigned)N, 2), jgrid(1, (unsigned)N, 2);
    for (int j = 0; j < n_classes; j++) {          // direction 0: from the surface of pred to that of target; direction 1: back
        MI3D_HIP(hipMemsetAsync(ws.state, 0, (size_t)N * 4 * sizeof(u64), s));
        w_kernel<<<rgrid, BLK, 0, s>>>(ws.target, ws.pred, j + 1, (int64_t)D * H, W, spacing[2], ws.a);
        MI3D_LAUNCH_CHECK();
        line_kernel<<<vgrid, BLK, 0, s>>>(ws.a, ws.b, V, W, H, spacing[1]);
        MI3D_LAUNCH_CHECK();
        query_kernel<<<vgrid, BLK, 0, s>>>(ws.b, ws.a, ws.pred, ws.target, j + 1, V, (int64_t)H * W, D, spacing[0], tol, ws.state, ws.partial,
                                           counts + (int64_t)j * COUNTS, (int64_t)n_classes * COUNTS);
        MI3D_LAUNCH_CHECK();
        select_kernel<<<jgrid, BLK, 0, s>>>((const u64*)ws.a, V, ws.state, ws.partial, blocks, q, table_out + (int64_t)j * TABLE,
                                            (int64_t)n_classes * TABLE);
        MI3D_LAUNCH_CHECK();
    }
    return 0;
}

size_t mi3d_signed_distance_workspace_bytes(int N, int D, int H, int W, int n_classes) {
    const int64_t NV = total_voxels(N, D, H, W);
    if (NV == 0 || n_classes < 1 || n_classes > MAXC || (int64_t)N * n_classes > 65535) {
        mi3d_set_error("mi3d_signed_distance_workspace_bytes: N >= 1, sides >= 1, D * H * W < 2^31, 1 to %d classes and N * n_classes <= 65535 "
                       "expected", MAXC);
        return 0;
    }
    return SignedWorkspace(nullptr, (int64_t)N * n_classes, NV / N).bytes;
}

int mi3d_signed_distance_maps(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d,
                              int64_t stride_h, int64_t stride_w, int n_classes, const int32_t* class_values, const double* spacing,
                              double inner_offset, float* phi_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = "mi3d_signed_distance_maps";
    MI3D_TRY(check_map(name, "labels", labels, label_dtype, stride_n, stride_d, stride_h, stride_w));
    MI3D_TRY(check_sizes(name, N, D, H, W));
    Classes cl{};
    MI3D_TRY(check_classes(name, n_classes, class_values, cl));
    MI3D_CHECK_ARG((int64_t)N * n_classes <= 65535, "%s: N * n_classes = %lld maps, at most 65535", name, (long long)N * n_classes);
    MI3D_TRY(check_spacing(name, spacing));
    MI3D_CHECK_ARG(std::isfinite(inner_offset) && inner_offset >= 0.0, "%s: inner_offset %g is not a finite number >= 0", name, inner_offset);
    MI3D_CHECK_ARG(phi_out && ((uintptr_t)phi_out & 3) == 0, "%s: phi_out must be a non-null, 4-byte aligned pointer", name);
    const Vol vol{N, D, H, W, stride_n, stride_d, stride_h, stride_w};
    const int64_t V = vol.V(), maps = (int64_t)N * n_classes;
    const SignedWorkspace ws(workspace, maps, V);
    MI3D_TRY(check_workspace(name, workspace, workspace_bytes, ws.bytes));
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)voxel_blocks(V);
    dim3 lgrid(blocks, (unsigned)N), vgrid(blocks, (unsigned)maps, 2), rgrid((unsigned)cdiv((int64_t)D * H, NW), (unsigned)maps, 2),
        sgrid(blocks, (unsigned)maps);
    dispatch_src(label_dtype, LabelTypes(),
                 [&](auto tag) { class_masks_kernel<<<lgrid, BLK, 0, s>>>((const decltype(tag)*)labels, vol, cl, ws.inside, ws.outside); });
    MI3D_LAUNCH_CHECK();
    // one sweep over maps x 2 jobs: job 2 m the distance to the class (features: inside), job 2 m + 1 to its complement
    w_kernel<<<rgrid, BLK, 0, s>>>(ws.inside, ws.outside, 1, (int64_t)D * H, W, spacing[2], ws.a);
    MI3D_LAUNCH_CHECK();
    line_kernel<<<vgrid, BLK, 0, s>>>(ws.a, ws.b, V, W, H, spacing[1]);
    MI3D_LAUNCH_CHECK();
    signed_kernel<<<sgrid, BLK, 0, s>>>(ws.b, ws.inside, V, (int64_t)H * W, D, spacing[0], inner_offset, phi_out);
    MI3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
