// patch.hip — foreground-balanced patch sampling of a label map on the GPU: what MONAI's RandCropByPosNegLabeld /
// RandCropByLabelClassesd do on the host with np.nonzero and a slice per patch, without an index list and without the count ever
// reaching the host (spatial.py draws the random words).
//   count_kernel   one workgroup per block of MI3D_PATCH_BLOCK consecutive voxel indices: rows along W in 16-byte loads (any other
//                  layout strided), the voxels of each group from one ballot + popcount per group  -> block counts, counts_out
//   pick_kernel    one workgroup per draw: sums the (sample, group)'s block counts in parallel, finds the block that holds rank r,
//                  scans that one block                                                            -> starts, voxel, picked
//   crop_kernel    K windows of image and label in one launch, the starts read from device memory; four consecutive W per thread,
//                  16-byte stores where the output row allows
// Contract: include/mi3d.h mi3d_patch_count / mi3d_patch_pick / mi3d_patch_crop.  Integer arithmetic only and integer atomics of
// sums: every output has the same bits on every run.  Every index is inside its array by construction: a voxel index past the
// volume is in no group and is never read; a window start is clamped to [0, n - size] where it is used.
#include "volume.h"

namespace {
constexpr int BLK = VOL_BLK, NW = BLK / 64;
constexpr int PB = MI3D_PATCH_BLOCK, PER = PB / BLK;          // voxel indices per block and per thread
constexpr int MAXG = MI3D_COMPONENTS_MAX_CLASSES, NONE = 15;
constexpr int DRAWS = 256;                                    // draws per pick launch: they ride in the kernel's arguments
constexpr int VW = 4;                                         // crop: consecutive W outputs per thread
typedef unsigned long long u64;
static_assert(PB % BLK == 0 && PER % 16 == 0 && MAXG <= NONE, "a thread's share of a block is whole 16-byte pieces of either dtype");

// group_of as 256 nibbles (NONE: in no group), by value in the kernel arguments
struct GroupTable {
    u64 m[16];
};

// every thread t < 256 puts entry t into LDS: unrolled selects, no indexing of the kernel's arguments
__device__ __forceinline__ void table_to_lds(const GroupTable& gt, uint8_t (&tab)[256]) {
    static_assert(BLK == 256, "one thread per table entry");
    u64 word = 0;
#pragma unroll
    for (int j = 0; j < 16; j++)
        if ((int)(threadIdx.x >> 4) == j) word = gt.m[j];
    tab[threadIdx.x] = (uint8_t)((word >> (4 * (threadIdx.x & 15))) & 15);
    __syncthreads();
}
// the group of a label value; an int64 value is tested as it is, before anything narrows it
__device__ __forceinline__ int group_at(const uint8_t (&tab)[256], uint8_t v) { return tab[v]; }
__device__ __forceinline__ int group_at(const uint8_t (&tab)[256], int64_t v) { return v >= 0 && v <= 255 ? tab[(int)v] : NONE; }

// element e of a 16-byte piece (e is a constant after unrolling)
__device__ __forceinline__ uint8_t value_at(const uint4& raw, int e, uint8_t) {
    const unsigned word[4] = {raw.x, raw.y, raw.z, raw.w};
    return (uint8_t)(word[e >> 2] >> (8 * (e & 3)));
}
__device__ __forceinline__ int64_t value_at(const uint4& raw, int e, int64_t) {
    return (int64_t)(e ? (u64)raw.z | (u64)raw.w << 32 : (u64)raw.x | (u64)raw.y << 32);
}

__device__ __forceinline__ void split3(unsigned i, const Vol& vol, int& d, int& h, int& w) {          // Vol::split in 32 bits
    const unsigned r = i / (unsigned)vol.W;
    w = (int)(i - r * (unsigned)vol.W), h = (int)(r % (unsigned)vol.H), d = (int)(r / (unsigned)vol.H);
}

// The groups of the E = 16 / sizeof(T) voxel indices from i (E divides i): one 16-byte load where they lie in one row along a
// unit stride at an aligned address, else one load each through the strides; NONE past the volume.
template <typename T> __device__ __forceinline__ void groups_of_piece(const T* __restrict__ lab, const Vol& vol, unsigned V, unsigned i,
                                                                      const uint8_t (&tab)[256], int (&g)[16 / sizeof(T)]) {
    constexpr int E = 16 / sizeof(T);
#pragma unroll
    for (int e = 0; e < E; e++) g[e] = NONE;
    if (i >= V) return;
    int d, h, w;
    split3(i, vol, d, h, w);
    const T* p = lab + vol.offset(d, h, w);
    if (vol.sw == 1 && w + E <= vol.W && ((uintptr_t)p & 15) == 0) {
        const uint4 raw = *reinterpret_cast<const uint4*>(p);
#pragma unroll
        for (int e = 0; e < E; e++) g[e] = group_at(tab, value_at(raw, e, T()));
        return;
    }
#pragma unroll
    for (int e = 0; e < E; e++) {
        if (i + e < V) g[e] = group_at(tab, lab[vol.offset(d, h, w)]);
        if (++w == vol.W) {
            w = 0;
            if (++h == vol.H) h = 0, d++;
        }
    }
}

// grid: x = block of PB voxel indices, y = sample.  blocks[(n * MAXG + g) * NB + b], counts_out[n * G + g] (zeroed by the entry).
template <typename T>
__global__ __launch_bounds__(BLK) void count_kernel(const T* __restrict__ lab, Vol vol, GroupTable gt, int G, int NB,
                                                    int32_t* __restrict__ blocks, u64* __restrict__ counts_out) {
    constexpr int E = 16 / sizeof(T);
    __shared__ uint8_t tab[256];
    __shared__ int wave_count[NW][MAXG];
    table_to_lds(gt, tab);
    const unsigned V = (unsigned)vol.V(), base = blockIdx.x * (unsigned)PB;
    lab += blockIdx.y * vol.sn;
    int cnt[MAXG] = {};          // wave-uniform
    for (int piece = threadIdx.x; piece < PB / E; piece += BLK) {          // the same trip count for every thread: the ballots are whole
        int g[E];
        groups_of_piece(lab, vol, V, base + (unsigned)piece * E, tab, g);
#pragma unroll
        for (int e = 0; e < E; e++)
#pragma unroll
            for (int j = 0; j < MAXG; j++) cnt[j] += __popcll(__ballot(g[e] == j));
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < MAXG; j++)
        if (lane == j) wave_count[wave][j] = cnt[j];
    __syncthreads();
    if (threadIdx.x < MAXG) {
        int sum = 0;
        for (int v = 0; v < NW; v++) sum += wave_count[v][threadIdx.x];
        blocks[((int64_t)blockIdx.y * MAXG + threadIdx.x) * NB + blockIdx.x] = sum;
        if ((int)threadIdx.x < G && sum) atomicAdd(counts_out + (int64_t)blockIdx.y * G + threadIdx.x, (u64)sum);
    }
}

// The exclusive prefix of x over the workgroup in thread order, and the total.  Every thread calls it.
__device__ __forceinline__ unsigned block_scan(unsigned x, unsigned (&wave_sum)[NW], unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    __syncthreads();          // the previous call's readers are done with wave_sum
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (int v = 0; v < NW; v++) {
        if (v < wave) before += wave_sum[v];
        total += wave_sum[v];
    }
    return before + incl - x;
}

struct Draws {          // of one launch, by value: sg = sample << 8 | group
    u64 rnd[DRAWS];
    int32_t sg[DRAWS];
};
struct Window {
    int size[3];
};

// One workgroup per draw.  blockIdx.x indexes the arguments uniformly: scalar loads from the argument segment.
template <typename T>
__global__ __launch_bounds__(BLK) void pick_kernel(const T* __restrict__ lab, Vol vol, GroupTable gt, int NB, const int32_t* __restrict__ blocks,
                                                   Draws draws, Window win, int32_t* __restrict__ starts_out, int32_t* __restrict__ voxel_out,
                                                   int32_t* __restrict__ picked_out) {
    __shared__ uint8_t tab[256];
    __shared__ unsigned wave_sum[NW];
    __shared__ unsigned found[2];          // the block that holds the rank, the rank within it; then [0] the voxel
    table_to_lds(gt, tab);
    const u64 rnd = draws.rnd[blockIdx.x];
    const int sample = draws.sg[blockIdx.x] >> 8, group = draws.sg[blockIdx.x] & 255;
    const unsigned V = (unsigned)vol.V();
    lab += sample * vol.sn;
    blocks += ((int64_t)sample * MAXG + group) * NB;
    // a contiguous run of block counts per thread, so that thread order is block order
    const int per = (NB + BLK - 1) / BLK, b0 = min((int)threadIdx.x * per, NB), b1 = min(b0 + per, NB);
    unsigned mine = 0;
    for (int b = b0; b < b1; b++) mine += (unsigned)blocks[b];
    unsigned count;
    unsigned before = block_scan(mine, wave_sum, count);
    unsigned voxel;
    if (count == 0) {          // uniform: the group is absent from this sample
        voxel = (unsigned)__umul64hi(rnd, (u64)V);
    } else {
        const unsigned r = (unsigned)__umul64hi(rnd, (u64)count);
        if (threadIdx.x == 0) found[0] = 0, found[1] = 0;
        __syncthreads();
        if (r >= before && r - before < mine) {          // exactly one thread
            unsigned left = r - before;
            int b = b0;
            for (; b < b1 - 1 && left >= (unsigned)blocks[b]; b++) left -= (unsigned)blocks[b];
            found[0] = (unsigned)b, found[1] = left;
        }
        __syncthreads();
        const unsigned base = found[0] * (unsigned)PB + threadIdx.x * PER, left = found[1];
        constexpr int E = 16 / sizeof(T);
        unsigned hits = 0;          // bit q: voxel base + q is of the group
#pragma unroll
        for (int piece = 0; piece < PER / E; piece++) {
            int g[E];
            groups_of_piece(lab, vol, V, base + piece * E, tab, g);
#pragma unroll
            for (int e = 0; e < E; e++) hits |= (unsigned)(g[e] == group) << (piece * E + e);
        }
        static_assert(PER <= 32, "a thread's hits fit one word");
        unsigned total;
        before = block_scan((unsigned)__popc(hits), wave_sum, total);
        if (threadIdx.x == 0) found[0] = 0;
        __syncthreads();
        if (left >= before && left - before < (unsigned)__popc(hits)) {          // exactly one thread
            unsigned skip = left - before, h = hits;
            for (; skip > 0; skip--) h &= h - 1;
            found[0] = base + (unsigned)__ffs(h) - 1;
        }
        __syncthreads();
        voxel = found[0];
    }
    if (threadIdx.x == 0) {
        int c[3];
        split3(min(voxel, V - 1), vol, c[0], c[1], c[2]);
        const int n[3] = {vol.D, vol.H, vol.W};
        const int64_t k = blockIdx.x;
#pragma unroll
        for (int a = 0; a < 3; a++) starts_out[k * 3 + a] = min(max(c[a] - win.size[a] / 2, 0), n[a] - win.size[a]);
        voxel_out[k] = (int)voxel;
        picked_out[k] = count ? group : -1;
    }
}

struct CropMap {
    int n[3], no[3];
};
__device__ __forceinline__ void store4(uint32_t* dst, const uint32_t (&v)[VW]) { *reinterpret_cast<uint4*>(dst) = make_uint4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void store4(int64_t* dst, const int64_t (&v)[VW]) {
    longlong2 a, b;
    a.x = v[0], a.y = v[1], b.x = v[2], b.y = v[3];
    *reinterpret_cast<longlong2*>(dst) = a;
    *reinterpret_cast<longlong2*>(dst + 2) = b;
}
// VW consecutive values of a row, loaded one by one (the source is unaligned by the window's start), stored at once where VEC
template <bool VEC, typename T> __device__ __forceinline__ void copy_piece(const T* __restrict__ src, T* __restrict__ dst, int left) {
    T v[VW];
#pragma unroll
    for (int j = 0; j < VW; j++) v[j] = (VEC || j < left) ? src[j] : T(0);
    if constexpr (VEC) {
        store4(dst, v);
    } else {
#pragma unroll
        for (int j = 0; j < VW; j++)
            if (j < left) dst[j] = v[j];
    }
}

// One thread: VW consecutive W outputs of output row (od, oh) of window blockIdx.y, every channel.  The image moves as 32-bit words:
// a copy keeps every bit pattern.  VEC needs Wo % VW == 0 and 16-byte aligned output bases.
template <bool VEC>
__global__ __launch_bounds__(BLK) void crop_kernel(const uint32_t* __restrict__ img_in, uint32_t* __restrict__ img_out,
                                                   const int64_t* __restrict__ lab_in, int64_t* __restrict__ lab_out,
                                                   const int32_t* __restrict__ starts, int C, CropMap m, int WQ, int64_t total) {
    const int64_t q = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (q >= total) return;
    const int64_t r = q / WQ;
    const int w0 = (int)(q - r * WQ) * VW, oh = (int)(r % m.no[1]), od = (int)(r / m.no[1]);
    const int Wo = m.no[2];
    const int64_t Vo = (int64_t)m.no[0] * m.no[1] * Wo, Vi = (int64_t)m.n[0] * m.n[1] * m.n[2];
    int st[3];
#pragma unroll
    for (int a = 0; a < 3; a++) st[a] = min(max(starts[blockIdx.y * 3 + a], 0), m.n[a] - m.no[a]);          // no_a <= n_a: inside, whatever came in
    const int64_t irow = ((int64_t)(st[0] + od) * m.n[1] + (st[1] + oh)) * m.n[2] + (st[2] + w0);
    const int64_t orow = (int64_t)blockIdx.y * C * Vo + ((int64_t)od * m.no[1] + oh) * Wo + w0;
    for (int c = 0; c < C; c++) {
        if (lab_in) copy_piece<VEC>(lab_in + c * Vi + irow, lab_out + c * Vo + orow, Wo - w0);
        if (img_in) copy_piece<VEC>(img_in + c * Vi + irow, img_out + c * Vo + orow, Wo - w0);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
int64_t patch_blocks(int64_t V) { return (V + PB - 1) / PB; }

struct Workspace {          // the layout, once: mi3d_patch_workspace_bytes counts it over a null base
    int32_t* blocks;        // [N][MAXG][NB]
    size_t bytes;
    Workspace(void* base, int N, int64_t NB) {
        Arena a{static_cast<char*>(base)};
        blocks = a.take<int32_t>((size_t)N * MAXG * NB);
        bytes = a.used;
    }
};

// group_of -> the nibble table and G = 1 + the largest group it names
int check_groups(const char* name, const uint8_t* group_of, GroupTable& gt, int& G) {
    MI3D_CHECK_ARG(group_of, "%s: null pointer (group_of)", name);
    gt = GroupTable{};
    G = 0;
    for (int v = 0; v < 256; v++) {
        const int g = group_of[v];
        MI3D_CHECK_ARG(g < MAXG || g == 255, "%s: group_of[%d] = %d is neither a group 0..%d nor 255", name, v, g, MAXG - 1);
        gt.m[v >> 4] |= (u64)(g == 255 ? NONE : g) << (4 * (v & 15));
        if (g != 255 && g + 1 > G) G = g + 1;
    }
    MI3D_CHECK_ARG(G >= 1, "%s: group_of names no group", name);
    return 0;
}

int check_common(const char* name, const void* labels, int label_dtype, int N, int D, int H, int W, int64_t sn, int64_t sd, int64_t sh,
                 int64_t sw, const void* workspace, size_t workspace_bytes_given) {
    MI3D_TRY(check_map(name, "labels", labels, label_dtype, sn, sd, sh, sw));
    MI3D_TRY(check_sizes(name, N, D, H, W));
    return check_workspace(name, workspace, workspace_bytes_given, Workspace(nullptr, N, patch_blocks((int64_t)D * H * W)).bytes);
}

// a sample that lies in C order is one row of V voxels: the same indices, every load wide
Vol row_view(int N, int D, int H, int W, int64_t sn, int64_t sd, int64_t sh, int64_t sw) {
    if (sw == 1 && (sh == W || H == 1) && (sd == (int64_t)H * W || D == 1)) return Vol{N, 1, 1, D * H * W, sn, (int64_t)D * H * W, (int64_t)D * H * W, 1};
    return Vol{N, D, H, W, sn, sd, sh, sw};
}
}  // namespace

extern "C" {

size_t mi3d_patch_workspace_bytes(int N, int D, int H, int W) {
    if (total_voxels(N, D, H, W) == 0) {
        mi3d_set_error("mi3d_patch_workspace_bytes: N in [1, 65535], sides >= 1 and D * H * W < 2^31 expected");
        return 0;
    }
    return Workspace(nullptr, N, patch_blocks((int64_t)D * H * W)).bytes;
}

int mi3d_patch_count(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d, int64_t stride_h,
                     int64_t stride_w, const uint8_t* group_of, int64_t* counts_out, void* workspace, size_t workspace_bytes,
                     void* stream) {
    const char* name = "mi3d_patch_count";
    MI3D_TRY(check_common(name, labels, label_dtype, N, D, H, W, stride_n, stride_d, stride_h, stride_w, workspace, workspace_bytes));
    GroupTable gt;
    int G;
    MI3D_TRY(check_groups(name, group_of, gt, G));
    MI3D_CHECK_ARG(counts_out && ((uintptr_t)counts_out & 7) == 0, "%s: counts_out is null or not 8-byte aligned", name);
    const Vol vol = row_view(N, D, H, W, stride_n, stride_d, stride_h, stride_w);
    const int NB = (int)patch_blocks(vol.V());
    const Workspace ws(workspace, N, NB);
    hipStream_t s = (hipStream_t)stream;
    MI3D_HIP(hipMemsetAsync(counts_out, 0, (size_t)N * G * sizeof(int64_t), s));
    dispatch_src(label_dtype, LabelTypes(), [&](auto tag) {
        using T = decltype(tag);
        count_kernel<T><<<dim3((unsigned)NB, (unsigned)N), BLK, 0, s>>>((const T*)labels, vol, gt, G, NB, ws.blocks, (u64*)counts_out);
    });
    MI3D_LAUNCH_CHECK();
    return 0;
}

int mi3d_patch_pick(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d, int64_t stride_h,
                    int64_t stride_w, const uint8_t* group_of, int K, const int32_t* sample, const int32_t* group, const uint64_t* rnd,
                    const int32_t* size, int32_t* starts_out, int32_t* voxel_out, int32_t* picked_out, const void* workspace,
                    size_t workspace_bytes, void* stream) {
    const char* name = "mi3d_patch_pick";
    MI3D_TRY(check_common(name, labels, label_dtype, N, D, H, W, stride_n, stride_d, stride_h, stride_w, workspace, workspace_bytes));
    GroupTable gt;
    int G;
    MI3D_TRY(check_groups(name, group_of, gt, G));
    MI3D_CHECK_ARG(K >= 1 && K <= 65535, "%s: 1 to 65535 draws, got %d", name, K);
    MI3D_CHECK_ARG(sample && group && rnd && size && starts_out && voxel_out && picked_out, "%s: null pointer", name);
    const int n[3] = {D, H, W};
    Window win;
    for (int a = 0; a < 3; a++) {
        MI3D_CHECK_ARG(size[a] >= 1 && size[a] <= n[a], "%s: a window of (%d, %d, %d) does not fit a volume of (%d, %d, %d)", name, size[0],
                       size[1], size[2], D, H, W);
        win.size[a] = size[a];
    }
    for (int k = 0; k < K; k++) {
        MI3D_CHECK_ARG(sample[k] >= 0 && sample[k] < N, "%s: draw %d names sample %d of %d", name, k, sample[k], N);
        MI3D_CHECK_ARG(group[k] >= 0 && group[k] < G, "%s: draw %d names group %d of %d", name, k, group[k], G);
    }
    // the pick splits a voxel index over the logical sides, so it keeps them; the count's row view has the same indices and blocks
    const Vol vol{N, D, H, W, stride_n, stride_d, stride_h, stride_w};
    const int NB = (int)patch_blocks(vol.V());
    const Workspace ws(const_cast<void*>(workspace), N, NB);
    hipStream_t s = (hipStream_t)stream;
    for (int k0 = 0; k0 < K; k0 += DRAWS) {
        const int kn = K - k0 < DRAWS ? K - k0 : DRAWS;
        Draws draws = {};
        for (int k = 0; k < kn; k++) draws.rnd[k] = rnd[k0 + k], draws.sg[k] = sample[k0 + k] << 8 | group[k0 + k];
        dispatch_src(label_dtype, LabelTypes(), [&](auto tag) {
            using T = decltype(tag);
            pick_kernel<T><<<kn, BLK, 0, s>>>((const T*)labels, vol, gt, NB, ws.blocks, draws, win, starts_out + (int64_t)k0 * 3, voxel_out + k0,
                                              picked_out + k0);
        });
        MI3D_LAUNCH_CHECK();
    }
    return 0;
}

int mi3d_patch_crop(const float* img_in, float* img_out, const int64_t* lab_in, int64_t* lab_out, int K, int C, int D, int H, int W, int Do,
                    int Ho, int Wo, const int32_t* starts, void* stream) {
    const char* name = "mi3d_patch_crop";
    MI3D_CHECK_ARG(!img_in == !img_out && !lab_in == !lab_out && (img_in || lab_in),
                   "%s: the image pair, the label pair or both, each with its input AND its output", name);
    MI3D_CHECK_ARG((!img_in || img_in != img_out) && (!lab_in || lab_in != lab_out), "%s: input and output alias", name);
    MI3D_CHECK_ARG(starts, "%s: null pointer (starts)", name);
    MI3D_CHECK_ARG(K >= 1 && K <= 65535, "%s: 1 to 65535 windows, got %d", name, K);
    MI3D_CHECK_ARG(C >= 1 && D >= 1 && H >= 1 && W >= 1 && (int64_t)C * D * H * W <= INT32_MAX && (int64_t)D * H <= INT32_MAX,
                   "%s: positive sizes and at most 2^31 - 1 input voxels expected, got (%d, %d, %d, %d)", name, C, D, H, W);
    MI3D_CHECK_ARG(Do >= 1 && Do <= D && Ho >= 1 && Ho <= H && Wo >= 1 && Wo <= W, "%s: a window of (%d, %d, %d) does not fit a volume of (%d, %d, %d)",
                   name, Do, Ho, Wo, D, H, W);
    const CropMap m{{D, H, W}, {Do, Ho, Wo}};
    const int WQ = (Wo + VW - 1) / VW;
    const int64_t total = (int64_t)Do * Ho * WQ;          // <= D * H * W
    const dim3 grid((unsigned)((total + BLK - 1) / BLK), (unsigned)K);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(img_in);
    uint32_t* dst = reinterpret_cast<uint32_t*>(img_out);
    hipStream_t s = (hipStream_t)stream;
    if (Wo % VW == 0 && aligned16(img_out) && aligned16(lab_out))
        crop_kernel<true><<<grid, BLK, 0, s>>>(src, dst, lab_in, lab_out, starts, C, m, WQ, total);
    else
        crop_kernel<false><<<grid, BLK, 0, s>>>(src, dst, lab_in, lab_out, starts, C, m, WQ, total);
    MI3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
