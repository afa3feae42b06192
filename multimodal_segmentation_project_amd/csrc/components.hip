// components.hip — connected components of a multi-class label volume, the k largest per class, and the filtered map: what a user
// of the segmenter does on the host with scipy.ndimage.label(labels == c, generate_binary_structure(3, conn)) per class, then
// np.bincount and np.isin.  The reference writes its predictions out uncleaned (test_model.py:299-309); scipy is the contract.
//   tile pass      union-find of one TD x TH x 64 tile in LDS, row runs from one ballot      -> parent (local root), cls, size in tile
//   seam pass      pairs of neighbours in different tiles, lock-free union in global memory  -> parent (a forest over the sample)
//   flatten        root[i] = the root of i, one integer atomic per (tile, component)         -> root, size[root]
//   select         every root offers (size << 32 | ~root) to the k slots of its class        -> stats (components, voxels, k keys)
//   finish         keys -> sizes and roots of the kept components                            -> stats
//   apply          a voxel of a listed class keeps its label iff its root is kept            -> labels_out, through the strides
// and the enclosed holes of the map filled by their enclosing class (mi3d_fill_holes): tile, seam and flatten over the BACKGROUND
// (the tile pass takes a value map and there also leaves a C-ordered volume of label codes), then
//   ring           a background voxel's non-background neighbours, min and max code          -> lo[root], hi[root]
//   fill           enclosed (hi below "outside"), one listed value (lo == hi), size in range -> labels_out, stats, summary
// A voxel's index is d * H * W + h * W + w in its sample, logical axes, whatever the strides.  A union always hangs the larger
// root under the smaller, so the root of a set is its smallest index, the first voxel in C order: the labelling is canonical, it
// does not depend on launch order, tile size or strides.  Only integer atomics (min, add, max of unique keys) are used: every
// output has the same bits on every run.  No workgroup waits on another; every parent-following loop counts its steps and, past
// its bound, sets the status word and leaves.
#include "volume.h"

namespace {
constexpr int BLK = 256, NW = BLK / 64;
constexpr int TW = 64, TH = MI3D_COMPONENTS_TILE, TD = MI3D_COMPONENTS_TILE, ROWS = TD * TH, TILE = ROWS * TW;
constexpr int MAXC = MI3D_COMPONENTS_MAX_CLASSES, MAXK = MI3D_COMPONENTS_MAX_KEEP, STATS = 3 + 2 * MAXK;
constexpr unsigned SELECT_BLOCKS = 512;          // the select pass strides over the sample: a workgroup's candidates meet 512 others at most
typedef unsigned long long u64;

struct Select {                      // bit v: label value v is selected; bit 0 is never set
    u64 m[4];
};
// What the tile pass labels is decided by a VALUE MAP, a template parameter of tile_kernel: value(v) is the component value 0..255 of
// label v (0: in no component), and a map with CODES = true also hands out the code volume that mi3d_fill_holes reads.
struct KeepSelected {                // components of the selected values 1..255, each under its own value
    static constexpr bool CODES = false;
    static constexpr int64_t PADDING = 0;          // the label a tile carries past the volume's edge: one whose value() is 0
    Select sel;
    __device__ __forceinline__ int value(int64_t v) const;
    __device__ __forceinline__ void put_code(int64_t, int64_t) const {}
};
constexpr int CODE_OTHER = 256, CODE_OUTSIDE = 257;          // above every label value; a position outside the volume above all
struct Background {                  // components of the background (label exactly 0) under value 1; code[i]: the label 0..255 of voxel i,
    static constexpr bool CODES = true;          // CODE_OTHER for every other int64 value
    static constexpr int64_t PADDING = 1;
    uint16_t* code;
    __device__ __forceinline__ int value(int64_t v) const { return v == 0; }
    __device__ __forceinline__ void put_code(int64_t i, int64_t v) const { code[i] = (uint16_t)(v >= 0 && v <= 255 ? (int)v : CODE_OTHER); }
};

__device__ __forceinline__ int selected(const Select& s, int64_t v) {
    if (v < 1 || v > 255) return 0;
    const u64 lo = (v & 64) ? s.m[1] : s.m[0], hi = (v & 64) ? s.m[3] : s.m[2];
    return (int)((((v & 128) ? hi : lo) >> (v & 63)) & 1);
}
__device__ __forceinline__ int KeepSelected::value(int64_t v) const { return selected(sel, v) ? (int)v : 0; }
template <typename T> __device__ __forceinline__ int64_t label_value(const T* p, int64_t off) { return (int64_t)p[off]; }

// The preceding half of the 26 neighbours in C order, without the left neighbour (0, 0, -1): dd < 0, or dd == 0 and dh < 0.
__device__ __forceinline__ void back_offset(int j, int& dd, int& dh, int& dw) {
    dd = j < 9 ? -1 : 0;
    dh = j < 9 ? j / 3 - 1 : -1;
    dw = j % 3 - 1;
}

// Which pairs need a union at all.  A voxel is a START if it opens a row run of its tile: its tile column is 0 or its left
// neighbour carries another value.  With v a voxel, n = v + (dd, dh, dw) of the same value:
//   dw ==  0: not needed if neither is a start: their left neighbours l, nl are joined to them by the runs and are a pair of the
//             same offset in the same two tiles, needed or (by induction down to a start) joined;
//   dw == -1: not needed if v is no start: n is the (dd, dh, 0) neighbour of v's left neighbour, the case above;
//   dw == +1: not needed if n is no start: n's left neighbour is the (dd, dh, 0) neighbour of v.
__device__ __forceinline__ bool pair_needed(int dw, bool v_start, bool n_start) {
    return dw == 0 ? (v_start || n_start) : dw < 0 ? v_start : n_start;
}

// ---- tile pass ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the root of x in the tile's forest; -1 past the bound
__device__ __forceinline__ int tile_find(int* par, int x, int& budget) {
    for (;;) {
        const int p = lds_load(par + x);
        if (p == x) return x;
        if (--budget < 0) return -1;
        x = p;
    }
}
// Join the sets of a and b: hang the larger root under the smaller with atomicMin and go on from what the atomic returned, which
// is the parent the larger root really had: if another wave re-parented it meanwhile, that parent is joined instead.
__device__ __forceinline__ bool tile_union(int* par, int a, int b, int budget) {
    for (;;) {
        a = tile_find(par, a, budget);
        b = tile_find(par, b, budget);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return true;
        if (--budget < 0) return false;
        a = old;
    }
}

// One workgroup per tile of TD x TH rows of 64 voxels along w; a wave takes a row at a time, lane = w.  grid: x = tile, y = sample.
template <typename T, typename Map>
__global__ __launch_bounds__(BLK) void tile_kernel(const T* __restrict__ lab, Vol vol, Map map, int conn, int tilesW, int tilesH,
                                                   int32_t* __restrict__ parent, uint8_t* __restrict__ cls, int32_t* __restrict__ size,
                                                   int32_t* __restrict__ status) {
    __shared__ int par[TILE];
    __shared__ uint8_t val[TILE];
    __shared__ u64 runs[ROWS];          // bit w: voxel w of the row continues the run of w - 1
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tw = blockIdx.x % tilesW, th = (blockIdx.x / tilesW) % tilesH, td = blockIdx.x / (tilesW * tilesH);
    const int d0 = td * TD, h0 = th * TH, w0 = tw * TW, w = w0 + lane;
    const int64_t V = vol.V(), sample = (int64_t)blockIdx.y * V;
    lab += blockIdx.y * vol.sn;
    int64_t mine[ROWS / NW];          // every load of the tile in flight before the first is used
#pragma unroll
    for (int q = 0; q < ROWS / NW; q++) {
        const int r = wave + q * NW, d = d0 + r / TH, h = h0 + r % TH;
        mine[q] = d < vol.D && h < vol.H && w < vol.W ? label_value(lab, vol.offset(d, h, w)) : Map::PADDING;
    }
#pragma unroll
    for (int q = 0; q < ROWS / NW; q++) {
        const int r = wave + q * NW, d = d0 + r / TH, h = h0 + r % TH;
        const bool in = d < vol.D && h < vol.H && w < vol.W;
        const int v = map.value(mine[q]);
        const int left = __shfl_up(v, 1, 64);
        const u64 cont = __ballot(lane > 0 && v != 0 && left == v);
        const u64 starts = ~cont & (~0ull >> (63 - lane));          // the starts at or below this lane; lane 0 is one
        const int start = 63 - __builtin_clzll(starts);
        val[r * TW + lane] = (uint8_t)v;
        par[r * TW + lane] = v ? r * TW + start : -1;
        if (lane == 0) runs[r] = cont;
        if (in) {
            const int64_t i = sample + ((int64_t)d * vol.H + h) * vol.W + w;
            cls[i] = (uint8_t)v;
            if constexpr (Map::CODES) map.put_code(i, mine[q]);
        }
    }
    __syncthreads();
    bool ok = true;
    for (int r = wave; r < ROWS; r += NW) {
        const int v = val[r * TW + lane];
        if (!v) continue;
        const int rd = r / TH, rh = r % TH;
        const bool v_start = !((runs[r] >> lane) & 1);
        for (int j = 0; j < 12; j++) {
            int dd, dh, dw;
            back_offset(j, dd, dh, dw);
            const int nd = rd + dd, nh = rh + dh, nw = lane + dw;
            if (nonzeros(dd, dh, dw) > conn || nd < 0 || nh < 0 || nh >= TH || nw < 0 || nw >= TW) continue;
            const int nr = nd * TH + nh;
            if (val[nr * TW + nw] != v) continue;
            if (!pair_needed(dw, v_start, !((runs[nr] >> nw) & 1))) continue;
            ok = tile_union(par, r * TW + lane, nr * TW + nw, 4 * TILE) && ok;
        }
    }
    __syncthreads();
    int local[ROWS / NW];          // the tile root of this lane's voxel in each of the wave's rows, -1 off-component
#pragma unroll
    for (int q = 0; q < ROWS / NW; q++) {
        const int x = (wave + q * NW) * TW + lane;
        int t = -1;
        if (val[x]) {
            int budget = TILE;
            t = tile_find(par, x, budget);
            if (t < 0) ok = false, t = x;          // its own root: stays in bounds, status tells
        }
        local[q] = t;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < TILE; x += BLK) par[x] = 0;          // from here on: voxels of the tile under each tile root
    __syncthreads();
#pragma unroll
    for (int q = 0; q < ROWS / NW; q++) {
        const u64 cont = runs[wave + q * NW];
        if (local[q] >= 0 && !((cont >> lane) & 1)) {          // the first voxel of a run adds the run: one LDS atomic per run
            const u64 above = lane == 63 ? 0 : ~cont >> (lane + 1);          // bit t: voxel lane + 1 + t opens another run
            atomicAdd(par + local[q], above ? __builtin_ctzll(above) + 1 : 64 - lane);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < ROWS / NW; q++) {
        const int r = wave + q * NW, d = d0 + r / TH, h = h0 + r % TH;
        if (!(d < vol.D && h < vol.H && w < vol.W)) continue;
        const int64_t i = sample + ((int64_t)d * vol.H + h) * vol.W + w;
        const int t = local[q], tr = t / TW;
        parent[i] = t < 0 ? -1 : (int)(((int64_t)(d0 + tr / TH) * vol.H + (h0 + tr % TH)) * vol.W + (w0 + t % TW));
        if (size) size[i] = par[r * TW + lane];          // > 0 at a tile root only
    }
    if (!ok) atomicOr(status, MI3D_COMPONENTS_STATUS_TILE);
}

// ---- seam pass ------------------------------------------------------------------------------------------------------------------
// Several workgroups read and write `parent` here and the 8 XCDs have private L2s: every access is an agent-scope relaxed atomic,
// performed at the memory all XCDs share, and every decision is taken on the value an atomic returned.  Within this launch a
// parent only ever decreases and always names a voxel of the same component, so a walk that reads an older value still climbs
// the same tree; the kernel boundary publishes the finished forest to the flatten pass.
__device__ __forceinline__ int g_load(int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int seam_find(int32_t* parent, int x, int64_t& budget) {
    for (;;) {
        const int p = g_load(parent + x);
        if (p == x) return x;
        if (--budget < 0 || p < 0) return -1;
        x = p;
    }
}
__device__ __forceinline__ bool seam_union(int32_t* parent, int a, int b, int64_t budget) {
    for (;;) {
        a = seam_find(parent, a, budget);
        b = seam_find(parent, b, budget);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return true;
        if (--budget < 0) return false;
        a = old;
    }
}

// One thread per voxel; only a voxel with a preceding neighbour in another tile has work.  grid: x over voxels, y = sample.
__global__ __launch_bounds__(BLK) void seam_kernel(Vol vol, int conn, int32_t* __restrict__ parent, const uint8_t* __restrict__ cls,
                                                   int32_t* __restrict__ status) {
    const int64_t V = vol.V(), i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= V) return;
    parent += blockIdx.y * V, cls += blockIdx.y * V;
    int d, h, w;
    vol.split(i, d, h, w);
    const int cw = w % TW, ch = h % TH, cd = d % TD;
    if (cd > 0 && ch > 0 && ch < TH - 1 && cw > 0 && cw < TW - 1) return;          // every neighbour in the same tile
    const int v = cls[i];
    if (!v) return;
    const bool v_start = cw == 0 || cls[i - 1] != v;
    bool ok = true;
    const int64_t bound = 2 * V + 64;
    if (cw == 0 && w > 0 && cls[i - 1] == v) ok = seam_union(parent, (int)i, (int)i - 1, bound);          // the run goes on
    for (int j = 0; j < 12; j++) {
        int dd, dh, dw;
        back_offset(j, dd, dh, dw);
        const int nd = d + dd, nh = h + dh, nw = w + dw;
        if (nonzeros(dd, dh, dw) > conn || nd < 0 || nh < 0 || nh >= vol.H || nw < 0 || nw >= vol.W) continue;
        if (nd / TD == d / TD && nh / TH == h / TH && nw / TW == w / TW) continue;          // the tile pass joined them
        const int64_t n = ((int64_t)nd * vol.H + nh) * vol.W + nw;
        if (cls[n] != v) continue;
        const bool n_start = nw % TW == 0 || cls[n - 1] != v;
        if (!pair_needed(dw, v_start, n_start)) continue;
        ok = seam_union(parent, (int)i, (int)n, bound) && ok;
    }
    if (!ok) atomicOr(status, MI3D_COMPONENTS_STATUS_SEAM);
}

// ---- flatten and sizes ----------------------------------------------------------------------------------------------------------
// Nothing writes `parent` here: plain loads of what the seam launch left.  size[i] came in as the voxels of i's tile under tile
// root i (0 elsewhere); every tile root that is not the root of its component adds its count to size[root]: one integer atomic per
// (tile, component).  A word that is read plainly here belongs to such a tile root and is nobody's target.
__global__ __launch_bounds__(BLK) void flatten_kernel(Vol vol, const int32_t* __restrict__ parent, int32_t* __restrict__ root,
                                                      int32_t* size, int32_t* __restrict__ status) {
    const int64_t V = vol.V(), i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= V) return;
    parent += blockIdx.y * V;
    int r = parent[i];
    if (r >= 0) {
        int64_t budget = V;
        for (;;) {
            const int p = parent[r];
            if (p == r) break;
            if (--budget < 0 || p < 0) {
                atomicOr(status, MI3D_COMPONENTS_STATUS_FLATTEN);
                r = (int)i;
                break;
            }
            r = p;
        }
    }
    root[blockIdx.y * V + i] = r;
    if (size && r >= 0 && r != (int)i) {
        const int in_tile = size[blockIdx.y * V + i];
        if (in_tile > 0) atomicAdd(size + blockIdx.y * V + r, in_tile);
    }
}

// ---- select ---------------------------------------------------------------------------------------------------------------------
// stats row of (sample, class) while the components are counted: [0] components, [1] voxels, [3 .. 3 + k) the k largest keys in
// descending order.  A key (size << 32) | (0xffffffff - root) is unique and never 0.  Insertion: atomicMax into slot 0 and carry
// the smaller of (key, what the slot held) to the next slot.  Every slot keeps the maximum of what reached it, and what reaches
// slot j + 1 is everything that reached slot j but that maximum, so slot j ends as the (j + 1)-th largest key whatever the order
// of the atomics.  Slots only grow: a key below slot k - 1 can never enter and is dropped after one look.  A workgroup first keeps
// its own k best per class in LDS by the same insertion (they include whatever it can contribute to the sample's k best) and counts
// components and voxels there; at its end it offers those keys and adds the counts, once.
__device__ __forceinline__ int keep_count(const KeepClasses& cl, int c) {          // cl.k[c] without indexing the kernel's arguments
    int k = 0;
#pragma unroll
    for (int j = 0; j < MAXC; j++)
        if (j == c) k = cl.k[j];
    return k;
}
__device__ __forceinline__ void offer(u64* slot, int k, u64 key) {
    if (key <= __hip_atomic_load(slot + k - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    for (int j = 0; j < k && key; j++) {
        const u64 old = atomicMax(slot + j, key);
        key = old < key ? old : key;
    }
}
__global__ __launch_bounds__(BLK) void select_kernel(Vol vol, KeepClasses cl, const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                     const uint8_t* __restrict__ cls, u64* __restrict__ stats) {
    __shared__ unsigned comps[MAXC], voxels[MAXC];
    __shared__ u64 best[MAXC][MAXK];
    if (threadIdx.x < MAXC) comps[threadIdx.x] = 0, voxels[threadIdx.x] = 0;
    if (threadIdx.x < MAXC * MAXK) best[threadIdx.x / MAXK][threadIdx.x % MAXK] = 0;
    __syncthreads();
    const int64_t V = vol.V();
    stats += (int64_t)blockIdx.y * cl.n * STATS;
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < V; i += (int64_t)gridDim.x * BLK) {
        if (root[blockIdx.y * V + i] != (int)i) continue;
        const int v = cls[blockIdx.y * V + i];
        int k;
        const int c = class_index(cl, v, k);
        if (c >= 0) {
            const unsigned sz = (unsigned)size[blockIdx.y * V + i];
            atomicAdd(&comps[c], 1u);
            atomicAdd(&voxels[c], sz);          // a workgroup's roots own fewer than 2^31 voxels together
            offer(best[c], k, ((u64)sz << 32) | (u64)(0xffffffffu - (unsigned)i));
        }
    }
    __syncthreads();
    if (threadIdx.x < MAXC * MAXK) {
        const int c = threadIdx.x / MAXK;
        const u64 key = best[c][threadIdx.x % MAXK];
        if (c < cl.n && key) offer(stats + c * STATS + 3, keep_count(cl, c), key);
    }
    if (threadIdx.x < cl.n) {
        if (comps[threadIdx.x]) atomicAdd(stats + threadIdx.x * STATS, (u64)comps[threadIdx.x]);
        if (voxels[threadIdx.x]) atomicAdd(stats + threadIdx.x * STATS + 1, (u64)voxels[threadIdx.x]);
    }
}

// keys -> the table of mi3d.h: a component is kept iff its rank is below k and its size is at least min_size; sizes fall with the
// rank, so the kept ones are a prefix.  One thread per (sample, class).
__global__ __launch_bounds__(BLK) void finish_kernel(int rows, KeepClasses cl, int64_t min_size, int64_t* __restrict__ stats) {
    const int t = blockIdx.x * BLK + threadIdx.x;
    if (t >= rows) return;
    int64_t* s = stats + (int64_t)t * STATS;
    const int k = keep_count(cl, t % cl.n);
    int64_t kept = 0;
    for (int j = 0; j < MAXK; j++) {
        const u64 key = (u64)s[3 + j];
        const int64_t sz = (int64_t)(key >> 32);
        const bool keep = j < k && key != 0 && sz >= min_size;
        s[3 + j] = keep ? sz : 0;
        s[3 + MAXK + j] = keep ? (int64_t)(0xffffffffu - (unsigned)(key & 0xffffffffu)) : -1;
        kept += keep ? sz : 0;
    }
    s[2] = kept;
}

// ---- apply ------------------------------------------------------------------------------------------------------------------------
// One thread per voxel, which reads its own label and writes its own output: out may be lab.
template <typename T>
__global__ __launch_bounds__(BLK) void apply_kernel(const T* lab, T* out, Vol vol, KeepClasses cl, int fill,
                                                    const int32_t* __restrict__ root, const uint8_t* __restrict__ cls,
                                                    const int64_t* __restrict__ stats) {
    __shared__ int kept[MAXC][MAXK];
    if (threadIdx.x < MAXC * MAXK) {
        const int c = threadIdx.x / MAXK, j = threadIdx.x % MAXK;
        kept[c][j] = c < cl.n ? (int)stats[((int64_t)blockIdx.y * cl.n + c) * STATS + 3 + MAXK + j] : -1;
    }
    __syncthreads();
    const int64_t V = vol.V(), i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= V) return;
    int d, h, w;
    vol.split(i, d, h, w);
    const int64_t off = blockIdx.y * vol.sn + vol.offset(d, h, w);
    T l = lab[off];
    const int v = cls[blockIdx.y * V + i];
    if (v) {
        const int r = root[blockIdx.y * V + i];
        const int c = class_index(cl, v, 0);
        bool keep = false;
#pragma unroll
        for (int j = 0; j < MAXK; j++) keep = keep || kept[c][j] == r;
        if (!keep) l = (T)fill;
    }
    out[off] = l;
}

// ---- hole filling: ring and fill --------------------------------------------------------------------------------------------------
// The components here are those of the background (tile_kernel<T, Background>), and `code` is the C-ordered volume of label codes
// the tile pass left: the neighbours are read from it, never through the strides of the input.
// ring: lo[root] / hi[root] = the minimum / maximum code on the ring of the component, CODE_OUTSIDE for a ring position outside the
// volume.  The ring carries one value iff lo == hi, and no position outside iff hi < CODE_OUTSIDE: integer min and max, so the
// order of the atomics cannot matter.  A background voxel forms the min and max over its own non-background neighbours and issues an
// atomic only where a relaxed load shows it would change the word: the outer component of a real map has hundreds of thousands
// of ring voxels aimed at two addresses, and all but the first few end as a load.  Even those loads meet at one place, so a wave
// first combines the lanes that share a root.  One thread per voxel; grid: x over voxels, y = sample.
__global__ __launch_bounds__(BLK) void ring_kernel(Vol vol, int conn, const uint16_t* __restrict__ code, const int32_t* __restrict__ root,
                                                   int32_t* __restrict__ lo, int32_t* __restrict__ hi) {
    const int64_t V = vol.V(), i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    code += blockIdx.y * V;
    int mn = INT32_MAX, mx = 0;          // mx stays 0 where the voxel has nothing to tell: not background, or background all around
    if (i < V && code[i] == 0) {
        int d, h, w;
        vol.split(i, d, h, w);
        // a voxel on a face has a neighbour of every connectivity outside the volume
        if (d == 0 || h == 0 || w == 0 || d == vol.D - 1 || h == vol.H - 1 || w == vol.W - 1) mn = mx = CODE_OUTSIDE;
        for (int j = 0; j < 27; j++) {
            const int dd = j / 9 - 1, dh = j / 3 % 3 - 1, dw = j % 3 - 1;
            const int nd = d + dd, nh = h + dh, nw = w + dw;
            if (j == 13 || nonzeros(dd, dh, dw) > conn || nd < 0 || nd >= vol.D || nh < 0 || nh >= vol.H || nw < 0 || nw >= vol.W) continue;
            const int c = code[((int64_t)nd * vol.H + nh) * vol.W + nw];
            if (c == 0) continue;
            mn = c < mn ? c : mn;
            mx = c > mx ? c : mx;
        }
    }
    bool has = mx != 0;
    const int r = has ? root[blockIdx.y * V + i] : -1;
    lo += blockIdx.y * V, hi += blockIdx.y * V;
    // The lanes of a wave that report to one root first combine what they have (twice: the outer component and one more), and one
    // lane speaks for them; every lane of the wave takes part in the shuffles.  The lanes still left report on their own.
    for (int round = 0; round < 2; round++) {
        const u64 todo = __ballot(has);
        if (!todo) break;
        const int leader = __builtin_ctzll(todo), lr = __shfl(r, leader, 64);
        const bool same = has && r == lr;
        int a = same ? mn : INT32_MAX, b = same ? mx : 0;
        for (int off = 32; off > 0; off >>= 1) {
            const int a2 = __shfl_xor(a, off, 64), b2 = __shfl_xor(b, off, 64);
            a = a2 < a ? a2 : a;
            b = b2 > b ? b2 : b;
        }
        if (lane == leader) {
            if (g_load(lo + lr) > a) atomicMin(lo + lr, a);
            if (g_load(hi + lr) < b) atomicMax(hi + lr, b);
        }
        has = has && !same;
    }
    if (has) {
        if (g_load(lo + r) > mn) atomicMin(lo + r, mn);
        if (g_load(hi + r) < mx) atomicMax(hi + r, mx);
    }
}

// fill: a background voxel of an enclosed component whose ring carries the single listed value v, of at most max_size voxels
// (0: no limit), becomes v; every other voxel is copied.  A thread reads its own label and writes its own output: out may be lab.
// The voxel that is its component's root classifies it for the tables: counts per workgroup in LDS, then one integer atomic per
// workgroup and non-zero word.  summary row: enclosed, filled, mixed, skipped; stats row of class c: holes, voxels.
template <typename T>
__global__ __launch_bounds__(BLK) void fill_kernel(const T* lab, T* out, Vol vol, Classes cl, int64_t max_size, const uint16_t* __restrict__ code,
                                                   const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                   const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, u64* __restrict__ stats,
                                                   u64* __restrict__ summary) {
    __shared__ unsigned holes[MAXC], voxels[MAXC], kinds[4];
    if (threadIdx.x < MAXC) holes[threadIdx.x] = 0, voxels[threadIdx.x] = 0;
    if (threadIdx.x < 4) kinds[threadIdx.x] = 0;
    __syncthreads();
    const int64_t V = vol.V(), i = (int64_t)blockIdx.x * BLK + threadIdx.x, base = blockIdx.y * V;
    if (i < V) {
        int d, h, w;
        vol.split(i, d, h, w);
        const int64_t off = blockIdx.y * vol.sn + vol.offset(d, h, w);
        T l = lab[off];
        if (code[base + i] == 0) {
            const int r = root[base + i];
            const int a = lo[base + r], b = hi[base + r], sz = size[base + r];
            const bool enclosed = b < CODE_OUTSIDE, one = a == b;
            const int c = one ? class_index(cl, a) : -1;          // a listed class is in 1..255: never CODE_OTHER
            const bool fill = enclosed && c >= 0 && (max_size == 0 || sz <= max_size);
            if (fill) l = (T)a;
            if (r == (int)i && enclosed) {
                atomicAdd(&kinds[0], 1u);
                atomicAdd(&kinds[fill ? 1 : one ? 3 : 2], 1u);
                if (fill) {
                    atomicAdd(&holes[c], 1u);
                    atomicAdd(&voxels[c], (unsigned)sz);          // a workgroup's roots own fewer than 2^31 voxels together
                }
            }
        }
        out[off] = l;
    }
    __syncthreads();
    if (threadIdx.x < cl.n) {
        u64* row = stats + ((int64_t)blockIdx.y * cl.n + threadIdx.x) * 2;
        if (holes[threadIdx.x]) atomicAdd(row, (u64)holes[threadIdx.x]);
        if (voxels[threadIdx.x]) atomicAdd(row + 1, (u64)voxels[threadIdx.x]);
    }
    if (threadIdx.x < 4 && kinds[threadIdx.x]) atomicAdd(summary + (int64_t)blockIdx.y * 4 + threadIdx.x, (u64)kinds[threadIdx.x]);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
struct Workspace {          // the layout, once: mi3d_components_workspace_bytes counts it over a null base
    int32_t *parent, *root, *size;
    uint8_t* cls;
    size_t bytes;
    Workspace(void* base, int64_t NV) {
        Arena a{static_cast<char*>(base)};
        parent = a.take<int32_t>(NV), root = a.take<int32_t>(NV), size = a.take<int32_t>(NV), cls = a.take<uint8_t>(NV);
        bytes = a.used;
    }
};
struct FillWorkspace : Workspace {          // mi3d_fill_holes_workspace_bytes: the same, then the code volume and the ring words per root
    uint16_t* code;
    int32_t *lo, *hi;
    FillWorkspace(void* base, int64_t NV) : Workspace(base, NV) {
        Arena a{static_cast<char*>(base), bytes};
        code = a.take<uint16_t>(NV), lo = a.take<int32_t>(NV), hi = a.take<int32_t>(NV);
        bytes = a.used;
    }
};

int check_common(const char* name, const void* labels, int label_dtype, int N, int D, int H, int W, int64_t sn, int64_t sd, int64_t sh,
                 int64_t sw, int connectivity, const int32_t* status_out, const void* workspace, size_t workspace_bytes_given, bool fill = false) {
    MI3D_TRY(check_map(name, "labels", labels, label_dtype, sn, sd, sh, sw));
    MI3D_TRY(check_sizes(name, N, D, H, W));
    MI3D_TRY(check_connectivity(name, connectivity));
    MI3D_CHECK_ARG(status_out, "%s: null pointer (status_out)", name);
    const int64_t NV = total_voxels(N, D, H, W);
    return check_workspace(name, workspace, workspace_bytes_given, fill ? FillWorkspace(nullptr, NV).bytes : Workspace(nullptr, NV).bytes);
}

// status = 0, then tile pass, seam pass, flatten into `root` (and the sizes where size != NULL)
template <typename Map>
int label_launch(const void* labels, int label_dtype, const Vol& vol, const Map& map, int conn, const Workspace& ws, int32_t* root,
                 int32_t* size, int32_t* status, hipStream_t stream) {
    MI3D_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), stream));
    const int tilesW = cdiv(vol.W, TW), tilesH = cdiv(vol.H, TH), tilesD = cdiv(vol.D, TD);
    const int64_t tiles = (int64_t)tilesW * tilesH * tilesD;          // <= V < 2^31
    dim3 tgrid((unsigned)tiles, (unsigned)vol.N), vgrid((unsigned)voxel_blocks(vol.V()), (unsigned)vol.N);
    dispatch_src(label_dtype, LabelTypes(), [&](auto tag) {
        tile_kernel<<<tgrid, BLK, 0, stream>>>((const decltype(tag)*)labels, vol, map, conn, tilesW, tilesH, ws.parent, ws.cls, size, status);
    });
    MI3D_LAUNCH_CHECK();
    if (tiles > 1) {
        seam_kernel<<<vgrid, BLK, 0, stream>>>(vol, conn, ws.parent, ws.cls, status);
        MI3D_LAUNCH_CHECK();
    }
    flatten_kernel<<<vgrid, BLK, 0, stream>>>(vol, ws.parent, root, size, status);
    MI3D_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" {

size_t mi3d_components_workspace_bytes(int N, int D, int H, int W) {
    const int64_t NV = total_voxels(N, D, H, W);
    if (NV == 0) {
        mi3d_set_error("mi3d_components_workspace_bytes: N in [1, 65535], sides >= 1 and D * H * W < 2^31 expected");
        return 0;
    }
    return Workspace(nullptr, NV).bytes;
}

int mi3d_component_roots(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d,
                         int64_t stride_h, int64_t stride_w, int connectivity, const uint8_t* class_select, int32_t* roots_out,
                         int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = "mi3d_component_roots";
    MI3D_TRY(check_common(name, labels, label_dtype, N, D, H, W, stride_n, stride_d, stride_h, stride_w, connectivity, status_out,
                          workspace, workspace_bytes));
    MI3D_CHECK_ARG(class_select && roots_out, "%s: null pointer", name);
    MI3D_CHECK_ARG(class_select[0] == 0, "%s: value 0 is the background and cannot be selected", name);
    KeepSelected keep{};
    Select& sel = keep.sel;
    for (int v = 1; v < 256; v++)
        if (class_select[v]) sel.m[v >> 6] |= 1ull << (v & 63);
    const Vol vol{N, D, H, W, stride_n, stride_d, stride_h, stride_w};
    return label_launch(labels, label_dtype, vol, keep, connectivity, Workspace(workspace, (int64_t)N * vol.V()), roots_out, nullptr, status_out,
                        (hipStream_t)stream);
}

int mi3d_keep_components(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d,
                         int64_t stride_h, int64_t stride_w, int connectivity, int n_classes, const int32_t* class_values,
                         const int32_t* keep_k, int64_t min_size, int fill, void* labels_out, int64_t* stats_out, int32_t* status_out,
                         void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = "mi3d_keep_components";
    MI3D_TRY(check_common(name, labels, label_dtype, N, D, H, W, stride_n, stride_d, stride_h, stride_w, connectivity, status_out,
                          workspace, workspace_bytes));
    MI3D_CHECK_ARG(class_values && keep_k && labels_out && stats_out, "%s: null pointer", name);
    MI3D_CHECK_ARG(((uintptr_t)stats_out & 7) == 0, "%s: stats_out must be 8-byte aligned", name);
    MI3D_CHECK_ARG(min_size >= 1, "%s: min_size must be at least 1", name);
    MI3D_CHECK_ARG(fill >= 0 && fill <= 255, "%s: fill %d outside 0..255", name, fill);
    KeepSelected keep{};
    Select& sel = keep.sel;
    KeepClasses cl{};
    MI3D_TRY(check_classes(name, n_classes, class_values, cl));
    for (int j = 0; j < n_classes; j++) {
        const int v = class_values[j], k = keep_k[j];
        MI3D_CHECK_ARG(v >= 1 && v <= 255, "%s: class value %d outside 1..255", name, v);
        MI3D_CHECK_ARG(k >= 1 && k <= MAXK, "%s: keep count %d of class %d outside 1..%d", name, k, v, MAXK);
        sel.m[v >> 6] |= 1ull << (v & 63);
        cl.k[j] = k;
    }
    const Vol vol{N, D, H, W, stride_n, stride_d, stride_h, stride_w};
    const Workspace ws(workspace, (int64_t)N * vol.V());
    hipStream_t s = (hipStream_t)stream;
    MI3D_HIP(hipMemsetAsync(stats_out, 0, (size_t)N * n_classes * STATS * sizeof(int64_t), s));
    MI3D_TRY(label_launch(labels, label_dtype, vol, keep, connectivity, ws, ws.root, ws.size, status_out, s));
    dim3 vgrid((unsigned)voxel_blocks(vol.V()), (unsigned)N);
    dim3 sgrid(vgrid.x < SELECT_BLOCKS ? vgrid.x : SELECT_BLOCKS, (unsigned)N);
    select_kernel<<<sgrid, BLK, 0, s>>>(vol, cl, ws.root, ws.size, ws.cls, (u64*)stats_out);
    MI3D_LAUNCH_CHECK();
    finish_kernel<<<cdiv(N * n_classes, BLK), BLK, 0, s>>>(N * n_classes, cl, min_size, stats_out);
    MI3D_LAUNCH_CHECK();
    dispatch_src(label_dtype, LabelTypes(), [&](auto tag) {
        using T = decltype(tag);
        apply_kernel<T><<<vgrid, BLK, 0, s>>>((const T*)labels, (T*)labels_out, vol, cl, fill, ws.root, ws.cls, stats_out);
    });
    MI3D_LAUNCH_CHECK();
    return 0;
}

size_t mi3d_fill_holes_workspace_bytes(int N, int D, int H, int W) {
    const int64_t NV = total_voxels(N, D, H, W);
    if (NV == 0) {
        mi3d_set_error("mi3d_fill_holes_workspace_bytes: N in [1, 65535], sides >= 1 and D * H * W < 2^31 expected");
        return 0;
    }
    return FillWorkspace(nullptr, NV).bytes;
}

int mi3d_fill_holes(const void* labels, int label_dtype, int N, int D, int H, int W, int64_t stride_n, int64_t stride_d, int64_t stride_h,
                    int64_t stride_w, int connectivity, int n_classes, const int32_t* class_values, int64_t max_size, void* labels_out,
                    int64_t* stats_out, int64_t* summary_out, int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = "mi3d_fill_holes";
    MI3D_TRY(check_common(name, labels, label_dtype, N, D, H, W, stride_n, stride_d, stride_h, stride_w, connectivity, status_out,
                          workspace, workspace_bytes, true));
    MI3D_CHECK_ARG(class_values && labels_out && stats_out && summary_out, "%s: null pointer", name);
    MI3D_CHECK_ARG((((uintptr_t)stats_out | (uintptr_t)summary_out) & 7) == 0, "%s: stats_out and summary_out must be 8-byte aligned", name);
    MI3D_CHECK_ARG(max_size >= 0, "%s: max_size must be at least 0 (0: no limit)", name);
    Classes cl{};
    MI3D_TRY(check_classes(name, n_classes, class_values, cl));
    for (int j = 0; j < n_classes; j++)
        MI3D_CHECK_ARG(cl.value[j] >= 1 && cl.value[j] <= 255, "%s: class value %d outside 1..255", name, cl.value[j]);
    const Vol vol{N, D, H, W, stride_n, stride_d, stride_h, stride_w};
    const int64_t NV = (int64_t)N * vol.V();
    const FillWorkspace ws(workspace, NV);
    hipStream_t s = (hipStream_t)stream;
    MI3D_HIP(hipMemsetAsync(stats_out, 0, (size_t)N * n_classes * 2 * sizeof(int64_t), s));
    MI3D_HIP(hipMemsetAsync(summary_out, 0, (size_t)N * 4 * sizeof(int64_t), s));
    MI3D_HIP(hipMemsetAsync(ws.lo, 0x7f, (size_t)NV * sizeof(int32_t), s));          // 0x7f7f7f7f: above every code
    MI3D_HIP(hipMemsetAsync(ws.hi, 0, (size_t)NV * sizeof(int32_t), s));             // below every code of a ring
    MI3D_TRY(label_launch(labels, label_dtype, vol, Background{ws.code}, connectivity, ws, ws.root, ws.size, status_out, s));
    dim3 vgrid((unsigned)voxel_blocks(vol.V()), (unsigned)N);
    ring_kernel<<<vgrid, BLK, 0, s>>>(vol, connectivity, ws.code, ws.root, ws.lo, ws.hi);
    MI3D_LAUNCH_CHECK();
    dispatch_src(label_dtype, LabelTypes(), [&](auto tag) {
        using T = decltype(tag);
        fill_kernel<T><<<vgrid, BLK, 0, s>>>((const T*)labels, (T*)labels_out, vol, cl, max_size, ws.code, ws.root, ws.size, ws.lo, ws.hi,
                                             (u64*)stats_out, (u64*)summary_out);
    });
    MI3D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
