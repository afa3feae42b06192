// volume.h — what the kernels on stored label maps and scans share (components, surface, preview, resample, patch): the strided volume
// view, the listed-class table, the workspace arena, the host argument checks and the source-dtype dispatch.  Integer code and plain
// additions only: nothing here depends on the floating-point contraction mode of the file that includes it.
#pragma once
#include "ops.h"
#include "../../include/mi3d.h"

namespace {
constexpr int VOL_BLK = 256;           // threads per workgroup of every kernel that walks voxels
constexpr int MAX_SIDE = 65535;        // a side that rides in gridDim.y; in-plane indices stay far inside int32

// (N, D, H, W) samples of a label map seen through element strides.  A voxel's index is d * H * W + h * W + w in its sample.
struct Vol {
    int N, D, H, W;
    int64_t sn, sd, sh, sw;
    MI3D_HD int64_t V() const { return (int64_t)D * H * W; }
    MI3D_HD void split(int64_t i, int& d, int& h, int& w) const { w = (int)(i % W), h = (int)(i / W % H), d = (int)(i / ((int64_t)W * H)); }
    MI3D_HD int64_t offset(int d, int h, int w) const { return d * sd + h * sh + w * sw; }          // within a sample
};

// The listed classes of an entry, by value in the kernel arguments; the keep counts of mi3d_keep_components ride beside them.
struct Classes {
    int n, value[MI3D_COMPONENTS_MAX_CLASSES];
};
struct KeepClasses : Classes {
    int k[MI3D_COMPONENTS_MAX_CLASSES];
};
// the index of the listed class whose value is v, `missing` where none is: unrolled selects, no indexing of the kernel's arguments
template <typename T> __device__ __forceinline__ int class_index(const Classes& cl, T v, int missing = -1) {
    int c = missing;
#pragma unroll
    for (int j = 0; j < MI3D_COMPONENTS_MAX_CLASSES; j++)
        if (j < cl.n && (T)cl.value[j] == v) c = j;
    return c;
}
// the same, and the keep count of that class (0 where none is) from the same selects: select_kernel needs both per root
template <typename T> __device__ __forceinline__ int class_index(const KeepClasses& cl, T v, int& k) {
    int c = -1;
    k = 0;
#pragma unroll
    for (int j = 0; j < MI3D_COMPONENTS_MAX_CLASSES; j++)
        if (j < cl.n && (T)cl.value[j] == v) c = j, k = cl.k[j];
    return c;
}
// how many of a neighbour offset's coordinates are not 0: the offset is part of connectivity c iff at most c are
__device__ __forceinline__ int nonzeros(int dd, int dh, int dw) { return (dd != 0) + (dh != 0) + (dw != 0); }

// The sum of x over a workgroup of VOL_BLK threads in a fixed order, in two steps around the caller's __syncthreads(): every thread
// puts its wave's sum (a __shfl_down tree) into the wave's LDS word; then one thread adds the words in ascending order.
__device__ __forceinline__ void block_sum_fixed_put(double x, double (&wave_sum)[VOL_BLK / 64]) {
    for (int off = 32; off > 0; off >>= 1) x = x + __shfl_down(x, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = x;
}
__device__ __forceinline__ double block_sum_fixed_get(const double (&wave_sum)[VOL_BLK / 64]) {
    double sum = wave_sum[0];
    for (int v = 1; v < VOL_BLK / 64; v++) sum = sum + wave_sum[v];
    return sum;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int64_t voxel_blocks(int64_t V) { return (V + VOL_BLK - 1) / VOL_BLK; }

// total voxels, or 0 where the sizes are outside the library's range
int64_t total_voxels(int N, int D, int H, int W) {
    if (N < 1 || N > 65535 || D < 1 || H < 1 || W < 1) return 0;
    const int64_t V = (int64_t)D * H * W;
    if ((int64_t)D * H >= ((int64_t)1 << 31) || V >= ((int64_t)1 << 31)) return 0;
    return N * V;          // < 2^47
}
// A single volume's sides and strides: a stride is positive and leaves the last element's offset far inside int64 (65535^3 < 2^48)
bool sides_ok(int a, int b, int c) { return a >= 1 && b >= 1 && c >= 1 && a <= MAX_SIDE && b <= MAX_SIDE && c <= MAX_SIDE; }
bool strides_ok(int64_t a, int64_t b, int64_t c) {
    const int64_t lim = (int64_t)1 << 44;
    return a >= 1 && b >= 1 && c >= 1 && a < lim && b < lim && c < lim;
}

// A workspace handed out in 256-byte aligned parts in the order of the take() calls; over a null base it only counts the bytes, so
// an entry writes its layout once, for its *_workspace_bytes query and for the launch.
struct Arena {
    char* base;
    size_t used = 0;
    template <typename T> T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += align256(count * sizeof(T));
        return p;
    }
};

// The argument checks of the label-map entries; name: the entry, which: the argument.
int check_map(const char* name, const char* which, const void* labels, int dtype, int64_t sn, int64_t sd, int64_t sh, int64_t sw) {
    MI3D_CHECK_ARG(labels, "%s: null pointer (%s)", name, which);
    MI3D_CHECK_ARG(dtype == MI3D_SRC_U8 || dtype == MI3D_SRC_I64, "%s: %s is uint8 or int64, not dtype code %d", name, which, dtype);
    MI3D_CHECK_ARG(sn >= 1 && sd >= 1 && sh >= 1 && sw >= 1, "%s: the strides of %s must be positive element counts", name, which);
    return 0;
}
int check_sizes(const char* name, int N, int D, int H, int W) {
    MI3D_CHECK_ARG(total_voxels(N, D, H, W) > 0, "%s: N in [1, 65535], sides >= 1 and D * H * W < 2^31 expected, got %d x (%d, %d, %d)", name, N, D, H, W);
    return 0;
}
int check_connectivity(const char* name, int connectivity) {
    MI3D_CHECK_ARG(connectivity >= 1 && connectivity <= 3, "%s: connectivity %d is not 1, 2 or 3", name, connectivity);
    return 0;
}
int check_classes(const char* name, int n, const int32_t* values, Classes& cl) {          // 1 to MAX_CLASSES distinct values -> cl
    MI3D_CHECK_ARG(n >= 1 && n <= MI3D_COMPONENTS_MAX_CLASSES, "%s: 1 to %d classes, got %d", name, MI3D_COMPONENTS_MAX_CLASSES, n);
    MI3D_CHECK_ARG(values, "%s: null pointer (class_values)", name);
    cl.n = n;
    for (int j = 0; j < n; j++) {
        for (int k = 0; k < j; k++) MI3D_CHECK_ARG(values[k] != values[j], "%s: class value %d listed twice", name, values[j]);
        cl.value[j] = values[j];
    }
    return 0;
}
int check_workspace(const char* name, const void* workspace, size_t given, size_t needed) {
    MI3D_CHECK_ARG(workspace, "%s: null pointer (workspace)", name);
    MI3D_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", name);
    MI3D_CHECK_ARG(given >= needed, "%s: workspace of %zu bytes, %zu needed", name, given, needed);
    return 0;
}

// Source-dtype dispatch: f(S()) for the one type S of the list whose MI3D_SRC_* code is `code`; false where none is
template <typename S> constexpr int src_code = -1;
template <> constexpr int src_code<uint8_t> = MI3D_SRC_U8;
template <> constexpr int src_code<int16_t> = MI3D_SRC_I16;
template <> constexpr int src_code<float> = MI3D_SRC_F32;
template <> constexpr int src_code<int64_t> = MI3D_SRC_I64;
template <typename... S> struct Types {};
template <typename... S, typename F> bool dispatch_src(int code, Types<S...>, F&& f) {
    return ((code == src_code<S> && (f(S()), true)) || ...);
}
typedef Types<uint8_t, int64_t> LabelTypes;          // what check_map lets through
}  // namespace
