// scratch.h — what scratch one conv layer / one decoder up step needs, as plain numbers, and the running offset every workspace
// layout of plan.hip and api.hip is cut with.  Host code only: nothing here allocates, launches or touches the device.
#pragma once
#include "ops.h"

// Consecutive areas of one workspace, each on a 256-byte boundary: take() returns the area's offset, off is the size taken so far.
// (The label-map files have a pointer-returning Arena of their own in volume.h's unnamed namespace; no file includes both headers.)
struct Arena {
    size_t off = 0;
    size_t take(size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; }
};

// One 3x3x3 conv layer whose activations have dtype dt, at geometry g: its route class and the scratch the kernels of that class use.
// The ONE place that asks the kernel files for these sizes: build_plan takes maxima over the layers, an entry lays one layer out.
struct ConvScratch {
    bool mfma, c1;                     // conv3_layer_class
    size_t wpf_bytes, wpd_bytes;       // packed weight images: forward, input gradient (mfma: bf16 MFMA images, else the direct floats)
    int stat_rows;                     // BatchNorm partial rows of [2][Cout] floats the forward conv's epilogue writes (1: none)
    size_t splitk_fwd_floats;          // split-K partials of the forward conv (Cin -> Cout); 0: single pass or not MFMA
    size_t splitk_bwd_floats;          // the same for the input-gradient conv (Cout -> Cin)
    size_t wgrad_floats;               // weight-gradient slabs of the kernel the class runs (MFMA, first layer, or direct)
};
inline ConvScratch conv3_scratch(int dt, int Cin, int Cout, Geo g) {
    ConvScratch S;
    conv3_layer_class(dt, Cin, Cout, S.mfma, S.c1);
    S.wpf_bytes = S.mfma ? conv3_mfma_pack_elems(Cin, Cout) * 2 : conv3_direct_pack_floats(Cin, Cout) * sizeof(float);
    S.wpd_bytes = S.mfma ? conv3_mfma_pack_elems(Cin, Cout) * 2 : conv3_direct_pack_floats(Cout, Cin) * sizeof(float);
    S.stat_rows = S.mfma ? conv3_mfma_stat_blocks(Cin, Cout, g) : S.c1 ? conv3_c1_fwd_stat_blocks(g) : 1;
    S.splitk_fwd_floats = S.mfma ? conv3_mfma_splitk_floats(Cin, Cout, g) : 0;
    S.splitk_bwd_floats = S.mfma ? conv3_mfma_splitk_floats(Cout, Cin, g) : 0;
    S.wgrad_floats = (S.mfma || S.c1) ? conv3_mfma_wgrad_ws_floats(Cin, Cout, g) : conv3_direct_wgrad_ws_floats(Cin, Cout, g);
    return S;
}
// the same layer on the direct fp32-FMA kernels (the fp32 class): where an entry lands when the caller's strides rule the others out
inline ConvScratch conv3_scratch_direct(int Cin, int Cout, Geo g) { return conv3_scratch(MI3D_F32, Cin, Cout, g); }

// One decoder up step (ConvTranspose3d k=2 s=2) at INPUT geometry g.  mfma: the class at the plan's strides (multiples of 8)
struct UpScratch {
    bool mfma;
    size_t pack_bytes, wgrad_floats;                   // weight images and slabs of the class's kernels
    size_t direct_pack_bytes, direct_wgrad_floats;     // the same of the direct kernels (the images: never smaller than the MFMA ones)
};
inline UpScratch upconv2_scratch(int dt, int Cin, int Cout, Geo g) {
    UpScratch S;
    S.mfma = dt == MI3D_BF16 && upconv2_mfma_supported(Cin, Cout, 8, 8);
    S.direct_pack_bytes = upconv2_pack_floats(Cin, Cout) * sizeof(float);
    S.direct_wgrad_floats = upconv2_bwd_ws_floats(Cin, Cout, g);
    S.pack_bytes = S.mfma ? upconv2_mfma_pack_elems(Cin, Cout) * 2 : S.direct_pack_bytes;
    S.wgrad_floats = S.mfma ? upconv2_mfma_bwd_ws_floats(Cin, Cout, g) : S.direct_wgrad_floats;
    return S;
}
