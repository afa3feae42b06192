"""What the label-map entries share (csrc/volume.h, _volume.py), no GPU needed: the workspace queries against the layouts they are
defined by, and the text of the argument errors raised before anything touches a device."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_segmentation_project_amd import _lib, components, preview, surface  # noqa: E402
from multimodal_segmentation_project_amd._lib import Mi3dError  # noqa: E402


def align256(b):
    return (b + 255) & ~255


def components_bytes(n, d, h, w):
    nv = n * d * h * w
    return 3 * align256(4 * nv) + align256(nv)


def surface_bytes(n, d, h, w):
    v = d * h * w
    return 2 * align256(n * v) + 2 * align256(16 * n * v) + align256(16 * n * ((v + 255) // 256)) + align256(32 * n)


# V a multiple of 256 and not, N > 1, one voxel, a row of one ballot word plus one, the largest sample under 2^31 voxels
SHAPES = [(1, 4, 8, 8), (1, 3, 5, 7), (2, 9, 10, 70), (3, 1, 1, 1), (5, 2, 3, 65), (65535, 1, 1, 3), (1, 2047, 1024, 1024)]
REFUSED = [(0, 4, 4, 4), (65536, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0), (1, 2048, 1024, 1024), (2, 1, 65536, 32768)]


@pytest.mark.parametrize("shape", SHAPES)
def test_workspace_queries_equal_the_documented_layouts(shape):
    lib = _lib.lib()
    assert lib.mi3d_components_workspace_bytes(*shape) == components_bytes(*shape)
    for n_classes in (1, 3, 8):
        assert lib.mi3d_surface_workspace_bytes(*shape, n_classes) == surface_bytes(*shape)


@pytest.mark.parametrize("shape", REFUSED)
def test_workspace_queries_refuse_sizes_outside_the_range(shape):
    lib = _lib.lib()
    assert lib.mi3d_components_workspace_bytes(*shape) == 0
    assert lib.mi3d_last_error().startswith(b"mi3d_components_workspace_bytes: N in [1, 65535]")
    assert lib.mi3d_surface_workspace_bytes(*shape, 3) == 0
    assert lib.mi3d_last_error().startswith(b"mi3d_surface_workspace_bytes: N in [1, 65535]")


@pytest.mark.parametrize("n_classes", [0, 9, -1])
def test_surface_workspace_query_refuses_the_class_count(n_classes):
    lib = _lib.lib()
    assert lib.mi3d_surface_workspace_bytes(2, 9, 10, 70, n_classes) == 0
    assert b"1 to 8 classes expected" in lib.mi3d_last_error()


U8 = torch.zeros((2, 4, 5, 6), dtype=torch.uint8)
F32 = torch.zeros((4, 5, 6), dtype=torch.float32)
OVERLAP = torch.zeros((4, 5, 6), dtype=torch.uint8)[None].expand(2, 4, 5, 6)
CPU = "tensor is on cpu; the MI355X HIP path needs GPU tensors (no CPU fallback)"
DENSE = ": a permutation of a contiguous array is expected, without padding, overlap or stride 0"

# (call, the message): every text is the one the modules raised before _volume.py existed
ERRORS = {
    "keep_largest/dtype": (lambda: components.keep_largest(U8.float()), "keep_largest: labels are torch.uint8 or torch.int64, got torch.float32"),
    "keep_largest/dense": (lambda: components.keep_largest(U8[:, :, ::2]),
                           f"keep_largest: the tensor is not dense (shape (4, 3, 6), strides (30, 12, 1)){DENSE}"),
    "keep_largest/rank": (lambda: components.keep_largest(U8[0, 0]),
                          "keep_largest: a (D, H, W) or (N, D, H, W) label volume expected, got (5, 6)"),
    "keep_largest/connectivity": (lambda: components.keep_largest(U8, connectivity=4),
                                  "keep_largest: connectivity 4 is not 1, 2 or 3 (6, 18 or 26 neighbours)"),
    "keep_largest/overlap": (lambda: components.keep_largest(OVERLAP),
                             "keep_largest: samples overlap (shape (2, 4, 5, 6), strides (0, 30, 6, 1))"),
    "keep_largest/class": (lambda: components.keep_largest(U8, keep={300: 1}), "keep_largest: class 300 cannot be listed: values 1..255 can"),
    "keep_largest/cpu": (lambda: components.keep_largest(U8), f"keep_largest: {CPU}"),
    "component_roots/dtype": (lambda: components.component_roots(U8.to(torch.int32)),
                              "component_roots: labels are torch.uint8 or torch.int64, got torch.int32"),
    "component_roots/dense": (lambda: components.component_roots(U8[0, :, :, ::2]),
                              f"component_roots: the tensor is not dense (shape (4, 5, 3), strides (30, 6, 2)){DENSE}"),
    "component_roots/rank": (lambda: components.component_roots(U8[None]),
                             "component_roots: a (D, H, W) or (N, D, H, W) label volume expected, got (1, 2, 4, 5, 6)"),
    "component_roots/connectivity": (lambda: components.component_roots(U8, connectivity=4),
                                     "component_roots: connectivity 4 is not 1, 2 or 3 (6, 18 or 26 neighbours)"),
    "component_roots/overlap": (lambda: components.component_roots(OVERLAP),
                                "component_roots: samples overlap (shape (2, 4, 5, 6), strides (0, 30, 6, 1))"),
    "component_roots/class": (lambda: components.component_roots(U8, classes=(0,)),
                              "component_roots: class 0 cannot be selected: values 1..255 can"),
    "component_roots/cpu": (lambda: components.component_roots(U8.long()), f"component_roots: {CPU}"),
    "surface_distances/dtype": (lambda: surface.surface_distances(U8, U8.float()),
                                "surface_distances: labels are torch.uint8 or torch.int64, got torch.float32"),
    "surface_distances/dense": (lambda: surface.surface_distances(U8[:, ::2], U8[:, ::2]),
                                f"surface_distances: the tensor is not dense (shape (2, 5, 6), strides (60, 6, 1)){DENSE}"),
    "surface_distances/rank": (lambda: surface.surface_distances(U8[0, 0], U8[0, 0]),
                               "surface_distances: a (D, H, W) or (N, D, H, W) label volume expected, got (5, 6)"),
    "surface_distances/connectivity": (lambda: surface.surface_distances(U8, U8, connectivity=4),
                                       "surface_distances: connectivity 4 is not 1, 2 or 3 (6, 18 or 26 neighbours)"),
    "surface_distances/overlap": (lambda: surface.surface_distances(U8, OVERLAP),
                                  "surface_distances: samples overlap (shape (2, 4, 5, 6), strides (0, 30, 6, 1))"),
    "surface_distances/class": (lambda: surface.surface_distances(U8, U8, classes=(1, 2 ** 31)),
                                "surface_distances: class 2147483648 is not a 32-bit value"),
    "surface_distances/cpu": (lambda: surface.surface_distances(U8, U8.long()), f"surface_distances: {CPU}"),
    "surface_mask/dtype": (lambda: surface.surface_mask(U8.to(torch.int16), 1),
                           "surface_mask: labels are torch.uint8 or torch.int64, got torch.int16"),
    "surface_mask/dense": (lambda: surface.surface_mask(U8[:, :, ::2], 1), f"surface_mask: the tensor is not dense (shape (4, 3, 6), strides (30, 12, 1)){DENSE}"),
    "surface_mask/rank": (lambda: surface.surface_mask(U8[0, 0, 0], 1),
                          "surface_mask: a (D, H, W) or (N, D, H, W) label volume expected, got (6,)"),
    "surface_mask/connectivity": (lambda: surface.surface_mask(U8, 1, connectivity=4),
                                  "surface_mask: connectivity 4 is not 1, 2 or 3 (6, 18 or 26 neighbours)"),
    "surface_mask/overlap": (lambda: surface.surface_mask(OVERLAP, 1), "surface_mask: samples overlap (shape (2, 4, 5, 6), strides (0, 30, 6, 1))"),
    "surface_mask/class": (lambda: surface.surface_mask(U8, -2 ** 31 - 1), "surface_mask: class -2147483649 is not a 32-bit value"),
    "surface_mask/cpu": (lambda: surface.surface_mask(U8, 1), f"surface_mask: {CPU}"),
    "distance_to/dtype": (lambda: surface.distance_to(F32), "distance_to: labels are torch.uint8 or torch.int64, got torch.float32"),
    "distance_to/dense": (lambda: surface.distance_to(U8[:, ::2]), f"distance_to: the tensor is not dense (shape (2, 5, 6), strides (60, 6, 1)){DENSE}"),
    "distance_to/rank": (lambda: surface.distance_to(U8[0, 0]), "distance_to: a (D, H, W) or (N, D, H, W) label volume expected, got (5, 6)"),
    "distance_to/overlap": (lambda: surface.distance_to(OVERLAP), "distance_to: samples overlap (shape (2, 4, 5, 6), strides (0, 30, 6, 1))"),
    "distance_to/cpu": (lambda: surface.distance_to(U8 > 0), f"distance_to: {CPU}"),
    "foreground_profiles/dtype": (lambda: preview.foreground_profiles(F32),
                                  "foreground_profiles: the label is torch.uint8 or torch.int64, got torch.float32"),
    "foreground_profiles/dense": (lambda: preview.foreground_profiles(U8[0, :, ::2]),
                                  f"foreground_profiles: the tensor is not dense (shape (4, 3, 6), strides (30, 12, 1)){DENSE}"),
    "foreground_profiles/rank": (lambda: preview.foreground_profiles(U8),
                                 "foreground_profiles: one 3-D label volume (leading singleton dims aside) expected, got (2, 4, 5, 6)"),
    "foreground_profiles/cpu": (lambda: preview.foreground_profiles(U8[:1]), f"foreground_profiles: {CPU}"),
    "overlay_slice/dtype": (lambda: preview.overlay_slice(F32.double(), U8[0], 0, 0),
                            "overlay_slice: the image is torch.float32 or torch.int16, got torch.float64"),
    "overlay_slice/label_dtype": (lambda: preview.overlay_slice(F32, F32, 0, 0),
                                  "overlay_slice: the label is torch.uint8 or torch.int64, got torch.float32"),
    "overlay_slice/dense": (lambda: preview.overlay_slice(F32, U8[0, :, :, ::2], 0, 0),
                            f"overlay_slice: the tensor is not dense (shape (4, 5, 3), strides (30, 6, 2)){DENSE}"),
    "overlay_slice/rank": (lambda: preview.overlay_slice(F32[0], U8[0], 0, 0),
                           "overlay_slice: one 3-D image volume (leading singleton dims aside) expected, got (5, 6)"),
    "overlay_slice/cpu": (lambda: preview.overlay_slice(F32, U8[0], 2, 5), f"overlay_slice: {CPU}"),
}


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_argument_errors_keep_their_text(case):
    fn, message = ERRORS[case]
    before = _lib.launches
    with pytest.raises(Mi3dError) as e:
        fn()
    assert str(e.value) == message
    assert _lib.launches == before
