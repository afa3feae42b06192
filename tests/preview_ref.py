"""numpy restatement of the reference's preview figure (visualize_prediction, test_model.py:66-193) and of the slider of
visualize_nifti.py:29-52: the yardstick of preview.py and csrc/preview.hip.  test_preview_cpu.py pins it to the arrays the
reference itself handed to imshow (tests/golden/preview.npz, tools/gen_golden.py --only preview).

  foreground_profiles(label)            np.sum(label > 0, axis=others) per axis (find_best_slice, :77-82)
  best_slices(label)                    np.argmax of each, n // 2 where the maximum is 0 (:85-89)
  take_slice(volume, axis, k)           the 2-D slice the figure draws: volume[k, :, :], volume[:, k, :] or volume[:, :, k]
  overlay(image_slice, label_slice)     create_overlay (:103-125), float64 (A, B, 3)
  as_dtype(overlay, dtype)              float64 as it is, float32 one rounding, uint8 (255 * value).astype(np.uint8) with NaN -> 0
  panels(image, label, pred)            the nine arrays in figure order and the three slice indices by axis
  overlay_stack(image, label, axis)     float64 (n, A, B, 3): overlay of every slice of the axis
"""
import numpy as np

SHAPES = ((5, 7, 9), (17, 33, 65), (3, 130, 67), (4, 6, 300), (300, 5, 6))
CASES = ("random", "tie", "background", "last", "big_label", "flat")
VIEW_AXES = (2, 0, 1)          # figure rows: axial, sagittal, coronal (test_model.py:94-96)
COLOURS = {1: (1.0, 0.0, 0.0), 2: (1.0, 0.65, 0.0), 3: (0.0, 0.5, 0.0)}
# what the fixture holds from the reference itself: the random case on four shapes ((3, 130, 67) alone would be half a megabyte of
# float64 panels), every other case on the smallest; the GPU tests run every case on every shape against this restatement
RECORDED = tuple(("random", s) for s in SHAPES if s != (3, 130, 67)) + tuple((c, SHAPES[0]) for c in CASES[1:])


def key(case, shape):
    return f"{case}/" + "x".join(str(n) for n in shape)


def make_case(case, shape):
    """(float32 image, int64 label, uint8 pred) of one case, seeded by its key.  The image has few mantissa bits (eighths), so the
    fixture compresses; the grey values (v - min) / (max - min) are full doubles all the same."""
    rng = np.random.default_rng(sum(key(case, shape).encode()) + 1000 * CASES.index(case))
    image = (np.round(rng.normal(0.0, 300.0, shape) * 8) / 8).astype(np.float32)
    pred = rng.integers(0, 4, shape).astype(np.uint8)
    label = np.zeros(shape, dtype=np.int64)              # "background": the middle slice n // 2 on every axis
    if case in ("random", "flat"):
        label = rng.integers(0, 4, shape)
    elif case == "tie":                                  # two slices of every axis hold four voxels each: the earlier one wins
        lo = [max(n // 3, 1) for n in shape]
        label[np.ix_(*[(a, n - 1) for a, n in zip(lo, shape)])] = rng.integers(1, 4, (2, 2, 2))
    elif case == "last":                                 # foreground in the last slice of every axis only
        label[-1, -1, -1] = 2
    elif case == "big_label":                            # values >= 4 count as foreground and stay grey
        label = rng.integers(0, 7, shape)
        label[rng.random(shape) < 0.05] = 255
        pred = rng.integers(0, 6, shape).astype(np.uint8)
    if case == "flat":                                   # the three chosen slices are constant: 0 / 0 wherever no colour lands
        best = best_slices(label)
        image[best[0], :, :] = image[:, best[1], :] = image[:, :, best[2]] = 7.5
    return image, label, pred


def foreground_profiles(label):
    fg = np.asarray(label) > 0
    return [np.sum(fg, axis=tuple(b for b in range(3) if b != a)).astype(np.int64) for a in range(3)]


def best_slices(label):
    out = []
    for a, c in enumerate(foreground_profiles(label)):
        k = int(np.argmax(c))
        out.append(k if c[k] > 0 else label.shape[a] // 2)
    return np.array(out, dtype=np.int32)


def take_slice(volume, axis, k):
    return np.take(volume, int(k), axis=axis)


def overlay(image_slice, label_slice):
    g = np.asarray(image_slice).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (g - g.min()) / (g.max() - g.min())
    out = np.repeat(g[..., None], 3, axis=-1)
    for value, rgb in COLOURS.items():
        out[np.asarray(label_slice) == value] = np.array(rgb)
    return out


def as_dtype(ov, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return ov
    if dtype == np.float32:
        return ov.astype(np.float32)
    assert dtype == np.uint8
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(ov), 0.0, 255 * ov).astype(np.uint8)


def panels(image, label, pred):
    """([raw, gt, pred] x 3 views in figure order: float32 (H, W) and float64 (H, W, 3) after np.rot90; int32 (3,) indices by axis)."""
    best = best_slices(label)
    out = []
    for a in VIEW_AXES:
        img = take_slice(image, a, best[a])
        out.append(np.rot90(img))
        out.append(np.rot90(overlay(img, take_slice(label, a, best[a]))))
        out.append(np.rot90(overlay(img, take_slice(pred, a, best[a]))))
    return out, best


def overlay_stack(image, label, axis):
    return np.stack([overlay(take_slice(image, axis, k), take_slice(label, axis, k)) for k in range(image.shape[axis])])


def same_values(a, b):
    """Equal as values, NaN positions included; a signed zero is not distinguished."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
