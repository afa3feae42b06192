"""float64 numpy restatement of scipy.ndimage.zoom(x, factors, order=3|0, mode='nearest', prefilter=False), the call the
reference's resampling scripts make (scripts/resampling/amos_ct_resample.py:60,70,93,97).  The checker of the resample
tests: written from scipy's documented behaviour, independent of the product module, pinned to scipy itself by
tests/golden/resample*.npz (tests/test_resample_cpu.py) and, where scipy imports, against scipy directly."""
import numpy as np


def stage1_image(golden, case):
    """scipy's float64 stage-1 image of a chain fixture, whole: one array, or slabs along axis 0 in files of their own."""
    g = golden("resample_" + case)
    if "image1" in g:
        return g["image1"]
    return np.concatenate([golden(f"resample_{case}_image1_{k}")["image1_part"] for k in range(int(g["image1_parts"]))], axis=0)


def out_shape(shape, factors):
    f = np.broadcast_to(np.asarray(factors, dtype=np.float64), (len(shape),))
    return tuple(int(round(n * float(z))) for n, z in zip(shape, f))


def _coords(n_in, n_out):
    z = float(n_in - 1) / float(n_out - 1) if n_out > 1 else 1.0      # scipy recomputes the zoom from the two shapes
    return np.arange(n_out, dtype=np.float64) * z


def nearest_index(n_in, n_out):
    return np.clip(np.floor(_coords(n_in, n_out) + 0.5).astype(np.int64), 0, n_in - 1)


def cubic_taps(n_in, n_out):
    """(indices (n_out, 4) clamped = mode 'nearest', B-spline weights (n_out, 4)), no prefilter."""
    cc = _coords(n_in, n_out)
    f = np.floor(cc)
    t = cc - f
    idx = np.clip(f.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    w = np.stack([(1 - t) ** 3, 3 * t ** 3 - 6 * t ** 2 + 4, -3 * t ** 3 + 3 * t ** 2 + 3 * t + 1, t ** 3], axis=1) / 6.0
    return idx, w


def zoom_to_shape(x, shape, order):
    """Zoom to a given output shape, axis by axis: take + weighted sum."""
    y = np.asarray(x, dtype=np.float64) if order == 3 else np.asarray(x)
    for ax, n_out in enumerate(shape):
        n_in = y.shape[ax]
        if order == 0:
            y = np.take(y, nearest_index(n_in, n_out), axis=ax)
        else:
            idx, w = cubic_taps(n_in, n_out)
            bshape = [1] * y.ndim
            bshape[ax] = n_out
            y = sum(np.take(y, idx[:, k], axis=ax) * w[:, k].reshape(bshape) for k in range(4))
    return y


def zoom(x, factors, order):
    return zoom_to_shape(x, out_shape(np.shape(x), factors), order)


def cubic_at(x, shape, od, oh, ow):
    """The order-3 zoom of x to `shape`, evaluated only at the output voxels (od[i], oh[i], ow[i]); float64."""
    x = np.asarray(x)
    (idd, wd), (idh, wh), (idw, ww) = (cubic_taps(n, m) for n, m in zip(x.shape, shape))
    acc = np.zeros(len(od), dtype=np.float64)
    for a in range(4):
        for b in range(4):
            wab = wd[od, a] * wh[oh, b]
            for c in range(4):
                acc += x[idd[od, a], idh[oh, b], idw[ow, c]].astype(np.float64) * (wab * ww[ow, c])
    return acc


def sample_voxels(shape, n, seed):
    """n seeded random output voxels + the 8 corners + one full line along each axis (through a seeded point)."""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    pts = [np.stack([rng.integers(0, D, n), rng.integers(0, H, n), rng.integers(0, W, n)], axis=1)]
    pts.append(np.array([[d, h, w] for d in (0, D - 1) for h in (0, H - 1) for w in (0, W - 1)]))
    p = [int(rng.integers(0, s)) for s in shape]
    for ax, s in enumerate(shape):
        line = np.tile(np.array(p), (s, 1))
        line[:, ax] = np.arange(s)
        pts.append(line)
    pts = np.concatenate(pts, axis=0)
    return pts[:, 0], pts[:, 1], pts[:, 2]
