"""What the modules on stored label maps and scans share (components, surface, preview): the views of a volume argument with
every check that needs no device, the dtype code tables and the workspace query.  A new label-map entry starts from here and from
csrc/volume.h."""
import operator

import torch

from . import _lib, orientation
from ._lib import Mi3dError

_IMAGE = {torch.float32: _lib.SRC_F32, torch.int16: _lib.SRC_I16}
_LABEL = {torch.uint8: _lib.SRC_U8, torch.int64: _lib.SRC_I64}


def _integer(v, what, name):
    try:
        return operator.index(v)
    except TypeError:
        raise Mi3dError(f"{what}: {name} {v!r} is not an integer") from None


def _connectivity(connectivity, what):
    if connectivity not in (1, 2, 3):
        raise Mi3dError(f"{what}: connectivity {connectivity!r} is not 1, 2 or 3 (6, 18 or 26 neighbours)")
    return int(connectivity)


def _strides(t):
    return [max(int(s), 1) for s in t.stride()]          # the stride of a one-element axis is never used


def _samples(labels, what):
    """The (N, D, H, W) view of a label argument, its dtype code and whether it came as 3-D; every check that needs no device."""
    if not isinstance(labels, torch.Tensor):
        raise Mi3dError(f"{what}: the labels are a torch tensor, got {type(labels).__name__}")
    if labels.dtype not in _LABEL:
        raise Mi3dError(f"{what}: labels are {' or '.join(str(d) for d in _LABEL)}, got {labels.dtype}")
    if labels.dim() not in (3, 4) or min(labels.shape) < 1:
        raise Mi3dError(f"{what}: a (D, H, W) or (N, D, H, W) label volume expected, got {tuple(labels.shape)}")
    single = labels.dim() == 3
    t = labels[None] if single else labels
    orientation.check_dense(t.shape[1:], t.stride()[1:], what)
    v = t.shape[1] * t.shape[2] * t.shape[3]
    if v >= 2 ** 31:
        raise Mi3dError(f"{what}: a sample of {v} voxels; fewer than 2^31 expected")
    if t.shape[0] > 1 and t.stride(0) < v:
        raise Mi3dError(f"{what}: samples overlap (shape {tuple(t.shape)}, strides {tuple(t.stride())})")
    return t, _LABEL[labels.dtype], single


def _volume3(t, codes, kind, what):
    """The 3-D view of a volume argument and its dtype code; every check that needs no device."""
    if not isinstance(t, torch.Tensor):
        raise Mi3dError(f"{what}: the {kind} is a torch tensor, got {type(t).__name__}")
    while t.dim() > 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3 or min(t.shape) < 1:
        raise Mi3dError(f"{what}: one 3-D {kind} volume (leading singleton dims aside) expected, got {tuple(t.shape)}")
    if t.dtype not in codes:
        raise Mi3dError(f"{what}: the {kind} is {' or '.join(str(d) for d in codes)}, got {t.dtype}")
    orientation.check_dense(t.shape, t.stride(), what)
    return t, codes[t.dtype]


def _workspace(entry, t, what, *more):
    """The bytes `entry` (a *_workspace_bytes query) asks for the samples t and its further arguments `more`."""
    nbytes = getattr(_lib.lib(), entry)(*t.shape, *more)
    if nbytes == 0:
        with_classes = f" with {more[0]} classes" if more else ""
        raise Mi3dError(f"{what}: {tuple(t.shape)}{with_classes} is outside the library's range")
    return nbytes
