"""tests/boundary_ref.py against independent routes, on the CPU: the map model against scipy's two distance transforms per class, the
term model against float64 torch autograd, the allowance constants against float32 torch, and the case lists against mutants."""
import numpy as np
import pytest
import torch

import boundary_ref as B

ndi = pytest.importorskip("scipy.ndimage")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _one_hot2dist(m, spacing, off):
    """Kervadec's one_hot2dist with `sampling` for one class mask, the literal 1 generalised to `off`."""
    return ndi.distance_transform_edt(~m, sampling=spacing) * ~m - (ndi.distance_transform_edt(m, sampling=spacing) - off) * m


@pytest.mark.parametrize("k", range(len(B.MAP_CASES)), ids=["%s-%s-%s" % (c[0], c[1][0], c[2]) for c in B.MAP_CASES])
def test_maps_equal_scipy(k):
    name, spacing, off = B.MAP_CASES[k]
    lab, classes = B.map_labels(name), B.MAP_LABELS[name][1]
    phi = B.map_case(k)
    off = B.default_offset(spacing) if off is None else off
    samples = lab[None] if lab.ndim == 3 else lab
    assert phi.dtype == np.float32 and phi.shape == lab.shape[:lab.ndim - 3] + (len(classes),) + lab.shape[-3:]
    for n, sample in enumerate(samples):
        for j, c in enumerate(classes):
            m, got = sample == c, phi.reshape((len(samples), len(classes)) + sample.shape)[n, j]
            if not m.any() or m.all():          # the stated rule: scipy would measure to a phantom voxel
                assert not got.any()
                continue
            assert np.array_equal(_bits(got), _bits(_one_hot2dist(m, spacing, off).astype(np.float32)))
            assert (got[~m] > 0).all() and ((got[m] <= 0).all() or off > min(spacing))


def test_absent_full_and_offsets_are_covered():
    """The case list has what the issue names: an absent class, a full class, a single voxel; at unit spacing the default offset is
    Kervadec's 1, and a literal 1 at 0.75 mm is positive inside an organ while the default is not."""
    lab = B.map_labels("absent_full")
    assert (lab[0] == 1).all() and not (lab[0] == 2).any() and (B.map_labels("single_voxel") == 2).sum() == 1
    assert B.default_offset((1.0, 1.0, 1.0)) == 1.0 and B.default_offset((2.5, 0.75, 0.75)) == 0.75
    box, sp = B.map_labels("box987"), (2.5, 0.75, 0.75)
    literal, default = B.signed_maps(box, (1,), sp, 1.0)[0], B.signed_maps(box, (1,), sp)[0]
    assert literal[box == 1].max() == 0.25 and default[box == 1].max() == 0.0


def _torch_term(i, dtype):
    """(weight L, gradient * grad_scale) of TERM_CASES[i] by torch autograd in `dtype`."""
    family, N, C, V, off, ch, mask, ign, weight, gs, flags = B.TERM_CASES[i]
    z, f, lab, _, _ = B.term_case(i)
    zt = torch.tensor(np.asarray(z), dtype=dtype, requires_grad=True)
    prod = torch.softmax(zt, dim=1)[:, list(ch)] * torch.tensor(np.asarray(f), dtype=dtype)
    if lab is not None:
        prod = prod * torch.tensor(lab != ign, dtype=dtype)[:, None]
    loss = prod.mean() * weight
    loss.backward()
    return float(loss.detach()), (zt.grad * gs).double().numpy()


SMALL = [i for i, c in enumerate(B.TERM_CASES) if c[3] <= B.CPU_MAX_V]


@pytest.mark.parametrize("i", SMALL, ids=[B.TERM_IDS[i] for i in SMALL])
def test_term_equals_float64_autograd(i):
    family, N, C, V, off, ch, mask, ign, weight, gs, flags = B.TERM_CASES[i]
    z, f, lab, value, grad = B.term_case(i)
    tv, tg = _torch_term(i, torch.float64)
    to64 = B.K_F64 * B.U64 / B.U          # the float32 allowances at constant 1, rescaled to float64
    assert abs(value - tv) <= to64 * B.value_allowance(z, f, ch, lab, ign, weight, value, k=1.0)
    assert np.all(np.abs(grad - tg) <= to64 * B.grad_allowance(z, f, ch, lab, ign, weight, gs, k=1.0))


def test_allowance_constants():
    """The constants are 4 x the largest float32-torch ratio over the case list, measured here and written in boundary_ref.py."""
    worst_v = worst_g = 0.0
    for i in SMALL:
        family, N, C, V, off, ch, mask, ign, weight, gs, flags = B.TERM_CASES[i]
        z, f, lab, value, grad = B.term_case(i)
        tv, tg = _torch_term(i, torch.float32)
        av = B.value_allowance(z, f, ch, lab, ign, weight, value, k=1.0)
        ag = B.grad_allowance(z, f, ch, lab, ign, weight, gs, k=1.0)
        if av > 0:
            worst_v = max(worst_v, abs(tv - value) / av)
        worst_g = max(worst_g, float((np.abs(tg - grad)[ag > 0] / ag[ag > 0]).max(initial=0.0)))
        assert not np.abs(tg - grad)[ag == 0].any()
    print(f"largest float32-torch ratio: value {worst_v:.3f} dlogits {worst_g:.3f}")
    # the constants are the measured values x 4 (rounded up a little), not more than that
    assert worst_v * 4 <= B.K_VALUE <= worst_v * 4 * 1.1
    assert worst_g * 4 <= B.K_GRAD <= worst_g * 4 * 1.1


@pytest.mark.parametrize("mutant", B.MAP_MUTANTS)
def test_map_cases_see_mutants(mutant):
    seen = 0
    for k, (name, spacing, off) in enumerate(B.MAP_CASES):
        bad = B.signed_maps(B.map_labels(name), B.MAP_LABELS[name][1], spacing, off, mutant=mutant)
        seen += not np.array_equal(_bits(bad), _bits(B.map_case(k)))
    assert seen >= 3


@pytest.mark.parametrize("mutant", B.TERM_MUTANTS)
def test_term_cases_see_mutants(mutant):
    """A mutant is seen where it leaves the allowance of the value or of a gradient element."""
    seen = 0
    for i in SMALL:
        family, N, C, V, off, ch, mask, ign, weight, gs, flags = B.TERM_CASES[i]
        z, f, lab, value, grad = B.term_case(i)
        bv, bg = B.term(z, f, ch, lab, ign, weight, gs, mutant=mutant)
        seen += bool(abs(bv - value) > B.value_allowance(z, f, ch, lab, ign, weight, value) or
                     (np.abs(bg - grad) > B.grad_allowance(z, f, ch, lab, ign, weight, gs)).any())
    assert seen >= 3
