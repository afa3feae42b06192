"""tests/entropy_ref.py against independent routes, on the CPU: the model against float64 torch autograd of
-sum softmax * log_softmax / (N V ln C), the allowance constants against the float32 restatement of the kernel's formula, and the case
list against four mutants."""
import math

import numpy as np
import pytest
import torch

import entropy_ref as E

SMALL = [i for i, c in enumerate(E.CASES) if c[3] <= E.CPU_MAX_V]


def _torch_term(i):
    """(weight L, gradient * grad_scale) of CASES[i] by float64 torch autograd."""
    family, N, C, V, off, mode, mask, ign, weight, gs, flags = E.CASES[i]
    z, lab, _, _ = E.case(i)
    zt = torch.tensor(np.asarray(z), dtype=torch.float64, requires_grad=True)
    h = -(torch.softmax(zt, dim=1) * torch.log_softmax(zt, dim=1)).sum(dim=1)
    if mode != E.ALL:
        hit = torch.tensor(lab == ign)
        h = h * (hit if mode == E.IGNORED else ~hit).double()
    loss = h.sum() / (N * V * math.log(C)) * weight
    loss.backward()
    return float(loss.detach()), (zt.grad * gs).numpy()


@pytest.mark.parametrize("i", SMALL, ids=[E.IDS[i] for i in SMALL])
def test_term_equals_float64_autograd(i):
    """1e-15 relative: of the value against its own size, of a gradient element against the largest element a voxel could have,
    |s| (the factor p q is of order 1), plus the element's own size."""
    family, N, C, V, off, mode, mask, ign, weight, gs, flags = E.CASES[i]
    z, lab, value, grad = E.case(i)
    tv, tg = _torch_term(i)
    s = abs(weight * gs) / (N * V * math.log(C))
    assert abs(value - tv) <= 1e-15 * max(abs(tv), abs(weight) * 1e-3), (value, tv)
    assert np.all(np.abs(grad - tg) <= 1e-15 * (np.abs(tg) + s))
    if family == "uniform":
        assert abs(value - weight * E.select(lab, ign, mode, (N, V)).mean()) <= 1e-12          # H / ln C = 1 on every selected voxel
    if family == "saturated":          # float64 still sees exp(-128) = 2.6e-56; float32 does not (test_allowance_constants)
        assert 0.0 <= value < 1e-50 and np.abs(grad).max() < 1e-50


def test_modes_partition_the_volume():
    """COUNTED + IGNORED = ALL for value and gradient, and the divisor does not depend on the selection."""
    z, lab = E.make_logits("gauss", 2, 4, 512, 3), E.make_labels("random30", 2, 4, 512, 255, 3)
    va, ga = E.term(z, lab, 255, E.ALL)
    vc, gc = E.term(z, lab, 255, E.COUNTED)
    vi, gi = E.term(z, lab, 255, E.IGNORED)
    assert abs(va - (vc + vi)) <= 1e-15 and np.allclose(ga, gc + gi, rtol=0, atol=1e-18)
    assert 0.0 < vi < vc < va < 1.0 and not (gc * gi).any()


def test_allowance_constants():
    """The constants are 4 x the largest ratio of the float32 restatement over the case list, measured here and written in
    entropy_ref.py; the restatement lies inside the allowances, and the saturated family is exactly zero in float32."""
    worst_v = worst_g = 0.0
    for i in SMALL:
        family, N, C, V, off, mode, mask, ign, weight, gs, flags = E.CASES[i]
        z, lab, value, grad = E.case(i)
        tv, tg = E.term32(z, lab, ign, mode, weight, gs)
        if family == "saturated":
            assert tv == 0.0 and not tg.any()
        av = E.value_allowance(z, lab, ign, mode, weight, value, k=1.0)
        ag = E.grad_allowance(z, lab, ign, mode, weight, gs, k=1.0)
        sel = np.broadcast_to(E.select(lab, ign, mode, (N, V))[:, None], grad.shape)
        assert not tg[~sel].any() and not grad[~sel].any()
        assert abs(tv - value) <= E.value_allowance(z, lab, ign, mode, weight, value)
        assert (np.abs(tg - grad) <= E.grad_allowance(z, lab, ign, mode, weight, gs)).all()
        if sel.any() and weight != 0.0:
            worst_v = max(worst_v, abs(tv - value) / av)
            worst_g = max(worst_g, float((np.abs(tg - grad)[sel] / ag[sel]).max()))
    print(f"largest float32-restatement ratio: value {worst_v:.4f} dlogits {worst_g:.4f}")
    # the constants are the measured values x 4 (rounded up a little), not more than that
    assert worst_v * 4 <= E.K_VALUE <= worst_v * 4 * 1.1
    assert worst_g * 4 <= E.K_GRAD <= worst_g * 4 * 1.1


def test_the_case_list_has_what_it_promises():
    fam = {c[0] for c in E.CASES}
    assert fam == set(E.FAMILIES)
    assert {c[2] for c in E.CASES} >= {2, 3, 4, 8} and {c[1] for c in E.CASES} == {1, 2, 3}
    assert {c[3] for c in E.CASES} >= {1, 70, 3220, 3221, 1200000} and sum(c[3] > E.CPU_MAX_V for c in E.CASES) == 1
    assert any(c[4] == 1 and c[3] == 3221 for c in E.CASES)
    for mode in (E.ALL, E.COUNTED, E.IGNORED):
        assert {c[6] for c in E.CASES if c[5] == mode} >= {"random30", "runs", "all", "unused"}
    assert {c[10] for c in E.CASES} == {0, 1, 2, 3} and {c[9] for c in E.CASES} == {1.0, 0.5} and any(c[8] < 0 for c in E.CASES)


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_cases_see_mutants(mutant):
    """A mutant is seen where it leaves the allowance of the value or of a gradient element."""
    seen = 0
    for i in SMALL:
        family, N, C, V, off, mode, mask, ign, weight, gs, flags = E.CASES[i]
        z, lab, value, grad = E.case(i)
        bv, bg = E.term(z, lab, ign, mode, weight, gs, mutant=mutant)
        seen += bool(abs(bv - value) > E.value_allowance(z, lab, ign, mode, weight, value) or
                     (np.abs(bg - grad) > E.grad_allowance(z, lab, ign, mode, weight, gs)).any())
    assert seen >= 3
