"""The detector detects: tests/guarded.py on the host.  A byte changed at either inner edge of a band raises with its offset, a
change inside the payload does not, the payload sits on the alignment asked for and no stricter one, and the comparison of runs
with different prefills fails when one element was left alone."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402


@pytest.mark.parametrize("nbytes", (0, 1, 13, 256, 4099))
@pytest.mark.parametrize("fill", G.FILLS)
def test_a_fresh_buffer_is_intact_and_holds_its_fill(nbytes, fill):
    g = G.Guarded(nbytes, fill=fill)
    g.check()
    assert g.nbytes == nbytes and g.payload.numel() == nbytes and g.untouched()
    assert nbytes == 0 or g.payload.data_ptr() == g.ptr          # an empty tensor has no address of its own
    assert (g.payload == fill).all() and not set(G.BAND) & set(G.FILLS)
    g.refill(G.FILLS[(G.FILLS.index(fill) + 1) % 3])
    g.check()
    assert g.untouched() and (nbytes == 0 or int(g.payload[0]) != fill)


@pytest.mark.parametrize("nbytes", (1, 13, 512))
def test_the_last_byte_of_the_front_band_is_watched(nbytes):
    g = G.Guarded(nbytes, band=64)
    g._raw[g.ptr - g._raw.data_ptr() - 1] ^= 1
    with pytest.raises(G.GuardError, match=r"offset -1 of a payload of %d bytes" % nbytes):
        g.check()


@pytest.mark.parametrize("nbytes", (1, 13, 512))
def test_the_first_byte_of_the_back_band_is_watched(nbytes):
    g = G.Guarded(nbytes, band=64)
    g._raw[g.ptr - g._raw.data_ptr() + nbytes] ^= 0x80
    with pytest.raises(G.GuardError, match=r"offset %d of a payload of %d bytes" % (nbytes, nbytes)):
        g.check()


def test_the_outer_edges_and_the_first_of_several_changes_are_reported():
    g = G.Guarded(100, band=64)
    at = g.ptr - g._raw.data_ptr()
    g._raw[at - 64] = 0
    with pytest.raises(G.GuardError, match="offset -64 "):
        g.check()
    g = G.Guarded(100, band=64)
    at = g.ptr - g._raw.data_ptr()
    g._raw[at + 100 + 63] = 0
    g._raw[at + 100 + 7] = 0
    with pytest.raises(G.GuardError, match=r"offset 107 .*\(2 bytes"):
        g.check()


def test_a_change_inside_the_payload_does_not_raise():
    g = G.Guarded(13, band=64)
    g.payload[0] = 1
    g.payload[12] = 2
    g.check()
    assert not g.untouched()


@pytest.mark.parametrize("nbytes", (1, 7, 105, 4097))
@pytest.mark.parametrize("align", (8, 16, 256))
def test_the_payload_is_aligned_as_asked_and_no_stricter(align, nbytes):
    g = G.Guarded(nbytes, align=align)
    assert g.ptr % align == 0 and g.ptr % (2 * align) == align and g.payload.data_ptr() == g.ptr
    g.check()


@pytest.mark.parametrize("dtype", sorted(G.PREFILLS, key=str), ids=str)
def test_an_output_holds_its_prefill_between_the_bands(dtype):
    for k, prefill in enumerate(G.PREFILLS[dtype]):
        o = G.GuardedOut((2, 3, 5), dtype, prefill)
        item = o.tensor.element_size()
        assert o.nbytes == 30 * item and o.ptr % item == 0 and o.tensor.data_ptr() == o.ptr and o.untouched()
        want = np.full((2, 3, 5), prefill, dtype=o.host().dtype)
        G.same_bits([o.host(), want])
        o.tensor[1, 2, 4] = 1
        o.check()
        assert not o.untouched()
    assert len({repr(p) for p in G.PREFILLS[dtype]}) == 3


def test_a_strided_output_covers_exactly_its_payload():
    a = np.arange(2 * 3 * 4 * 5, dtype=np.int64).reshape(2, 3, 4, 5)
    o = G.GuardedOut(a.shape, torch.int64, -1, strides=(60, 1, 3, 12))          # each sample Fortran-ordered
    o.set(a)
    assert o.untouched() and np.array_equal(o.host(), a)
    assert np.array_equal(o.payload.view(torch.int64).numpy(), np.stack([s.transpose(2, 1, 0).ravel() for s in a]).ravel())
    o.check()


def entry_that_skips(out, skip):
    """A stand-in for an entry that writes every element of its output but `skip`."""
    flat = out.tensor.view(-1)
    for i in range(flat.numel()):
        if i != skip:
            flat[i] = 3 * i
    return out.host()


@pytest.mark.parametrize("dtype", (torch.int32, torch.float32, torch.float64, torch.uint8), ids=str)
def test_an_element_left_alone_fails_the_comparison_of_runs(dtype):
    whole = [entry_that_skips(G.GuardedOut((4, 5), dtype, p), None) for p in G.PREFILLS[dtype]]
    G.same_bits(whole)
    holed = [entry_that_skips(G.GuardedOut((4, 5), dtype, p), 13) for p in G.PREFILLS[dtype]]
    with pytest.raises(G.GuardError, match=r"1 elements differ between run 0 and run 1, the first at \(2, 3\)"):
        G.same_bits(holed)
    with pytest.raises(G.GuardError, match="run 2"):          # NaN against a number, and a number against a number
        G.same_bits([holed[0], holed[0], holed[2]])
    # a stale but correct value is exactly what one prefill cannot show: the same hole under one prefill passes
    G.same_bits([entry_that_skips(G.GuardedOut((4, 5), dtype, G.PREFILLS[dtype][0]), 13) for _ in range(2)])


def test_same_bits_tells_signed_zeros_nans_shapes_and_dtypes_apart():
    G.same_bits([np.array([np.nan, 0.0]), np.array([np.nan, 0.0])])
    with pytest.raises(G.GuardError):
        G.same_bits([np.array([0.0]), np.array([-0.0])])
    with pytest.raises(G.GuardError):
        G.same_bits([np.zeros(3, np.int32), np.zeros(3, np.int64)])
    with pytest.raises(G.GuardError):
        G.same_bits([np.zeros((1, 3)), np.zeros(3)])
    G.same_bits([np.float32(1.5), np.float32(1.5)])
