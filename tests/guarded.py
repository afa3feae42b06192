"""Caller-owned memory for the tests that hand the C entries their workspaces and outputs: a buffer of exactly the bytes an entry may
touch, between two guard bands, on the device or on the host.  No torch beyond plain tensors, no framework.

  Guarded(nbytes, align, band, fill, device)          uint8 [band | payload of exactly nbytes | band]; .ptr .nbytes .payload
                                                      .refill(fill) .check() .untouched()
  GuardedOut(shape, dtype, prefill, ...)              the same bands around an output of a dtype and shape; .tensor as well
  same_bits(runs, what)                               raises unless every array of `runs` holds the same bits

The payload starts on an `align` boundary and on no stricter one (its address is an odd multiple of align), so an entry that
quietly needs more than it documents shows.  The payload holds one of FILLS: 0x00, 0xA5, or 0xFF, which reads as -1 in every
integer width and as NaN in float32 and float64.  The bands, and the slack around them, hold BAND, four bytes that none of the
fills contains.  check() compares both bands on the host and raises with the offset of the first changed byte, counted from the
payload's first byte: -1 is the last byte of the front band, nbytes the first byte of the back band.

An element an entry skips keeps its prefill, and cannot hold the same bits after two runs with different prefills: same_bits over
runs with different prefills is the proof that every element of an output was written."""
import numpy as np
import torch

FILLS = (0x00, 0xA5, 0xFF)
BAND = (0xC3, 0x3C, 0x96, 0x69)
# what an output holds before the call, one per run; every value of a run's column differs from the other runs'
PREFILLS = {
    torch.uint8: (0x5A, 0xE1, 0x17),
    torch.int32: (-7777777, 0x5A5A5A5A, 1234567),
    torch.int64: (-7777777, 0x5A5A5A5A5A5A5A5A, 1234567),
    torch.float32: (7e7, float("nan"), -3e-3),
    torch.float64: (7e7, float("nan"), -3e-3),
}


class GuardError(AssertionError):
    pass


class Guarded:
    def __init__(self, nbytes, align=256, band=4096, fill=0xA5, device="cpu"):
        assert nbytes >= 0 and band >= 1 and align >= 1 and align & (align - 1) == 0 and band % len(BAND) == 0
        self.nbytes, self.align, self.band = int(nbytes), align, band
        raw = torch.empty(2 * band + self.nbytes + 2 * align, dtype=torch.uint8, device=device)
        start = (align - (raw.data_ptr() + band)) % (2 * align)          # the payload at an odd multiple of align
        pattern = torch.tensor(BAND, dtype=torch.uint8, device=device)
        raw.copy_(pattern.repeat(-(-raw.numel() // len(BAND)))[:raw.numel()])
        self._raw = raw
        self._front = raw[start:start + band]
        self.payload = raw[start + band:start + band + self.nbytes]
        self._back = raw[start + band + self.nbytes:start + 2 * band + self.nbytes]
        self._front_want, self._back_want = self._front.cpu().numpy().copy(), self._back.cpu().numpy().copy()
        self.ptr = raw.data_ptr() + start + band
        assert self.ptr % align == 0 and self.ptr % (2 * align) != 0
        self.refill(fill)

    def refill(self, fill):
        assert fill in FILLS, fill
        self.fill = fill
        self.payload.fill_(fill)

    def _sync(self):
        if self._raw.is_cuda:
            torch.cuda.synchronize(self._raw.device)

    def check(self, what="buffer"):
        """Both bands as they were, or GuardError with the offset (from the payload's first byte) of the first changed byte."""
        self._sync()
        for got, want, base in ((self._front, self._front_want, -self.band), (self._back, self._back_want, self.nbytes)):
            changed = np.flatnonzero(got.cpu().numpy() != want)
            if changed.size:
                raise GuardError(f"{what}: guard band changed at offset {base + int(changed[0])} of a payload of {self.nbytes} bytes "
                                 f"({changed.size} bytes of the band changed)")

    def untouched(self):
        """Whether every payload byte still holds the fill."""
        self._sync()
        return bool((self.payload == self.fill).all())


class GuardedOut(Guarded):
    """An output of `shape` and `dtype` (dense; `strides` in elements for another dense layout) of exactly its extent, between the
    bands, every element holding `prefill`.  align defaults to the element size."""

    def __init__(self, shape, dtype, prefill, align=None, band=4096, strides=None, device="cpu"):
        shape = tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        super().__init__(int(np.prod(shape, dtype=np.int64)) * item, align or item, band, FILLS[0], device)
        flat = self.payload.view(dtype)
        self.tensor = flat.view(shape) if strides is None else torch.as_strided(flat, shape, tuple(int(s) for s in strides))
        self.tensor.fill_(prefill)
        self._before = self.payload.clone()

    def set(self, array):
        """Give the output a content of its own (an in-place input, a sum that is added to) in place of the prefill."""
        self.tensor.copy_(torch.from_numpy(np.array(array, order="C")).to(self.tensor.device))
        self._before = self.payload.clone()

    def untouched(self):
        """Whether every byte is what it was before the call."""
        self._sync()
        return torch.equal(self.payload, self._before)

    def host(self):
        self._sync()
        return self.tensor.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))


def same_bits(runs, what="output"):
    """Raises unless all arrays of `runs` have one shape, one dtype and the same bits; names the first element that differs."""
    first = np.ascontiguousarray(runs[0])
    for k, other in enumerate(runs[1:], 1):
        other = np.ascontiguousarray(other)
        if other.shape != first.shape or other.dtype != first.dtype:
            raise GuardError(f"{what}: run {k} is {other.dtype}{other.shape}, run 0 is {first.dtype}{first.shape}")
        differs = np.flatnonzero((bits(first) != bits(other)).any(axis=-1).reshape(-1))
        if differs.size:
            at = np.unravel_index(int(differs[0]), first.shape) if first.ndim else ()
            raise GuardError(f"{what}: {differs.size} elements differ between run 0 and run {k}, the first at {tuple(int(i) for i in at)}: "
                             f"{first[at]!r} against {other[at]!r} (an element that was never written keeps its prefill)")
