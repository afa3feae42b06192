"""Plain numpy model of the foreground-balanced patch sampler (include/mi3d.h mi3d_patch_count / mi3d_patch_pick / mi3d_patch_crop,
spatial.pick_starts / crop_patches): the checker of tests/test_gpu_patch.py, written from the contract, independent of the product
module (it imports nothing of it), and checked against Python integers, np.flatnonzero and a brute-force statement of the start rule
by tests/test_patch_ref_cpu.py.  Integers only: every comparison is exact.

    index    d H W + h W + w over the logical axes of a sample, V = D H W
    group    group_of[v] for a value 0..255 (255: in no group); an int64 value outside 0..255 is in no group, tested as it is
    mulhi64  floor(a b / 2^64)
    pick     c = voxels of the group in the sample;  c > 0: the r-th of them in ascending index, r = mulhi64(rnd, c), picked = group;
             c == 0: voxel mulhi64(rnd, V), picked = -1
    start    clamp(centre_a - size_a // 2, 0, n_a - size_a) per axis
    crop     out[k, c] = in[c, start_d : start_d + Do, start_h : start_h + Ho, start_w : start_w + Wo]

rank_word(r, c) = ceil(r 2^64 / c) is the smallest word that mulhi64 maps to rank r: with it a test asks for every rank of a group.

CASES is the one list the CPU and the GPU tests share; MUTANTS are four wrong readings of the contract, and the CPU test checks that
the list tells each of them from the model, so a kernel that makes one of these mistakes cannot pass the GPU tests.
"""
import collections
import functools

import numpy as np

NO_GROUP = 255
MAX_GROUPS = 8
MUTANTS = ("rank off by one", "label truncated to a byte", "start clamped to n - size - 1", "fallback uses the count")

POS_NEG = (0,) + (1,) * 255                                          # RandCropByPosNegLabel's table
PER_CLASS = tuple(range(4)) + (NO_GROUP,) * 252                      # RandCropByLabelClasses(num_classes=4)'s


def mulhi64(a, b):
    """floor(a * b / 2^64) of uint64 arrays (or scalars), through 32-bit halves: no intermediate leaves 64 bits."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    lo, s = np.uint64(0xFFFFFFFF), np.uint64(32)
    a0, a1, b0, b1 = a & lo, a >> s, b & lo, b >> s
    mid = (a0 * b0 >> s) + (a1 * b0 & lo) + (a0 * b1 & lo)           # < 3 * 2^32
    return a1 * b1 + (a1 * b0 >> s) + (a0 * b1 >> s) + (mid >> s)


def rank_word(r, c):
    """The smallest 64-bit word w with mulhi64(w, c) == r, for 0 <= r < c: ceil(r * 2^64 / c), in Python integers."""
    return -((-int(r) << 64) // int(c))


def groups_of(labels, group_of, mutant=None):
    """The group of every voxel (NO_GROUP where none) as uint8, shape of labels."""
    table = np.asarray(group_of, dtype=np.uint8)
    lab = np.asarray(labels)
    if lab.dtype == np.uint8 or mutant == "label truncated to a byte":
        return table[lab.astype(np.uint8)]
    inside = (lab >= 0) & (lab <= 255)
    return np.where(inside, table[np.where(inside, lab, 0)], np.uint8(NO_GROUP)).astype(np.uint8)


def n_groups(group_of):
    return 1 + max(g for g in group_of if g != NO_GROUP)


def counts(labels, group_of, mutant=None):
    """(N, G) int64: voxels of each group per sample of labels (N, D, H, W)."""
    g = groups_of(labels, group_of, mutant).reshape(labels.shape[0], -1)
    return np.stack([np.bincount(row, minlength=256)[:n_groups(group_of)] for row in g]).astype(np.int64)


def start_of(centre, size, n, mutant=None):
    top = n - size - 1 if mutant == "start clamped to n - size - 1" else n - size
    return min(max(centre - size // 2, 0), top)


def pick(labels, group_of, sample, group, rnd, size, mutant=None):
    """(starts (K, 3) int32, voxel (K,) int32, picked (K,) int32, counts (N, G) int64) of labels (N, D, H, W) in logical order."""
    n = labels.shape[1:]
    v = int(np.prod(n))
    g = groups_of(labels, group_of, mutant).reshape(labels.shape[0], -1)
    cnt = counts(labels, group_of, mutant)
    members = {}
    starts, voxel, picked = [], [], []
    for s, q, word in zip(sample, group, rnd):
        s, q, c = int(s), int(q), int(cnt[int(s), int(q)])
        if c > 0:
            if (s, q) not in members:
                members[s, q] = np.flatnonzero(g[s] == q)
            r = int(mulhi64(word, c)) + (1 if mutant == "rank off by one" else 0)
            i = int(members[s, q][min(r, c - 1)])
        else:
            i = int(mulhi64(word, c if mutant == "fallback uses the count" else v))
        centre = np.unravel_index(i, n)
        starts.append([start_of(int(centre[a]), size[a], n[a], mutant) for a in range(3)])
        voxel.append(i)
        picked.append(q if c > 0 else -1)
    return np.array(starts, dtype=np.int32).reshape(-1, 3), np.array(voxel, dtype=np.int32), np.array(picked, dtype=np.int32), cnt


def crop(x, starts, size):
    """(K, C, Do, Ho, Wo) of x (C, D, H, W): plain slices, so every bit pattern is kept."""
    return np.stack([x[:, s[0]:s[0] + size[0], s[1]:s[1] + size[1], s[2]:s[2] + size[2]] for s in np.asarray(starts)])


def all_ranks(labels, group_of, sample, group):
    """(sample, group, rnd) arrays that ask for every rank 0..c-1 of one (sample, group), in order."""
    c = int(counts(labels, group_of)[sample, group])
    return [sample] * c, [group] * c, [rank_word(r, c) for r in range(c)]


# ---------------------------------------------------------------------------------------------- cases
TOP = 2 ** 64 - 1
Case = collections.namedtuple("Case", "name labels group_of sample group rnd size")


def _random_labels(shape, dtype, seed, high=4):
    return np.random.default_rng(seed).integers(0, high, shape).astype(dtype)


def _build_cases():
    out = []
    # every rank of one class in a little over two blocks of 4096 voxel indices; windows odd and even, one as wide as its side
    lab = _random_labels((1, 5, 7, 300), np.uint8, 1)
    out.append(Case("ranks-u8", lab, PER_CLASS, *all_ranks(lab, PER_CLASS, 0, 2), (3, 4, 101)))
    out.append(Case("ranks-u8-full-w", lab, PER_CLASS, *all_ranks(lab, PER_CLASS, 0, 0), (2, 7, 300)))
    # two samples with different content: every rank of the second's foreground
    lab = _random_labels((2, 3, 5, 150), np.int64, 2)
    lab[1] = (lab[1] == 3) * 3
    out.append(Case("ranks-i64-n2", lab, POS_NEG, *all_ranks(lab, POS_NEG, 1, 1), (2, 2, 7)))
    # int64 values that are in no group and must not be narrowed: -1 -> 255, 256 -> 0, 2^40 + 1 -> 1
    lab = _random_labels((1, 4, 6, 9), np.int64, 3, high=2)
    lab.reshape(-1)[::5] = -1
    lab.reshape(-1)[1::7] = 256
    lab.reshape(-1)[2::11] = 2 ** 40 + 1
    for g in (0, 1):
        out.append(Case(f"wild-i64-g{g}", lab, POS_NEG, *all_ranks(lab, POS_NEG, 0, g), (3, 3, 4)))
    # a class the scan lacks: any voxel, picked = -1
    lab = _random_labels((1, 4, 5, 6), np.uint8, 4, high=3)
    words = [0, 1, TOP, 2 ** 63, 0x123456789ABCDEF0, TOP // 3]
    out.append(Case("absent", lab, PER_CLASS, [0] * 6, [3] * 6, words, (2, 3, 4)))
    # the class's only voxel is the last voxel of a volume that ends inside a block
    lab = np.zeros((1, 5, 7, 300), dtype=np.uint8)
    lab[0, -1, -1, -1] = 2
    out.append(Case("last-voxel", lab, PER_CLASS, [0] * 4, [2, 2, 0, 0], [0, TOP, 0, TOP], (3, 3, 8)))
    # centres at all eight corners; even and odd windows, one as large as its side
    lab = np.zeros((1, 6, 7, 9), dtype=np.int64)
    lab[0, ::5, ::6, ::8] = 1
    for size in ((3, 4, 5), (6, 2, 9), (1, 7, 1), (4, 3, 8)):
        out.append(Case("corners-" + "x".join(map(str, size)), lab, POS_NEG, *all_ranks(lab, POS_NEG, 0, 1), size))
    # fewer voxels than one block
    lab = _random_labels((1, 3, 4, 5), np.uint8, 5)
    for g in range(4):
        out.append(Case(f"small-g{g}", lab, PER_CLASS, *all_ranks(lab, PER_CLASS, 0, g), (2, 2, 3)))
    for c in out:
        c.labels.setflags(write=False)
    return tuple(out)


CASES = _build_cases()


def case(name):
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def model(name, mutant=None):
    """(starts, voxel, picked, counts) of a case, computed once and shared (callers must not write into them)."""
    c = case(name)
    out = pick(c.labels, c.group_of, c.sample, c.group, c.rnd, c.size, mutant)
    for a in out:
        a.setflags(write=False)
    return out
