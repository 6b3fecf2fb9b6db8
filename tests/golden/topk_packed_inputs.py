"""The opt-in bit-packed Top-K index wire ("TopKBitPackedCompression") restated in numpy, and the recipes of
its tests (tests/test_topk_packed_host.py, tests/test_gpu_topk_packed_matrix.py, tests/test_gpu_topk_packed_wire.py).

The wire: the k tensor-local indices of a tensor of n elements, b = index_bits(n) bits each, LSB-first
little-endian — index i at bits [i b, (i + 1) b) of the stream, the first ceil(k b / 8) bytes sent, the unused
high bits of the last byte 0.  The packed arena of a plan (sizes) and a count vector: a group of 32 consecutive
indices of a tensor is b whole 32-bit words; tensor t's first group is goff[t] = sum_{u<t} ceil(k_u / 32), its
first word woff[t] = sum_{u<t} ceil(k_u / 32) b_u; the codes after a tensor's k_t-th index are 0.

Nothing here imports the package under test.
"""

from collections import namedtuple

import numpy as np

MAX_ELEMS = 2**32
GROUP = 32
CANARY_WORD = np.uint32(0xC0DEFACE)
CANARY_INDEX = np.int64(-0x0123456789ABCDEF)


def index_bits(n):
    n = int(n)
    if not 1 <= n <= MAX_ELEMS:
        raise ValueError(f"n = {n} outside [1, 2^32]")
    return max(1, (n - 1).bit_length())


def _bits_of(codes, b):
    """The k codes' bits, LSB first, as one uint8 vector of k b bits."""
    codes = np.asarray(codes, dtype=np.uint64).reshape(-1)
    return ((codes[:, None] >> np.arange(b, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)


def pack_indices(indices, n):
    """indices_data of a layer: ceil(k b / 8) bytes."""
    b = index_bits(n)
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < n)
    return np.packbits(_bits_of(idx, b), bitorder="little").tobytes()


def unpack_indices(data, k, n):
    """The k int64 indices of indices_data; bits past k b are ignored."""
    b = index_bits(n)
    raw = np.frombuffer(data, dtype=np.uint8)
    assert raw.size * 8 >= k * b
    bits = np.unpackbits(raw, bitorder="little")[:k * b].reshape(k, b).astype(np.uint64)
    return (bits << np.arange(b, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64).astype(np.int64)


Layout = namedtuple("Layout", "bits koff goff woff words")


def arena_layout(sizes, counts):
    bits = [index_bits(n) for n in sizes]
    koff, goff, woff = [0], [0], [0]
    for k, b in zip(counts, bits):
        g = -(-int(k) // GROUP)
        koff.append(koff[-1] + int(k))
        goff.append(goff[-1] + g)
        woff.append(woff[-1] + g * b)
    return Layout(bits, koff, goff, woff, woff[-1])


def pack_arena(sizes, counts, indices, pad_ones=False):
    """The packed arena's words (uint32).  ``pad_ones``: every bit past a tensor's k_t b set to 1 (what a
    receiver must ignore) instead of the 0 a sender writes."""
    lay = arena_layout(sizes, counts)
    out = np.zeros(lay.words, dtype=np.uint32)
    idx = np.asarray(indices, dtype=np.int64)
    for t, (k, b) in enumerate(zip(counts, lay.bits)):
        nw = lay.woff[t + 1] - lay.woff[t]
        bits = np.full(32 * nw, 1 if pad_ones else 0, dtype=np.uint8)
        bits[:k * b] = _bits_of(idx[lay.koff[t]:lay.koff[t + 1]], b)
        out[lay.woff[t]:lay.woff[t + 1]] = np.packbits(bits, bitorder="little").view("<u4")
    return out


def unpack_arena(sizes, counts, words):
    lay = arena_layout(sizes, counts)
    w = np.ascontiguousarray(words, dtype="<u4")
    out = np.zeros(lay.koff[-1], dtype=np.int64)
    for t, k in enumerate(counts):
        out[lay.koff[t]:lay.koff[t + 1]] = unpack_indices(w[lay.woff[t]:lay.woff[t + 1]].tobytes(), k, sizes[t])
    return out


# ---------------------------------------------------------------- recipes

# the device matrix: eighteen sizes at the edges of the rule (widths 1, 2, 3, 5, 6, 7, 9, 16, 17, 20, 21, 25, 26),
# then one size for each width below 26 they leave out, so that the plan holds every b = 1 .. 26
MATRIX_EDGE_SIZES = [1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 257, 65535, 65536, 65537, 2**20, 2**20 + 1, 2**25, 2**25 + 1]
MATRIX_FILL_SIZES = [9, 200, 1000, 2047, 4096, 4097, 16384, 20000, 2**17 + 1, 2**19, 2**21 + 1, 2**23, 2**23 + 1]
MATRIX_SIZES = MATRIX_EDGE_SIZES + MATRIX_FILL_SIZES


def count_choices(n):
    c = {0, 1, 31, 32, 33, min(n, 1000)}
    if n <= 257:
        c.add(n)
    return sorted(k for k in c if k <= n)


def count_vectors(sizes=MATRIX_SIZES, seed=20):
    """Count vectors over ``sizes``: every choice of every tensor appears at least once (vector v takes each
    tensor's choice v + t, cyclically: neighbours differ), then the largest of each, then drawn ones."""
    rng = np.random.default_rng(seed)
    most = max(len(count_choices(n)) for n in sizes)
    vs = [[count_choices(n)[(v + t) % len(count_choices(n))] for t, n in enumerate(sizes)] for v in range(most)]
    vs.append([count_choices(n)[-1] for n in sizes])
    for _ in range(3):
        vs.append([int(rng.choice(count_choices(n))) for n in sizes])
    return vs


def draw_indices(sizes, counts, seed):
    """Per tensor k_t indices in [0, n_t): 0 and n_t - 1 among them when k_t allows, the rest random, in
    random order."""
    rng = np.random.default_rng(seed)
    out = []
    for n, k in zip(sizes, counts):
        ix = rng.integers(0, n, size=k, dtype=np.int64)
        if k >= 1:
            ix[0] = n - 1
        if k >= 2:
            ix[1] = 0
        rng.shuffle(ix)
        out.append(ix)
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def size_of_width(b, rng):
    """A tensor size whose width is b: 2^b, 2^(b-1) + 1 or one between."""
    lo, hi = (1, 2) if b == 1 else (2**(b - 1) + 1, 2**b)
    return int(rng.choice([lo, hi, int(rng.integers(lo, hi + 1))]))


# the wire test's dict
WIRE_SIZES = [1_000_003, 70_000, 4_097, 33, 1]
WIRE_RATIO = 0.01
