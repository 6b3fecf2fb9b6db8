"""Inputs and numpy oracles of the packed QSGD matrix (tests/test_gpu_qsgd_packed_matrix.py);
tests/test_qsgd_packed_host.py checks, without a GPU, that they have the properties the matrix relies on.
Data recipes and numpy arithmetic only: no GPU, no torch device.

* Levels: one code width b per cell, every b in 2..32, and per b up to two levels: L_lo = 2^(b-2) (a
  power of two: the decoders' exact-multiply path) and L_hi = min(2^(b-1) - 1, 2^31 - 2) (every b-bit code
  but one is a valid level; the division path from b = 4 on).  61 levels.
* Layouts: fixed sizes and offsets (multiples of 32), see LAYOUTS.
* Payloads for the pack: levels uniform in [-L, L] with -L, +L, 0, +1 and -1 forced at the edges of every
  tensor and of every 32-element group inside one; the payload arena's padding holds a filler that is no
  level (int8 -128, int32 INT32_MIN) and must never reach the output.
* ``pack_ref``: the packed arena the header specifies, a canary word wherever nothing is written.
* Messages for the decoders: random 32-bit words with runs of all-zero and all-one words in every tensor,
  made by no encoder; codes above 2L occur.  ``codes_ref`` reads code i of a tensor from bits
  [i b, (i + 1) b) of its stream, ``levels_ref`` takes code - L as int32 (modulo 2^32), and
  qsgd_matrix_inputs.decode_ref turns that into floats.
"""

import numpy as np

import qsgd_matrix_inputs as M
from oracle import bitpack

WIDTHS = tuple(range(2, 33))
GROUP = 32        # elements per packed group: b words
BLOCK = 8192      # elements per workgroup of the pack and the decode
CANARY = np.float32(-12345.5)
CANARY_WORD = np.uint32(0xC0DEFACE)
FILL = {8: np.int8(-128), 32: np.int32(np.iinfo(np.int32).min)}
EDGE = ("-L", "+L", "0", "+1", "-1")

MIX_SIZES = [1, 31, 32, 33, 5, 4097, 1000, 40000, 8192, 8193, 13001]
MIX_OFFSETS = [0, 32, 64, 128, 192, 224, 7104, 8256, 48256, 56448, 64672]

LAYOUTS = {
    "MIX": (MIX_SIZES, MIX_OFFSETS),                        # tests/test_gpu_decode_sum_packed.py's arena
    "LEAD32": ([33, 1, 4097], [32, 96, 128]),               # exactly one leading padding group
    "LEADBLK": ([40, 8200], [8256, 8320]),                  # the first 8 Ki block is leading padding, and more
    "TINY": ([5], [0]),                                     # less than one group
    "TINY_LEAD": ([3], [64]),
    "EXACT": ([8192, 32, 8160], [0, 8192, 8224]),           # no padding, ends on an 8 Ki block
}


def levels_of(b):
    """The levels of width b: (L_lo, L_hi), one level where they coincide (b = 2)."""
    lo, hi = 1 << (b - 2), min((1 << (b - 1)) - 1, (1 << 31) - 2)
    return (lo,) if lo == hi else (lo, hi)


ALL_LEVELS = [(b, L) for b in WIDTHS for L in levels_of(b)]


def storage_widths(L):
    """The payload widths the pack accepts at L: int8 while L <= 127, int32 always."""
    return (8, 32) if L <= 127 else (32,)


class Layout:
    def __init__(self, name):
        self.name = name
        self.sizes, self.offsets = (list(v) for v in LAYOUTS[name])
        self.nt = len(self.sizes)
        self.end = self.offsets[-1] + self.sizes[-1]
        self.groups = -(-self.end // GROUP)
        self.ranges = list(zip(self.offsets, self.sizes))
        self.pad = np.ones(self.end, bool)
        for o, n in self.ranges:
            self.pad[o:o + n] = False
        self.prev = (np.random.default_rng(5).standard_normal(self.end) * 0.5).astype(np.float32)
        self.prev[self.pad] = CANARY

    def words(self, b):
        """32-bit words of the packed arena."""
        return self.groups * b

    def payload_elems(self, width):
        return self.end if width == 32 else (self.end + 3) & ~3

    def tensor_words(self, t, b):
        """(first word, word count) of tensor t's groups, its partial last group included."""
        o, n = self.ranges[t]
        return o // GROUP * b, -(-n // GROUP) * b

    def written_words(self, b):
        """Mask over the packed arena: the words of some tensor's groups."""
        m = np.zeros(self.words(b), bool)
        for t in range(self.nt):
            w0, nw = self.tensor_words(t, b)
            m[w0:w0 + nw] = True
        return m

    def edge_positions(self):
        """Arena positions of the first and last element of every tensor and of the elements on both
        sides of every 32-group boundary (so of every 8 Ki boundary) inside a tensor, ascending."""
        pos = set()
        for o, n in self.ranges:
            pos.update((o, o + n - 1))
            for g in range(o + GROUP, o + n, GROUP):
                pos.update((g - 1, g))
        return sorted(pos)


_layouts = {}


def layout(name):
    if name not in _layouts:
        _layouts[name] = Layout(name)
    return _layouts[name]


def _seed(*parts):
    return [int(p) & 0xFFFFFFFF for p in parts]


def edge_value(kind, L):
    return {"-L": -L, "+L": L, "0": 0, "+1": 1, "-1": -1}[kind]


def edge_kind(j, b, width):
    """The forced value at the j-th edge position: the cycle -L, +L, 0, +1, -1, shifted by the cell."""
    return EDGE[(j + b + (width == 32)) % len(EDGE)]


def pack_payload(width, L, lay):
    """The payload arena (``lay.payload_elems(width)`` int8 or int32): uniform levels, the forced edge
    values, and FILL everywhere outside the tensors."""
    b = bitpack.packed_bits(L)
    rng = np.random.default_rng(_seed(0x9ACC, width, L, lay.end))
    q = rng.integers(-L, L + 1, lay.end, dtype=np.int64)
    for j, p in enumerate(lay.edge_positions()):
        q[p] = edge_value(edge_kind(j, b, width), L)
    dtype = np.int8 if width == 8 else np.int32
    buf = np.full(lay.payload_elems(width), FILL[width], dtype)
    buf[:lay.end][~lay.pad] = q[~lay.pad].astype(dtype)
    return buf


def pack_ref(q, L, lay, canary=CANARY_WORD):
    """The packed arena of the payload arena q (uint32 words): per tensor its levels, extended with -L
    (code 0) to whole groups, through bitpack.pack at word offsets[t] b / 32; the canary elsewhere."""
    b = bitpack.packed_bits(L)
    out = np.full(lay.words(b), canary, np.uint32)
    for t, (o, n) in enumerate(lay.ranges):
        ext = np.full(-(-n // GROUP) * GROUP, -L, np.int64)
        ext[:n] = q[o:o + n]
        w = np.frombuffer(bitpack.pack(ext, L), "<u4")
        w0, nw = lay.tensor_words(t, b)
        assert w.size == nw
        out[w0:w0 + nw] = w
    return out


def message(b, lay, seed=0):
    """A packed arena no encoder made (uint32 words): random words, and in every tensor a run of all-zero
    and a run of all-one words at its two ends (which end is which alternates with t + seed) and, where
    it is long enough, a zero run next to a one run in the middle."""
    rng = np.random.default_rng(_seed(0x3E55, b, lay.end, seed))
    w = rng.integers(0, 1 << 32, lay.words(b), dtype=np.uint64).astype(np.uint32)
    ones = np.uint32(0xFFFFFFFF)
    for t in range(lay.nt):
        w0, nw = lay.tensor_words(t, b)
        r = max(1, min(nw // 3, b + 1))
        first, last = (0, ones) if (t + seed) % 2 == 0 else (ones, 0)
        w[w0:w0 + r] = first
        w[w0 + nw - r:w0 + nw] = last
        if nw >= 6 * r:
            mid = w0 + nw // 2
            w[mid - r:mid] = last
            w[mid:mid + r] = first
    return w


def codes_ref(words, lay, t, b):
    """Tensor t's codes (uint64): code i from bits [i b, (i + 1) b) of its stream, LSB first."""
    o, n = lay.ranges[t]
    w0, nw = lay.tensor_words(t, b)
    stream = np.ascontiguousarray(words[w0:w0 + nw]).astype("<u4").view(np.uint8)
    bits = np.unpackbits(stream, bitorder="little")[:n * b].reshape(n, b)
    weight = np.uint64(1) << np.arange(b, dtype=np.uint64)
    return (bits.astype(np.uint64) * weight[None, :]).sum(axis=1, dtype=np.uint64)


def levels_ref(codes, L):
    """code - L reduced to int32 two's complement (the reduction only matters at b = 32)."""
    return ((codes.astype(np.int64) - int(L)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def norms_for(lay, b, k=0):
    """DEC_NORMS cycled over the tensors, the cycle shifted by b (and by the client k)."""
    return np.array([M.DEC_NORMS[(t + b + k) % len(M.DEC_NORMS)] for t in range(lay.nt)], np.float32)


def decode_terms(words, L, lay, norms):
    """The decode of every tensor's codes (fp32), +0 in the padding."""
    b = bitpack.packed_bits(L)
    term = np.zeros(lay.end, np.float32)
    for t, (o, n) in enumerate(lay.ranges):
        term[o:o + n] = M.decode_ref(levels_ref(codes_ref(words, lay, t, b), L), norms[t], L)
    return term


def decode_want(words, L, lay, norms):
    """(plain decode into an arena of canaries, accumulating decode into ``lay.prev``)."""
    term = decode_terms(words, L, lay, norms)
    plain = np.full(lay.end, CANARY, np.float32)
    plain[~lay.pad] = term[~lay.pad]
    acc = lay.prev.copy()
    with np.errstate(all="ignore"):
        acc[~lay.pad] = lay.prev[~lay.pad] + term[~lay.pad]
    return plain, acc


def sum_ref(lay, terms, start=None, divisor=None):
    """s = start (or +0); s = fl32(s + term_k) on the tensors' elements in client order; then one IEEE
    division on the tensors' elements and, from +0, on the padding too (+0 / divisor)."""
    s = np.zeros(lay.end, np.float32) if start is None else start.copy()
    with np.errstate(all="ignore"):
        for term in terms:
            s[~lay.pad] = s[~lay.pad] + term[~lay.pad]
        if divisor is not None:
            where = np.ones(lay.end, bool) if start is None else ~lay.pad
            s[where] = s[where] / np.float32(divisor)
    return s
