"""Inputs and oracle of the Top-K receive matrix (tests/test_gpu_topk_recv_matrix.py);
tests/test_topk_recv_host.py checks, without a GPU, that they have the properties the matrix relies
on.  Data recipes and numpy arithmetic only: seeded numpy Generators, no torch RNG, no GPU.

The receive side consumes bytes it did not produce: a message carries arbitrary int64 indices and
arbitrary per-tensor counts.  So the recipes below are not an encoder's selections.

Layouts (``LAYOUTS``; arena_layout of topk_matrix_inputs, so every start is a multiple of ``align``):

* ``aligned``  [5, 70001, 1 << 20, 3000, 200003, 65536, 131071] at 64-element starts: tensors that start
               mid-super-tile (64 Ki arena elements), one of exactly a super-tile's elements, an arena end
               that is no multiple of 4.
* ``tight``    the ``edges`` sizes of topk_matrix_inputs at starts 4 apart: adjacent tensors share
               float4s and words of the duplicate check's bitmap.
* ``many``     700 tensors of 100 elements around four odd ones: every place block (4096 values) spans
               more than 512 tensors, so the tensor lookup is the binary search in global memory.
* ``tiny``     one tensor of 3 elements, less than a float4.
* ``large``    three tensors, 2.2 M elements: the ``most`` count vector selects over 1.1 M values of the
               first tensor alone, past the 4096-workgroup cap of both scatter kernels; the index check's
               messages select every element, past its 2048-workgroup cap.

Count vectors (``count_vectors``): a ratio's own (``r01``, ``r05``; ``r1`` = every element on tight and
tiny), zero counts leading / in the middle / trailing, all zero (``none``), ``full`` (one large tensor
with counts[t] = sizes[t]: its super-tiles' bucket capacity is clamped to 65536), ``clu20k`` (aligned:
20000 values for the 1 << 20 tensor) and ``most`` (large: four fifths of every tensor).

Index profiles (``message``): ``uniform``, ``clustered``, ``edges_of_tiles`` (its own counts) and
``skipped``; values N(0, 1) with planted specials (``SPECIAL_BITS``); ``make_base`` is the arena modes 1
and 2 decode onto.  ``check_messages`` / ``dup_messages`` are the messages of the two check kernels.

Oracle: ``decode_ref``, ``check_ref``, ``dup_ref``, ``caps_ref`` restate the reference decoder
(``dense[indices] = values`` per layer), include/omf_codec.h and omf_topk_layout.cpp dec_tables_host.
"""

import math
import zlib

import numpy as np

import topk_matrix_inputs as TM

SUPER_BITS, SUB_BITS = 16, 14  # omf_topk_layout.h kDecSuperBits, omf_topk_recv.hip kDecSubBits
SUPER, SUB = 1 << SUPER_BITS, 1 << SUB_BITS
DEC_STAGE = 2048   # bucket entries a tile workgroup stages in LDS (more: read unstaged)
DEC_CHUNK = 4096   # selected values per place block
DEC_WIN = 512      # most tensors of a place block whose koff is staged in LDS
SCATTER_CAP = 4096 * 256  # values one grid trip of topk_scatter / topk_scatter_arena covers
DUP_TRIP = 2048 * 256     # entries one grid trip of the duplicate check covers
CHECK_BLOCK = 4 * 256     # entries per workgroup of the index check (until its 2048-workgroup cap)
NO_BAD = 0x7F7F7F7F
CANARY = TM.CANARY
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TWO32 = 1 << 32
# -0.0, +-inf, +-FLT_MAX, a subnormal, a quiet and a signalling NaN of distinct payloads
SPECIAL_BITS = (0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x000116C2, 0x7FC00000, 0x7FA00001)
BASE_BITS = (0x80000000, 0x7F800000, 0x7FC00000)  # planted in the base: -0.0, inf, NaN
RATIOS = {"r01": 0.01, "r05": 0.05, "r1": 1.0}


class Layout:
    def __init__(self, name, seed, sizes, align=TM.ALIGN):
        self.name, self.seed, self.align = name, seed, align
        self.sizes = [int(n) for n in sizes]
        self.offsets, self.arena_end = TM.arena_layout(self.sizes, align)
        self.nt = len(self.sizes)
        self.names = [f"n{n}@{t}" for t, n in enumerate(self.sizes)]

    def ks(self, ratio):
        return [TM.topk_k(n, ratio) for n in self.sizes]

    @property
    def nsuper(self):
        return (self.arena_end + SUPER - 1) >> SUPER_BITS


_MANY_SIZES = [1] + [100] * 350 + [4097, 513] + [100] * 350 + [7]

LAYOUTS = {
    "aligned": Layout("aligned", 31, [5, 70001, 1 << 20, 3000, 200003, 65536, 131071]),
    "tight": Layout("tight", 32, TM._EDGE_SIZES, align=4),
    "many": Layout("many", 33, _MANY_SIZES),
    "tiny": Layout("tiny", 34, [3]),
    "large": Layout("large", 35, [1_400_003, 500_001, 300_000]),
}
FULL_TENSOR = {"aligned": 4, "large": 2}  # the tensor of the ``full`` count vector
CLUSTER_TENSOR, CLUSTER_COUNT = 2, 20000  # aligned: the 1 << 20 tensor


def padding_mask(L):
    pad = np.ones(L.arena_end, bool)
    for o, n in zip(L.offsets, L.sizes):
        pad[o:o + n] = False
    return pad


# ------------------------------------------------------------------ count vectors

def count_vectors(L):
    """name -> per-tensor counts, 0 <= counts[t] <= sizes[t]."""
    r01, r05 = L.ks(0.01), L.ks(0.05)
    out = {"r01": r01, "r05": r05}
    if L.name in ("tight", "tiny"):
        out["r1"] = list(L.sizes)
    if L.nt >= 3:
        third = L.nt // 3
        out["zeros_lead"] = [0] * third + r05[third:]
        out["zeros_mid"] = r05[:third] + [0] * (L.nt - 2 * third) + r05[L.nt - third:]
        out["zeros_trail"] = r05[:L.nt - third] + [0] * third
    out["none"] = [0] * L.nt
    if L.name in FULL_TENSOR:
        full = list(r01)
        full[FULL_TENSOR[L.name]] = L.sizes[FULL_TENSOR[L.name]]
        out["full"] = full
    if L.name == "aligned":
        clu = list(r01)
        clu[CLUSTER_TENSOR] = CLUSTER_COUNT
        out["clu20k"] = clu
    if L.name == "large":
        out["most"] = [n * 4 // 5 for n in L.sizes]
    return out


def koff_of(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


# ------------------------------------------------------------------ index profiles

def _rng(L, *key):
    """A Generator of its own per (layout, key): strings enter the seed by their CRC-32."""
    return np.random.default_rng([L.seed, *[zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key]])


def _subset(rng, n, k):
    """k distinct indices of [0, n), in random order."""
    if k == 0:
        return np.zeros(0, np.int64)
    if 8 * k < n:
        return rng.choice(n, k, replace=False).astype(np.int64)
    return rng.permutation(n)[:k].astype(np.int64)


def uniform_indices(L, counts, rng):
    return [_subset(rng, n, k) for n, k in zip(L.sizes, counts)]


def cluster_super(L):
    """The first super-tile that lies wholly inside aligned's 1 << 20 tensor."""
    o = L.offsets[CLUSTER_TENSOR]
    s = (o + SUPER - 1) >> SUPER_BITS
    assert (s + 1) << SUPER_BITS <= o + L.sizes[CLUSTER_TENSOR]
    return s


def clustered_indices(L, counts, rng):
    """uniform, but every index of the 1 << 20 tensor lies in one super-tile of the arena."""
    per = uniform_indices(L, counts, rng)
    lo = (cluster_super(L) << SUPER_BITS) - L.offsets[CLUSTER_TENSOR]
    per[CLUSTER_TENSOR] = lo + _subset(rng, SUPER, counts[CLUSTER_TENSOR])
    return per


def edges_of_tiles_indices(L, rng):
    """Per tensor: the first and last element of every sub-tile (16 Ki arena elements; a super-tile's
    edges are among them) the tensor touches, clipped to the tensor — so its own first and last element
    too, and the arena's last.  In random order."""
    per = []
    for o, n in zip(L.offsets, L.sizes):
        q = np.arange(o >> SUB_BITS, ((o + n - 1) >> SUB_BITS) + 1, dtype=np.int64)
        pos = np.unique(np.concatenate([np.maximum(o, q << SUB_BITS), np.minimum(o + n - 1, ((q + 1) << SUB_BITS) - 1)]))
        per.append(rng.permutation(pos - o).astype(np.int64))
    return per


def skipped_variants(n, i):
    """The values include/omf_codec.h says a decoder skips, for a tensor of n elements; i: a valid index
    (the last two are valid only after truncation to 32 bits)."""
    return [-1, n, n + 3, -n - 1, TWO32 + int(i), -TWO32 + int(i)]


def skipped_indices(L, counts, rng):
    """uniform with every eighth entry of a tensor (at least one) replaced by a skipped value; returns
    (per-tensor indices, per-tensor mask of the replaced entries)."""
    per = uniform_indices(L, counts, rng)
    masks = []
    for t, (n, idx) in enumerate(zip(L.sizes, per)):
        m = np.zeros(idx.size, bool)
        if idx.size:
            where = rng.choice(idx.size, max(1, idx.size // 8), replace=False)
            for j, w in enumerate(where):
                idx[w] = skipped_variants(n, idx[w])[(t + j) % 6]
            m[where] = True
        masks.append(m)
    return per, masks


def make_values(rng, k):
    """N(0, 1) with the specials planted (fewer than 8 values: the first k specials)."""
    sp = np.array(SPECIAL_BITS, np.uint32).view(np.float32)
    if k <= sp.size:
        return sp[:k].copy()
    v = rng.standard_normal(k).astype(np.float32)
    v[rng.choice(k, sp.size, replace=False)] = sp
    return v


def make_base(L):
    """The arena modes 1 and 2 decode onto: N(0, 1) with -0.0, inf and NaN planted (8 of each; every
    element of a tiny arena is one), CANARY in the padding."""
    rng = _rng(L, "base")
    base = rng.standard_normal(L.arena_end).astype(np.float32)
    pad = padding_mask(L)
    inside = np.flatnonzero(~pad)
    pos = rng.choice(inside, min(24, inside.size), replace=False)
    base[pos] = np.array([BASE_BITS[j % 3] for j in range(pos.size)], np.uint32).view(np.float32)
    base[pad] = CANARY
    return base


class Message:
    def __init__(self, L, counts_name, profile, counts, per, skipped=None):
        self.layout, self.counts_name, self.profile = L, counts_name, profile
        self.counts = [int(c) for c in counts]
        self.per = per  # per-tensor index arrays
        self.indices = np.concatenate(per).astype(np.int64) if per else np.zeros(0, np.int64)
        self.ktot = int(self.indices.size)
        self.values = make_values(_rng(L, counts_name, profile, "values"), self.ktot)
        self.skipped = np.concatenate(skipped) if skipped is not None else np.zeros(self.ktot, bool)
        self.ratio = RATIOS.get(counts_name)  # not None: the counts are this ratio's own
        self.key = (L.name, counts_name, profile)


def message_keys(L):
    """Every (counts name, profile) of the layout's decode cells."""
    keys = []
    for name, counts in count_vectors(L).items():
        keys.append((name, "uniform"))
        if sum(counts):
            keys.append((name, "skipped"))
        if L.name == "aligned" and name in ("clu20k", "r05"):
            keys.append((name, "clustered"))
    keys.append(("edges", "edges_of_tiles"))
    return keys


_MESSAGES = {}


def message(L, counts_name, profile):
    key = (L.name, counts_name, profile)
    if key in _MESSAGES:
        return _MESSAGES[key]
    rng = _rng(L, counts_name, profile)
    if profile == "edges_of_tiles":
        per = edges_of_tiles_indices(L, rng)
        m = Message(L, counts_name, profile, [p.size for p in per], per)
    else:
        counts = count_vectors(L)[counts_name]
        if profile == "uniform":
            m = Message(L, counts_name, profile, counts, uniform_indices(L, counts, rng))
        elif profile == "clustered":
            m = Message(L, counts_name, profile, counts, clustered_indices(L, counts, rng))
        elif profile == "skipped":
            per, masks = skipped_indices(L, counts, rng)
            m = Message(L, counts_name, profile, counts, per, masks)
        else:
            raise ValueError(profile)
    _MESSAGES[key] = m
    return m


# ------------------------------------------------------------------ messages of the check kernels

def _blocks(L, counts, rng):
    return uniform_indices(L, counts, rng)


def check_counts(L):
    """The count vector of the layout's index-check messages: zero-count tensors between non-empty
    ones where the layout has tensors to spare, and more than one workgroup where it has the elements."""
    cv = count_vectors(L)
    if L.name == "many":
        return [0 if t % 5 == 3 else min(n, 9) for t, n in enumerate(L.sizes)]
    if L.name == "tight":
        return [0 if t in (4, 9) else min(n, max(7, n // 4)) for t, n in enumerate(L.sizes)]
    if L.name == "aligned":
        return [5, 3500, 0, 150, 10000, 0, 6553]
    if L.name == "large":
        return list(L.sizes)
    return cv["r1"]


def check_messages(L):
    """name -> (counts, indices) for omf_topk_check_indices."""
    counts = check_counts(L)
    koff = koff_of(counts)
    live = [t for t in range(L.nt) if counts[t] > 0]
    out = {}

    def start(name):
        per = _blocks(L, counts, _rng(L, "check", name))
        return per

    def done(name, per):
        out[name] = (list(counts), np.concatenate(per).astype(np.int64))

    done("clean", start("clean"))
    # every boundary value, in every tensor with room for the seven (fewer: the first counts[t])
    per = start("boundaries")
    for t in live:
        n = L.sizes[t]
        b = [-n - 1, -n, -n + 1, -1, 0, n - 1, n]
        per[t][:min(7, counts[t])] = b[:min(7, counts[t])]
    done("boundaries", per)
    # no bad entry: the valid boundaries, and every other entry negative (i - n)
    per = start("wrap_only")
    for t in live:
        n = L.sizes[t]
        per[t][1::2] -= n
        b = [-n, -n + 1, -1, 0, n - 1]
        c = min(5, counts[t])
        per[t][counts[t] - c:] = b[:c]
    done("wrap_only", per)
    # the extremes and the 32-bit aliases of valid indices, in the upper half of the tensors
    per = start("extremes")
    for t in live[len(live) // 2:]:
        i = int(per[t][0])
        b = [I64_MIN, I64_MAX, TWO32 + i, -TWO32 + i]
        per[t][:min(4, counts[t])] = b[:min(4, counts[t])]
    done("extremes", per)
    # bad entries in three tensors: all over the last one, at the first entry of a middle one and at
    # the LAST entry of the lowest, which a workgroup of its own meets (where the message has several)
    per = start("multi_bad")
    a, b, c = multi_bad_tensors(L)
    per[c][::3] = L.sizes[c]
    per[b][0] = -L.sizes[b] - 1
    per[a][-1] = L.sizes[a] + 3
    done("multi_bad", per)
    per = start("last_only")
    per[live[-1]][-1] = L.sizes[live[-1]]
    done("last_only", per)
    out["none"] = ([0] * L.nt, np.zeros(0, np.int64))
    return out


def multi_bad_tensors(L):
    live = [t for t, c in enumerate(check_counts(L)) if c > 0]
    return live[len(live) // 3], live[2 * len(live) // 3], live[-1]


FAR_COUNTS = [700_000, 10, 10]  # large: one tensor's entries span two grid trips of the duplicate check
FAR_A, FAR_B = 0, 650_000


def dup_messages(L):
    """name -> (counts, indices, clean) for omf_topk_check_duplicates: ``clean`` selects the positions of
    ``indices`` once (every later occurrence of a repeated index replaced by n, which is ignored)."""
    out = {}
    counts = count_vectors(L)["r1" if L.name in ("tight", "tiny") else "r05"]
    if L.name == "aligned":
        counts = [5, 3500, 52428, 150, 10000, 3276, 6553]
    live = [t for t in range(L.nt) if counts[t] >= 2]

    def add(name, cnts, per):
        idx = np.concatenate(per).astype(np.int64)
        clean = []
        for n, p in zip(L.sizes, per):
            p = p.copy()
            ok = (p >= 0) & (p < n)
            _, first = np.unique(p, return_index=True)
            later = np.ones(p.size, bool)
            later[first] = False
            p[later & ok] = n
            clean.append(p)
        out[name] = (list(cnts), idx, np.concatenate(clean).astype(np.int64))

    add("none", counts, uniform_indices(L, counts, _rng(L, "dup", "none")))
    if live:
        # a repeat within one wave: two adjacent entries, in the first and the last tensor with two
        per = uniform_indices(L, counts, _rng(L, "dup", "wave"))
        for t in {live[0], live[-1]}:
            per[t][1] = per[t][0]
        add("wave", counts, per)
        # repeats only among out-of-range values: nothing to flag
        per = uniform_indices(L, counts, _rng(L, "dup", "oor"))
        for t in live:
            n = L.sizes[t]
            v = skipped_variants(n, per[t][0])
            for j in range(min(counts[t] // 2, 6)):
                per[t][2 * j] = per[t][2 * j + 1] = v[j]
        add("oor", counts, per)
    if L.name == "tight":
        # every element of every tensor once: each bitmap word is shared by neighbours, none repeats
        add("shared_word", list(L.sizes), uniform_indices(L, L.sizes, _rng(L, "dup", "shared")))
    if L.name == "large":
        per = uniform_indices(L, FAR_COUNTS, _rng(L, "dup", "far"))
        per[0][FAR_B] = per[0][FAR_A]
        add("far", FAR_COUNTS, per)
    return out


# ------------------------------------------------------------------ oracle

def decode_ref(mode, base, L, counts, values, indices):
    """include/omf_codec.h, omf_topk_decode*: mode 0: +0 over [0, arena_end), padding included, then
    y[begin_t + i] = v; mode 1: the same stores over base; mode 2: y[begin_t + i] = fl32(y[..] + v).
    Indices outside [0, n_t) are skipped; every other element of base is unchanged.  (Indices unique
    per tensor: the reference's dense[indices] = values.)"""
    y = np.zeros(L.arena_end, np.float32) if mode == 0 else np.array(base, np.float32, copy=True)
    values = np.ascontiguousarray(values, np.float32)
    koff = koff_of(counts)
    for t, (o, n) in enumerate(zip(L.offsets, L.sizes)):
        i = indices[koff[t]:koff[t + 1]]
        v = values[koff[t]:koff[t + 1]]
        ok = (i >= 0) & (i < n)
        pos = o + i[ok]
        if mode == 2:
            with np.errstate(all="ignore"):
                y[pos] = (y[pos] + v[ok]).astype(np.float32)
        else:
            y[pos] = v[ok]
    return y


def check_ref(L, counts, indices):
    """omf_topk_check_indices: (wrapped, bad) — i + n for i in [-n, 0), everything else as it was; the
    lowest tensor with an index outside [-n, n), or NO_BAD."""
    wrapped = np.array(indices, np.int64, copy=True)
    koff = koff_of(counts)
    bad = NO_BAD
    for t, n in enumerate(L.sizes):
        i = wrapped[koff[t]:koff[t + 1]]  # a view
        if ((i < -n) | (i >= n)).any():
            bad = min(bad, t)
        neg = (i >= -n) & (i < 0)
        i[neg] += n
    return wrapped, bad


def dup_ref(L, counts, indices):
    """omf_topk_check_duplicates: flags[t] = 1 where an index of tensor t inside [0, n) occurs twice."""
    koff = koff_of(counts)
    flags = np.zeros(L.nt, np.int32)
    for t, n in enumerate(L.sizes):
        i = indices[koff[t]:koff[t + 1]]
        i = i[(i >= 0) & (i < n)]
        flags[t] = int(np.unique(i).size < i.size)
    return flags


def caps_ref(L, counts):
    """omf_topk_layout.cpp dec_tables_host: the bucket capacity of every super-tile,
    min(ceil(2 * expect) + 256, 65536), expect = each tensor's count spread evenly over its elements."""
    expect = [0.0] * L.nsuper
    for o, n, k in zip(L.offsets, L.sizes, counts):
        if k <= 0:
            continue
        dens = float(k) / float(n)
        for s in range(o >> SUPER_BITS, ((o + n - 1) >> SUPER_BITS) + 1):
            lo, hi = max(o, s << SUPER_BITS), min(o + n, (s + 1) << SUPER_BITS)
            expect[s] += dens * float(hi - lo)
    return [min(int(math.ceil(2.0 * e)) + 256, SUPER) for e in expect]


def super_counts(L, counts, indices):
    """How many in-range values of the message land in every super-tile."""
    koff = koff_of(counts)
    got = np.zeros(L.nsuper, np.int64)
    for t, (o, n) in enumerate(zip(L.offsets, L.sizes)):
        i = indices[koff[t]:koff[t + 1]]
        i = i[(i >= 0) & (i < n)]
        got += np.bincount((o + i) >> SUPER_BITS, minlength=L.nsuper)
    return got
