"""Inputs of the Top-K oracle matrix (tests/test_gpu_topk_matrix.py); tests/test_topk_matrix_host.py
checks, without a GPU, that they have the properties the matrix relies on.  Data recipes and numpy
arithmetic only: a seeded numpy Generator per tensor, no torch RNG, no GPU.

Four plans (arena_layout: every tensor starts at a multiple of 64 elements, so every size that is no
multiple of 64 leaves padding, and the odd sizes end inside a float4):

* ``edges``    15 small tensors, n = 1 .. 16385 around the 512-element sub-chunk, the 4096-element
               bucket and the 16384-element item, at ratios 0.01, 0.29, 1/3 and 1.0 (k == n).  The
               small ratios keep every element as a candidate; from n = 4095 on the large ones are sampled.
* ``sampled``  five tensors large enough to be sampled at both ratios (0.01, 0.1), sample_runs = 2048.
* ``many``     300 tensors (sizes cycling 1, 7, 100, 513, 5000; kinds cycling the seven basic ones, so
               every size meets every kind) at ratio 0.05: more than 256 tensors take the exact path.
* ``tight``    the tensors of ``edges`` packed as closely as the ABI allows — every start at the next
               multiple of 4 elements, so a tensor's padding is the 0 to 3 elements that complete its last
               float4 and a sub-chunk's 512 elements of the arena span several tensors — at ratios 0.01, 1/3.

Tensor kinds (the t' of a sequence's first call, up to the weighting alpha):

* ``gauss``          N(0, 1): no ties.
* ``quantised``      round(8 g) / 8: a few dozen magnitudes, ties everywhere and across rank k
                     (n < 16: +-0.5 alternating).
* ``all_equal``      one magnitude (0.75), mixed signs.
* ``sparse``         topk_k(n, 0.01) // 2 non-zeros (fewer than k at every ratio), the rest zeros,
                     every other one -0.0: the selection is completed by the lowest-index zeros.
* ``specials``       N(0, 1) with +-inf, three NaN (one payload, 0x7fc00000), +-FLT_MAX, subnormals
                     and signed zeros at random positions.
* ``ramp_up``        +-(i + 1): the largest magnitudes are the last elements (the tail sub-chunk, the
                     last partial float4).  ``ramp_down`` the reverse.
* ``sample_is_top``  (65536) the elements the sampler reads are 10.0, every other one 1.0.  Ratio 0.1:
                     4096 candidates < k = 6553, so the tensor is redone exactly.  Ratio 0.01: the 4096
                     equal keys are one fine bin over half a bucket: a big-bin bucket of the fast path.
* ``under_sampled``  (262144) 300 sampled elements in [1, 2), everything else below 0.5 but 4000
                     unsampled elements in [4, 8): the sample puts the sure magnitude inside [1, 2), so
                     more than k = 2621 keys are "sure" at ratio 0.01 and the bucket kernels must give t'
                     back to the ones past rank k.
* ``cluster``        (2^20) N(0, 1) with 5000 elements of magnitude exactly 2.0: inside the top k at
                     ratio 0.1 — one fine bin over a bucket's 4096 keys, so the device decides on the
                     fallback by itself — and below the sampled threshold at ratio 0.01, where the call
                     (every tensor of the plan: the verdict is the call's) stays on the fast path.

Later error-feedback calls add fresh N(0, scale) x, scale = the kind's (SCALE).
"""

import numpy as np

ALIGN = 64
FLT_MAX = np.finfo(np.float32).max
NAN_BITS = 0x7FC00000
CANARY = -3.0e38  # padding of x and of the residual: the largest magnitude of the arena if read as data
ALPHAS = (1.0, 3.0, 0.3)  # 0.3: every product rounds
SAMPLE_RUNS = 2048
BASIC = ("gauss", "quantised", "all_equal", "sparse", "specials", "ramp_up", "ramp_down")
N_CALLS = 3  # the error-feedback sequence: mode 2, then mode 1 twice


def arena_layout(sizes, align=ALIGN):
    """omnifed_amd.codec.arena_layout's offsets and the arena's end (offsets[-1] + sizes[-1])."""
    offs, cur = [], 0
    for n in sizes:
        offs.append(cur)
        cur += (int(n) + align - 1) // align * align
    return offs, offs[-1] + int(sizes[-1])


def topk_k(n, ratio):
    return max(1, int(n * float(ratio)))


class PlanSpec:
    def __init__(self, name, seed, sizes, kinds, ratios, align=ALIGN):
        self.name, self.seed = name, seed
        self.sizes, self.kinds, self.ratios = list(sizes), list(kinds), tuple(ratios)
        assert len(self.sizes) == len(self.kinds)
        self.offsets, self.arena_end = arena_layout(self.sizes, align)
        self.names = [f"{k}{n}@{t}" for t, (k, n) in enumerate(zip(self.kinds, self.sizes))]

    def ks(self, ratio):
        return [topk_k(n, ratio) for n in self.sizes]

    def tensor_of(self, kind):
        return self.kinds.index(kind)


_EDGE_SIZES = (1, 2, 3, 5, 100, 101, 511, 512, 513, 4095, 4096, 4097, 16383, 16384, 16385)
_EDGE_KINDS = tuple(BASIC[i % 7] for i in range(14)) + ("quantised",)
_MANY_SIZES = (1, 7, 100, 513, 5000)

PLANS = {
    "edges": PlanSpec("edges", 11, _EDGE_SIZES, _EDGE_KINDS, (0.01, 0.29, 1.0 / 3.0, 1.0)),
    "sampled": PlanSpec("sampled", 12, (70_001, 65_536, 262_144, 262_147, 1 << 20),
                        ("quantised", "sample_is_top", "under_sampled", "specials", "cluster"), (0.01, 0.1)),
    "many": PlanSpec("many", 13, [_MANY_SIZES[i % 5] for i in range(300)], [BASIC[i % 7] for i in range(300)],
                     (0.05,)),
    # the same tensors as edges (the same seed), every start at the next multiple of 4 elements
    "tight": PlanSpec("tight", 11, _EDGE_SIZES, _EDGE_KINDS, (0.01, 1.0 / 3.0), align=4),
}
SCALE = {"ramp_up": 0.25, "ramp_down": 0.25}  # x the tensor's size; every other kind: 1.0
UNDER_SAMPLED_HI, UNDER_SAMPLED_TOP = 300, 4000
CLUSTER_N, CLUSTER_MAG = 5000, 2.0


# ------------------------------------------------------------------ the sampler's positions

def _fmix32(h):
    h = h.astype(np.uint64)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    return h ^ (h >> np.uint64(16))


def _sample_positions(n, t, max_runs):
    """The elements omf_topk_sampled.hip's topk_sample reads for tensor t: one aligned run of 16 per
    max(256, ceil(n / max_runs)) elements, at a hashed position."""
    stride = max(256, -(-n // max_runs))
    lo = np.arange(0, n, stride, dtype=np.uint64)
    key = lo ^ np.uint64((t * 0x9E3779B9) & 0xFFFFFFFF)
    span = np.minimum(np.uint64(stride), np.uint64(n) - lo)
    runs = np.maximum(np.uint64(1), span // np.uint64(16))
    start = (lo + np.uint64(16) * (_fmix32(key) % runs)).astype(np.int64)
    pos = (start[:, None] + np.arange(16)[None, :]).reshape(-1)
    return pos[pos < n]


# ------------------------------------------------------------------ tensors

def _signs(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)


def _specials_list():
    """NaN, -inf, FLT_MAX, -0.0, a subnormal, +inf, NaN, NaN, -FLT_MAX, +0.0, -0.0, +inf, the smallest
    subnormal of either sign, a negative subnormal (tensors of n < 16 take the first n)."""
    bits = [NAN_BITS, 0xFF800000, 0x7F7FFFFF, 0x80000000, 0x000116C2, 0x7F800000, NAN_BITS, NAN_BITS, 0xFF7FFFFF,
            0x00000000, 0x80000000, 0x7F800000, 0x00000001, 0x80000001, 0x800116C2]
    return np.array(bits, np.uint32).view(np.float32)


def make_tensor(spec, t):
    """Tensor t of the plan (fp32), from its own fixed seed."""
    kind, n = spec.kinds[t], spec.sizes[t]
    rng = np.random.default_rng([spec.seed, t])
    if kind == "gauss":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "quantised":
        if n < 16:
            return np.where(np.arange(n) % 2 == 0, 0.5, -0.5).astype(np.float32)
        return (np.rint(8.0 * rng.standard_normal(n)) / 8.0).astype(np.float32)
    if kind == "all_equal":
        return np.float32(0.75) * _signs(rng, n)
    if kind == "sparse":
        x = np.zeros(n, np.float32)
        x[1::2] = -0.0
        nnz = topk_k(n, 0.01) // 2
        pos = rng.choice(n, nnz, replace=False)
        x[pos] = (rng.standard_normal(nnz) + 3.0).astype(np.float32) * _signs(rng, nnz)
        return x
    if kind == "specials":
        sp = _specials_list()
        if n < 16:
            return sp[:n].copy()
        x = rng.standard_normal(n).astype(np.float32)
        x[rng.choice(n, sp.size, replace=False)] = sp
        return x
    if kind in ("ramp_up", "ramp_down"):
        x = np.arange(1, n + 1, dtype=np.float32) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
        return x if kind == "ramp_up" else x[::-1].copy()
    if kind == "sample_is_top":
        x = np.ones(n, np.float32)
        x[_sample_positions(n, t, SAMPLE_RUNS)] = 10.0
        return x
    if kind == "under_sampled":
        sp = _sample_positions(n, t, SAMPLE_RUNS)
        x = rng.uniform(0.05, 0.45, n)
        hi = rng.choice(sp, UNDER_SAMPLED_HI, replace=False)
        x[hi] = rng.uniform(1.0, 1.99, UNDER_SAMPLED_HI)
        rest = np.setdiff1d(np.arange(n), sp)
        top = rng.choice(rest, UNDER_SAMPLED_TOP, replace=False)
        x[top] = rng.uniform(4.0, 7.99, UNDER_SAMPLED_TOP)
        return x.astype(np.float32) * _signs(rng, n)
    if kind == "cluster":
        x = rng.standard_normal(n).astype(np.float32)
        pos = rng.choice(n, CLUSTER_N, replace=False)
        x[pos] = np.float32(CLUSTER_MAG) * _signs(rng, CLUSTER_N)
        return x
    raise ValueError(kind)


def scale_of(spec, t):
    return SCALE.get(spec.kinds[t], 0.0) * spec.sizes[t] or 1.0


def make_arena(spec, call=0):
    """The x arena of call ``call`` of a sequence (call 0: the kinds above; later: N(0, scale)), with
    CANARY in the padding."""
    x = np.full(spec.arena_end, CANARY, np.float32)
    for t, (o, n) in enumerate(zip(spec.offsets, spec.sizes)):
        if call == 0:
            x[o:o + n] = make_tensor(spec, t)
        else:
            rng = np.random.default_rng([spec.seed, t, call])
            x[o:o + n] = (rng.standard_normal(n) * scale_of(spec, t)).astype(np.float32)
    return x


def padding_mask(spec):
    pad = np.ones(spec.arena_end, bool)
    for o, n in zip(spec.offsets, spec.sizes):
        pad[o:o + n] = False
    return pad
