"""Inputs of the bucketed-QSGD oracle matrix (tests/test_gpu_qsgd_bucket_matrix.py); tests/test_qsgd_bucket_oracle_host.py
checks, without a GPU, that they have the properties the matrix relies on.  Data recipes and numpy arithmetic only.

One arena per bucket size d, every tensor from its own fixed seed:

* the shape tensors (SHAPES): less than a quad, around a 32-element group, a bucket, a 4 Ki block and a 16 Ki item,
  a partial group inside a partial bucket in a block's second row.  N(0, 1e-3), -0.0 at 1/16 of the positions.
* ``many``     64 d + d / 2 + 3 elements, N(0, 1e-3): 65 buckets whose norm bits a change of summation order moves
               (the host test counts them), across several 16 Ki items at every d.
* ``special``  8 d elements, one bucket each:
    0 ordinary; 1 all +0 / -0; 2 ordinary; 3 one non-zero element (norm exactly |v|, its level exactly -L);
    4 N(0, 1) 1e-20 with |z| held to [0.01, 8]: every square is an fp32 subnormal;
    5 N(0, 1) 1e-25 with |z| held to [0.01, 8]: every square underflows to 0 — norm 0 over non-zero values;
    6 |values| in 3e19 [0.9, 1.1]: the first square is already +inf; norm inf;
    7 ordinary.
* ``nan``      3 d elements, one NaN in the middle bucket.

``message``: a payload no encoder made (levels uniform in [-L, L], bucket norms in [0, 4) with zeros), for the decode
sums and the PS step.
"""

import numpy as np

ALIGN = 64
SEED, OFFSET = 0xB0C_0000_0003, 3  # bits above 2^32 in the seed, a non-zero call offset
ONE_VALUE, ONE_AT = -2.5e-3, 7     # special bucket 3
S_ZERO, S_ONE, S_SUBNORMAL, S_UNDERFLOW, S_INF = 1, 3, 4, 5, 6  # buckets of ``special``


def shapes(d):
    return [1, 3, 31, 33, d - 1, d, d + 1, 2 * d + 5, 4095, 4096, 4097, 4096 + d + 1, 16383, 16384 + d // 2 + 3]


N_SHAPES = len(shapes(64))
MANY_T, SPECIAL_T, NAN_T = N_SHAPES, N_SHAPES + 1, N_SHAPES + 2


def sizes(d):
    return shapes(d) + [64 * d + d // 2 + 3, 8 * d, 3 * d]


def arena_layout(sz, align=ALIGN):
    """omnifed_amd.codec.arena_layout's offsets (starts at multiples of 64 elements) and arena_end."""
    offs, cur = [], 0
    for n in sz:
        offs.append(cur)
        cur += (int(n) + align - 1) // align * align
    return offs, offs[-1] + int(sz[-1])


def bucket_layout(sz, d):
    """omnifed_amd.codec.bucket_layout: the tensors' offsets into the bucket-norm arena, and its length."""
    boff, nb = [], 0
    for n in sz:
        boff.append(nb)
        nb += -(-int(n) // d)
    return boff, nb


def _gauss(rng, n, scale=1e-3):
    x = (rng.standard_normal(n) * scale).astype(np.float32)
    if n >= 16:
        x[rng.choice(n, n // 16, replace=False)] = -0.0
    return x


def _held(rng, n, scale):
    z = rng.standard_normal(n)
    return (np.sign(z) * np.clip(np.abs(z), 0.01, 8.0) * scale).astype(np.float32)


def make_tensor(d, t):
    """Tensor t of the arena of bucket size d (fp32)."""
    rng = np.random.default_rng(0xB0C0000 + 64 * d + t)
    n = sizes(d)[t]
    if t < N_SHAPES:
        return _gauss(rng, n)
    if t == MANY_T:
        return (rng.standard_normal(n) * 1e-3).astype(np.float32)
    if t == NAN_T:
        x = _gauss(rng, n)
        x[d + d // 2] = np.nan
        return x
    x = _gauss(rng, n)
    b = lambda j: slice(j * d, (j + 1) * d)
    x[b(S_ZERO)] = np.where(np.arange(d) % 3 == 0, -0.0, 0.0).astype(np.float32)
    x[b(S_ONE)] = 0.0
    x[S_ONE * d + ONE_AT] = ONE_VALUE
    x[b(S_SUBNORMAL)] = _held(rng, d, 1e-20)
    x[b(S_UNDERFLOW)] = _held(rng, d, 1e-25)
    x[b(S_INF)] = (np.where(rng.random(d) < 0.5, -1.0, 1.0) * rng.uniform(0.9, 1.1, d) * 3e19).astype(np.float32)
    return x


def tensors(d):
    return [make_tensor(d, t) for t in range(len(sizes(d)))]


# (tensor, bucket) beside a zero, underflow, inf or NaN bucket: their norms and levels must be their own
NEIGHBOURS = ((SPECIAL_T, S_ZERO - 1), (SPECIAL_T, S_ZERO + 1), (SPECIAL_T, S_UNDERFLOW - 1), (SPECIAL_T, S_INF),
              (SPECIAL_T, S_UNDERFLOW), (SPECIAL_T, S_INF + 1), (NAN_T, 0), (NAN_T, 2))


def message(payload_elems, nb, L, seed):
    """``(levels int32[payload_elems], bucket norms fp32[nb])``: levels uniform in [-L, L]; norms in [0, 4), every
    7th one zero (its terms are +0 or -0 by the level's sign)."""
    rng = np.random.default_rng(0x5E55 + seed)
    q = rng.integers(-L, L + 1, payload_elems).astype(np.int32)
    bn = (rng.random(nb) * 4.0).astype(np.float32)
    bn[::7] = 0.0
    return q, bn


def decode_np(q, bn, bidx, L):
    """The decode rule on an arena: ``fl32(fl32(norm_b q) / L)`` with ``bidx`` every element's bucket."""
    with np.errstate(invalid="ignore", over="ignore"):
        return ((bn[bidx] * q[:bidx.size].astype(np.float32)).astype(np.float32) / np.float32(L)).astype(np.float32)
