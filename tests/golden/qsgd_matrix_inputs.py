"""Inputs and reference helpers of the QSGD oracle matrix (tests/test_gpu_qsgd_matrix.py,
tests/test_gpu_qsgd_decode_matrix.py); tests/test_qsgd_matrix_host.py checks, without a GPU, that
they have the properties the matrix relies on.  Data recipes and numpy arithmetic only.

The encoder arena: eight "shape" tensors and the "level" tensors behind them.

* ``one``       n = 1: vn = 1, so the level is exactly L (fp16, s >= 16: 0 by the inf rule).
* ``five``      n = 5.
* ``gauss``     n = 4102: N(0, 1e-3), -0.0 at 1/16 of the positions and as the last element, and one
                element of 0.05 (|vn| > 0.5: fp16's inf rule reaches this tensor from s = 17 on).
* ``dominant``  n = 16385: one element with 0.99 of the norm, values at (1 - 0.01)/16 and
                -(2 - 0.01)/16 of the norm, noise of 1e-5 and -0.0 elsewhere.
* ``heavy``     n = 70001: N(0,1) 10^U(-3,3), and one element of -0.6 of the others' norm (again
                for the inf rule at s = 17); sampled by the bracketed encoder, five ring chunks.
* ``zero``      n = 1003: +0.0 and -0.0 only.  Norm 0, all-zero payload.
* ``tiny``      n = 3002: N(0,1) 1e-12.  The fp32 squares are normal; in fp16 every element rounds
                to zero, a second zero-norm tensor for that format.
* ``minus``     n = 2: -0.3 and -0.0, so vn = -1 and the level is exactly -L at every s.
* level tensors: a tensor's normalised values have squares summing to 1, so one tensor can hold
  only a few of the values (j - 0.01)/16, j = 1..16 of either sign (their squares sum to 11.7).
  They are packed first-fit into small tensors (LEVEL_GROUPS), each completed by one element that
  carries the rest of the norm and then scaled (norms from 1e-2 to 1e2); every such tensor has an
  element of |vn| > 0.5.  With them every level -L..L occurs at every s <= 4.

Every size but 1 leaves a partial last quad.
"""

import hashlib

import numpy as np

ALIGN = 64
BASE = (("one", 1), ("five", 5), ("gauss", 4102), ("dominant", 16385), ("heavy", 70001), ("zero", 1003),
        ("tiny", 3002), ("minus", 2))
ZERO_T, TINY_T, FIVE_T, HEAVY_T = 5, 6, 1, 4
SEED, OFFSET = 0x9E37_79B9_7F4A_7C15, 7  # bits above 2^32 in the seed, a non-zero call offset
DIVISOR = 3.0
BITS = (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 16, 17, 24, 30)


def _level_groups(L=16):
    """The values +-(j - 0.01)/L, j = 1..L, packed first-fit (largest first) into groups whose squares
    leave room for one more element of |vn| >= 0.55 unless the group's first value is one itself."""
    vals = sorted((sg * (j - 0.01) / L for j in range(1, L + 1) for sg in (1.0, -1.0)), key=lambda r: (-abs(r), r))
    groups, room = [], []
    for r in vals:
        for i in range(len(groups)):
            if room[i] >= r * r:
                groups[i].append(r)
                room[i] -= r * r
                break
        else:
            groups.append([r])
            room.append((1.0 - 1e-6 if abs(r) >= 0.5 else 0.69) - r * r)
    return groups


LEVEL_GROUPS = _level_groups()


def _level_size(k):
    n = len(LEVEL_GROUPS[k]) + 4  # the group, the element carrying the rest of the norm, three of noise / -0.0
    return n if n % 4 else n + 1 + k % 3  # never a multiple of 4


SIZES = [n for _, n in BASE] + [_level_size(k) for k in range(len(LEVEL_GROUPS))]
NAMES = [name for name, _ in BASE] + [f"level{k}" for k in range(len(LEVEL_GROUPS))]


def arena_layout(sizes, align=ALIGN):
    """omnifed_amd.codec.arena_layout's offsets (starts at multiples of 64 elements) and arena_end."""
    offs, cur = [], 0
    for n in sizes:
        offs.append(cur)
        cur += (int(n) + align - 1) // align * align
    return offs, offs[-1] + int(sizes[-1])


OFFSETS, ARENA_END = arena_layout(SIZES)


def _neg_zeros(rng, x):
    n = x.size
    if n >= 16:
        x[rng.choice(n, n // 16, replace=False)] = -0.0


def make_tensor(t):
    """Tensor t of the encoder arena (fp32), from its own fixed seed."""
    rng = np.random.default_rng(7000 + t)
    name, n = NAMES[t], SIZES[t]
    if name == "one":
        return np.array([0.7], np.float32)
    if name == "five":
        return (rng.standard_normal(n) * 0.1).astype(np.float32)
    if name == "gauss":
        x = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        _neg_zeros(rng, x)
        x[int(rng.integers(0, n - 1))] = 0.05
        x[n - 1] = -0.0
        return x
    if name == "dominant":
        x = (rng.standard_normal(n) * 1e-5).astype(np.float32)
        _neg_zeros(rng, x)
        p0, p1, p2 = rng.choice(n - 1, 3, replace=False)
        r1, r2 = (1 - 0.01) / 16, (2 - 0.01) / 16
        x[p1], x[p2] = r1, -r2
        x[p0] = -np.sqrt(1.0 - r1 * r1 - r2 * r2)
        x[n - 1] = -0.0
        return x
    if name == "heavy":
        z = rng.standard_normal(n) * np.power(10.0, rng.uniform(-3.0, 3.0, n))
        p = int(rng.integers(0, n - 1))
        z[p] = 0.0
        z[p] = -0.6 * np.sqrt(np.sum(z * z))
        return z.astype(np.float32)
    if name == "zero":
        x = np.zeros(n, np.float32)
        x[::16] = -0.0
        x[n - 1] = -0.0
        return x
    if name == "tiny":
        return (rng.standard_normal(n) * 1e-12).astype(np.float32)
    if name == "minus":
        return np.array([-0.3, -0.0], np.float32)
    g = LEVEL_GROUPS[t - len(BASE)]
    x = (rng.standard_normal(n) * 1e-5).astype(np.float32)
    pos = rng.permutation(n - 1)[:len(g) + 1]  # the last element stays free: it is -0.0
    x[pos[:-1]] = np.array(g, np.float32)
    rest = np.sqrt(max(0.0, 1.0 - float(np.sum(np.square(g)))))
    x[pos[-1]] = rest if t % 2 else -rest
    x[n - 1] = -0.0
    return x * np.float32(10.0 ** ((t - len(BASE) - 6) / 3.0))  # norms from 1e-2 to 1e2


def make_arena():
    """The fp32 encoder arena (padding zero)."""
    x = np.zeros(ARENA_END, np.float32)
    for t, (o, n) in enumerate(zip(OFFSETS, SIZES)):
        x[o:o + n] = make_tensor(t)
    return x


def make_side_inputs():
    """Everything else a cell reads, in the arena layout: caller uniforms ``u``; caller norms ``norm_in``
    (``five``'s so small that |vn| L passes 2^63: level 0; a non-zero one for ``zero``; 0 for the first
    level tensor: all-zero payload); the last client's payloads ``q8`` (the whole int8 range, -128
    included) and ``q32`` (beyond both levels_in, and INT32_MIN / INT32_MAX / +-(2^24 + 1)) and its norms
    ``anorm`` (0 for ``zero``: a tensor absent from its message)."""
    rng = np.random.default_rng(99)
    nt = len(SIZES)
    u = rng.random(ARENA_END, dtype=np.float32)
    norm_in = (0.05 + rng.random(nt)).astype(np.float32)
    norm_in[FIVE_T] = 1e-20
    norm_in[ZERO_T] = 0.5
    norm_in[len(BASE)] = 0.0
    anorm = (0.01 + 0.01 * rng.random(nt)).astype(np.float32)
    anorm[ZERO_T] = 0.0
    q8 = rng.integers(-128, 128, ARENA_END).astype(np.int8)
    q32 = rng.integers(-4096, 4097, ARENA_END).astype(np.int32)
    for t in (0, 2, HEAVY_T):
        q8[OFFSETS[t]] = -128
    h = OFFSETS[HEAVY_T]
    q32[h + 5:h + 9] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, (1 << 24) + 1, -(1 << 24) - 1]
    q8[OFFSETS[1] + 4] = 127
    return {"u": u, "norm_in": norm_in, "anorm": anorm, "q8": q8, "q32": q32}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------ reference helpers

def norm64(v):
    """The fp64 L2 norm of an array."""
    return float(np.sqrt(np.sum(np.asarray(v, np.float64) ** 2)))


def round_to_format(x, fmt):
    """The fp64 value x rounded once (to nearest even) to "bf16" or "fp16", as a Python float."""
    x = float(x)
    if fmt == "fp16":
        with np.errstate(over="ignore"):
            return float(np.float64(x).astype(np.float16))
    if x == 0.0 or not np.isfinite(x):
        return x
    m, e = np.frexp(x)  # bf16: 8 significant bits, fp32's exponent range (no subnormal norms here)
    return float(np.ldexp(np.rint(m * 256.0) / 256.0, e))


def half_norm_bounds(ref, fmt, rtol=2e-6):
    """[lo, hi]: a norm within rtol of the fp64 norm ``ref``, rounded to the format, lies in it."""
    return round_to_format(ref * (1.0 - rtol), fmt), round_to_format(ref * (1.0 + rtol), fmt)


def half_norm_ok(norm, ref, fmt, rtol=2e-6):
    """``norm`` is a value of the format and lies in ``half_norm_bounds``."""
    lo, hi = half_norm_bounds(ref, fmt, rtol)
    norm = float(norm)
    return round_to_format(norm, fmt) == norm and lo <= norm <= hi


def decode_ref(q, norm, levels):
    """fl32(fl32(norm * q) / fl32(levels)) in numpy: oracle.qsgd_dequantize's op sequence."""
    with np.errstate(all="ignore"):
        return ((np.float32(norm) * np.asarray(q).astype(np.float32)) / np.float32(levels)).astype(np.float32)


# ------------------------------------------------------------------ the decode matrix's arena

DEC_SIZES = [1, 3, 5, 64, 1000, 4095, 4097, 10, 13001, 2, 9]
DEC_NORMS = (0.0, -0.0, 1.0, 0.37, 1e-40, 3e38, float("inf"), float("nan"))
DEC_LEVELS = {8: (1, 2, 10, 16, 127), 32: (128, 1000, 1 << 24, (1 << 24) + 1, 1 << 30, (1 << 31) - 1)}


def dec_layout():
    """Starts at multiples of 4 with caller-chosen gaps (some none); tensor 8 has whole 4096-blocks inside."""
    rng = np.random.default_rng(4242)
    offsets, cur = [], 0
    for n in DEC_SIZES:
        cur = (cur + 3) // 4 * 4 + 4 * int(rng.integers(0, 40))
        offsets.append(cur)
        cur += n
    return offsets, cur


def dec_payload(width, levels, arena_end):
    """A payload arena (padding included: a decoder must not use it): width 8 the whole int8 range;
    width 32 random values mixed with 0, +-1, +-levels, +-(2^24 + 1), +-2^30, INT32_MIN and INT32_MAX."""
    rng = np.random.default_rng(1000 + width + levels % 9973)
    if width == 8:
        q = rng.integers(-128, 128, arena_end).astype(np.int8)
        q[rng.choice(arena_end, arena_end // 8, replace=False)] = -128
        return q
    i32 = np.iinfo(np.int32)
    q = rng.integers(-min(2 * levels, i32.max), min(2 * levels, i32.max), arena_end, dtype=np.int64).astype(np.int32)
    special = np.array([0, 1, -1, levels, -levels, (1 << 24) + 1, -(1 << 24) - 1, 1 << 30, -(1 << 30), i32.min,
                        i32.max], np.int64).astype(np.int32)
    where = rng.random(arena_end) < 0.5
    q[where] = special[rng.integers(0, special.size, int(where.sum()))]
    return q
