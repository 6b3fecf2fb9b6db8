"""The opt-in quantised Top-K value wire ("TopKQuantPackedCompression") restated in numpy from this
repository's own oracle, and the recipes of its tests (tests/test_topk_qval_host.py,
tests/test_gpu_topk_qval_matrix.py, tests/test_gpu_topk_qval_wire.py).

The quantiser, per tensor t with its k selected fp32 values v (the selection's order):

* scale  m = max |v| (exact; NaN when a value is NaN);
* levels ``oracle.qsgd.qsgd_quantize(v, s, norm=m, u=u)`` with L = 2^s and
  u = ``oracle.philox.philox_uniforms(seed, offset, t, k)`` — "element" is the position in the selection;
* code   q + L in b = s + 2 bits, packed by ``oracle.bitpack.pack`` (LSB-first little-endian);
* decode d = fl32(fl32(m q) / L) (``oracle.qsgd.qsgd_dequantize``);
* error feedback e = fl32(v - d) stored at residual[offsets[t] + index], indices outside [0, n) skipped;
* m = 0: every code L, no draw, no store;  m NaN, infinite or above FLT_MAX / L: nothing written.

The value arena of a count vector: a group of 32 consecutive values of a tensor is b whole 32-bit words, group
g (counted over the whole selection, goff[t] = sum_{u<t} ceil(k_u / 32)) at word g b; the codes after a tensor's
k_t-th value are 0.

Nothing here imports the package under test.
"""

import numpy as np
import torch

from oracle import bitpack, philox, qsgd

GROUP = 32
FLT_MAX = float(np.finfo(np.float32).max)
CANARY_WORD = np.uint32(0xC0DEFACE)
CANARY_FLOAT = np.array([0xC0DEFACE], np.uint32).view(np.float32)[0]  # about -6.96, a plain finite number


def code_bits(s):
    s = int(s)
    if not 1 <= s <= 8:
        raise ValueError(f"value_bits = {s} outside 1..8")
    assert bitpack.packed_bits(2**s) == s + 2
    return s + 2


def scale_of(v):
    """max |v| as the unsigned maximum of the magnitudes' bits (NaN above inf); 0 for no value."""
    v = np.ascontiguousarray(v, np.float32)
    if v.size == 0:
        return np.float32(0.0)
    return np.array([(v.view(np.uint32) & np.uint32(0x7FFFFFFF)).max()], np.uint32).view(np.float32)[0]


def usable(m, s):
    """Finite, and m L does not overflow fp32."""
    m = float(m)
    return bool(np.isfinite(m) and 0.0 <= m <= FLT_MAX / 2.0**s)


def quantize(v, s, seed, offset, t, m=None):
    """One tensor's selection: ``(m, q, d, e)`` — the scale, the signed levels (int64), the decoded values and
    the error fl32(v - d), all of v's length; ``(m, None, None, None)`` for an unusable scale."""
    v = np.ascontiguousarray(v, np.float32)
    L = 2**int(s)
    m = scale_of(v) if m is None else np.float32(m)
    if not usable(m, s):
        return m, None, None, None
    if m == 0 or v.size == 0:
        q = np.zeros(v.size, np.int64)
    else:
        u = philox.philox_uniforms(int(seed), int(offset), int(t), v.size)
        qt, norm, _w, lv = qsgd.qsgd_quantize(torch.from_numpy(v.copy()), int(s), norm=float(m), u=torch.from_numpy(u))
        assert norm == float(m) and lv == L
        q = qt.numpy().astype(np.int64)
    d = dequantize(q, m, s)
    with np.errstate(all="ignore"):
        e = (v - d).astype(np.float32)
    return m, q, d, e


def dequantize(q, m, s):
    """d = fl32(fl32(m q) / L) for signed levels q (any integers: a receiver decodes what it is sent)."""
    q = np.asarray(q, np.int64)
    if q.size == 0:
        return np.zeros(0, np.float32)
    out = qsgd.qsgd_dequantize(torch.from_numpy(q.astype(np.int32)), float(m), 2**int(s), q.shape)
    return out.numpy().astype(np.float32)


def pack_codes(q, s):
    """values_data of a layer: the codes q + L, ceil(k b / 8) bytes."""
    return bitpack.pack(np.asarray(q, np.int64), 2**int(s))


def unpack_codes(data, k, s):
    return bitpack.unpack(data, int(k), 2**int(s))


def bits_of(codes, b):
    codes = np.asarray(codes, dtype=np.uint64).reshape(-1)
    return ((codes[:, None] >> np.arange(b, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)


def group_offsets(counts):
    goff = [0]
    for k in counts:
        goff.append(goff[-1] + -(-int(k) // GROUP))
    return goff


def value_arena(counts, codes, s, base=None, pad_ones=False):
    """The value arena's words (uint32): tensor t's ``codes[t]`` (unsigned, or None: the tensor's words keep
    ``base``'s — a skipped tensor) from word goff[t] b.  ``pad_ones``: the bits past a tensor's k_t b are 1
    (what a receiver must ignore) instead of the 0 a sender writes."""
    b = code_bits(s)
    goff = group_offsets(counts)
    out = np.zeros(goff[-1] * b, np.uint32) if base is None else np.array(base, np.uint32)
    assert out.size >= goff[-1] * b
    for t, k in enumerate(counts):
        if codes[t] is None or k == 0:
            continue
        nw = (goff[t + 1] - goff[t]) * b
        bits = np.full(32 * nw, 1 if pad_ones else 0, np.uint8)
        bits[:k * b] = bits_of(codes[t], b)
        out[goff[t] * b:goff[t] * b + nw] = np.packbits(bits, bitorder="little").view("<u4")
    return out


def stream_bytes(counts, t, s):
    """(first byte, length) of tensor t's code stream in the arena: what the wire sends."""
    b = code_bits(s)
    return 4 * group_offsets(counts)[t] * b, (int(counts[t]) * b + 7) // 8


def residual_after(residual, offsets, sizes, indices, es):
    """The residual arena after the quantiser's stores: e at offsets[t] + index for the tensors with an error
    vector (None: nothing stored), indices outside [0, n_t) skipped."""
    out = np.array(residual, np.float32)
    for t, (ix, e) in enumerate(zip(indices, es)):
        if e is None:
            continue
        ok = (ix >= 0) & (ix < sizes[t])
        out[offsets[t] + ix[ok]] = e[ok]
    return out


# ---------------------------------------------------------------- the worked vector
# s = 2: L = 4, b = 4.  v = [3, -1.5, 0.75]: m = 3, |v| / m L = 4, 2, 1 — whole levels, so no draw matters:
# q = [4, -2, 1], codes [8, 2, 5] -> nibbles 8, 2 | 5, 0 -> b"\x28\x05"; d = 3 q / 4 = v, e = 0.
WORKED = dict(s=2, v=[3.0, -1.5, 0.75], m=3.0, q=[4, -2, 1], data=b"\x28\x05", d=[3.0, -1.5, 0.75])


# ---------------------------------------------------------------- the device matrix
# k_t in {0, 1, 31, 32, 33, 4097, 8191, 8193}: a partial group, a workgroup's run of 256 groups = 8192 values
# crossed inside a tensor, the Philox layout's 1024- and 4096-element periods; then the scale's edge cases.
MATRIX_SIZES = [7, 1, 40, 32, 100, 5000, 9000, 8193, 64, 64, 64, 64, 50]
MATRIX_COUNTS = [0, 1, 31, 32, 33, 4097, 8191, 8193, 40, 40, 40, 40, 33]
T_ZEROS, T_INF, T_NAN, T_BIG, T_SUB, T_BADIDX = 8, 9, 10, 11, 12, 4
UNUSABLE = (T_INF, T_NAN, T_BIG)


def matrix_values(seed=3):
    """Per tensor its selected values: magnitudes over many binades, +-0 and subnormals among them, the
    maximum present with both signs; an all-(+-0) tensor, one with an infinity, one with a NaN, one whose
    maximum is FLT_MAX (above FLT_MAX / L for every L), one of subnormals and zeros alone."""
    rng = np.random.default_rng(seed)
    out = []
    for t, k in enumerate(MATRIX_COUNTS):
        v = (rng.standard_normal(k) * np.exp2(rng.integers(-12, 4, k))).astype(np.float32)
        if k >= 8:
            v[1], v[2], v[3] = 0.0, -0.0, 1e-41
            v[5], v[k - 1] = np.abs(v).max(), -np.abs(v).max()
        if t == T_ZEROS:
            v = np.where(np.arange(k) % 3 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        if t == T_INF:
            v[7] = -np.inf
        if t == T_NAN:
            v[11] = np.nan
        if t == T_BIG:
            v[13] = FLT_MAX
        if t == T_SUB:
            v = (rng.integers(-2000, 2000, k) * np.float64(2.0**-149)).astype(np.float32)
            v[4] = -0.0
        out.append(v)
    return out


def matrix_indices(seed=4):
    """Per tensor k_t distinct indices in [0, n_t) in random order; tensor T_BADIDX also holds n, -1 and 2^40."""
    rng = np.random.default_rng(seed)
    out = [rng.permutation(n)[:k].astype(np.int64) for n, k in zip(MATRIX_SIZES, MATRIX_COUNTS)]
    out[T_BADIDX][[2, 9, 20]] = [MATRIX_SIZES[T_BADIDX], -1, 2**40]
    return out


# ---------------------------------------------------------------- the wire test's dict
WIRE_SIZES = [70_000, 4_096, 33, 1]
WIRE_RATIOS = [0.01, 0.25]


def llama400m_miniature(div=1024):
    """Llama-400M's shapes (2 x 32 768 000, 80 x 2^20, 60 x 2^22, 41 x 1024 elements) with every tensor's
    element count divided by ``div`` (at least 1): 183 tensors of the same proportions."""
    sizes = [32_768_000] * 2 + [2**20] * 80 + [2**22] * 60 + [1024] * 41
    return [max(1, n // div) for n in sizes]
