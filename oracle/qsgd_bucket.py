"""Bucketed QSGD restated in numpy — TEST INFRASTRUCTURE ONLY.

Not part of the reference (bucket norms are the QSGD paper's §3.3, a new ``compression_type``); what it restates is
the header of ``omnifed_amd/csrc/omf_qsgd_bucket.h``: bucket j of a tensor is elements [j d, min((j + 1) d, n)), and
a bucket's norm is ``fl32(sqrt(sum v^2))`` with the fp32 summation order of the header's steps 1-5, so the norm
bits depend only on the bucket's values and on d:

1. quad sums ``fma(v3, v3, fma(v2, v2, fma(v1, v1, fma(v0, v0, +0))))`` (absent elements of a short last bucket
   are +0);
2. d > 1024: quad i of row r is ``i = 256 r + lane``; the rows of one lane are added ``r ^ 1``, then ``r ^ 2``;
3. and 4. the xor butterfly over a row's lanes and the ``w ^ 1``, ``w ^ 2`` wave step: an adjacent-pair tree over
   the row's quads (fp32 + commutes exactly, so every lane of the butterfly holds the tree's bits);
5. a correctly rounded fp32 ``sqrt``.

Plain IEEE arithmetic, subnormals included; every add rounds to fp32.  The levels and the decode are the per-tensor
oracle's (``oracle.qsgd_quantize`` / ``qsgd_dequantize``) on each bucket.
"""

from __future__ import annotations

import numpy as np
import torch

from .qsgd import qsgd_dequantize, qsgd_quantize

F32 = np.float32


def fma_sq(a: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fp32 ``fma(a, a, c)``, rounded once.  ``a * a`` is exact in float64 (48 bits); the float64 sum with ``c``
    is rounded to odd (TwoSum gives the error term), so the cast to fp32 cannot double-round: 53 >= 24 + 2."""
    a = np.asarray(a, dtype=F32)
    c = np.asarray(c, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = a.astype(np.float64) * a.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0.0)
        bits = np.atleast_1d(s).view(np.int64).copy()
        even = (bits & 1) == 0
        # an even s moves one float64 towards the exact sum: the odd neighbour
        step = np.where((np.atleast_1d(err) > 0.0) == (np.atleast_1d(s) > 0.0), 1, -1)
        bits = np.where(np.atleast_1d(fix) & even, bits + step, bits)
        return bits.view(np.float64).reshape(np.shape(s)).astype(F32)


def quad_sums(v: np.ndarray, d: int) -> np.ndarray:
    """Step 1 of every bucket of one tensor: (nb, d / 4) fp32 quad sums, the last bucket padded with +0."""
    v = np.asarray(v, dtype=F32).reshape(-1)
    nb = -(-v.size // d)
    pad = np.zeros(nb * d, dtype=F32)
    pad[:v.size] = v
    q = pad.reshape(nb, d // 4, 4)
    s = np.zeros((nb, d // 4), dtype=F32)
    for k in range(4):
        s = fma_sq(q[:, :, k], s)
    return s


def pair_tree(s: np.ndarray) -> np.ndarray:
    """The adjacent-pair tree over the last axis (a power of two), every add rounded to fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        while s.shape[-1] > 1:
            s = (s[..., 0::2] + s[..., 1::2]).astype(F32)
    return s[..., 0]


def bucket_sums(v: np.ndarray, d: int) -> np.ndarray:
    """Steps 1-4: the fp32 sum of squares of every bucket of one tensor."""
    s = quad_sums(v, d)
    if d > 1024:  # step 2: the rows' sums of one lane, r ^ 1 and then r ^ 2
        s = s.reshape(s.shape[0], d // 1024, 256)
        with np.errstate(invalid="ignore", over="ignore"):
            while s.shape[1] > 1:
                s = (s[:, 0::2, :] + s[:, 1::2, :]).astype(F32)
        s = s[:, 0, :]
    return pair_tree(s)


def bucket_norms(v, d: int) -> np.ndarray:
    """The ``ceil(n / d)`` fp32 bucket norms of one tensor ``v = fl32(alpha x)``, by the header's steps 1-5."""
    d = int(d)
    if d < 64 or d > 4096 or d & (d - 1):
        raise ValueError("bucket size must be a power of two in [64, 4096]")
    v = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    if v.dtype != F32:
        raise ValueError("bucket_norms takes fp32 values")
    with np.errstate(invalid="ignore"):
        return np.sqrt(bucket_sums(v, d)).astype(F32)


def _scaled(x, alpha: float) -> torch.Tensor:
    x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return x.reshape(-1).float() * torch.tensor(alpha, dtype=torch.float32)  # fl32(alpha x)


def encode_bucketed(x, alpha: float, s: int, d: int, u, bnorm=None):
    """One tensor's bucketed encode: ``(levels int64, bnorm fp32)``, each bucket ``oracle.qsgd_quantize`` of
    ``fl32(alpha x)`` against its own norm (``bucket_norms``, or the caller's ``bnorm``) and its slice of ``u``."""
    v = _scaled(x, alpha)
    n = v.numel()
    bnorm = bucket_norms(v, d) if bnorm is None else np.asarray(bnorm, dtype=F32)
    u = u if isinstance(u, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(u))
    out = torch.empty(n, dtype=torch.int64)
    for j in range(-(-n // d)):
        lo, hi = j * d, min((j + 1) * d, n)
        out[lo:hi] = qsgd_quantize(v[lo:hi], s, norm=float(bnorm[j]), u=u[lo:hi])[0].long()
    return out, bnorm


def decode_bucketed(q, bnorm, L: int, d: int) -> torch.Tensor:
    """One tensor's bucketed decode: ``fl32(fl32(norm_b q) / L)`` per bucket (``oracle.qsgd_dequantize``)."""
    q = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q))
    q = q.reshape(-1)
    n = q.numel()
    out = torch.empty(n, dtype=torch.float32)
    for j in range(-(-n // d)):
        lo, hi = j * d, min((j + 1) * d, n)
        out[lo:hi] = qsgd_dequantize(q[lo:hi], float(bnorm[j]), L, (-1,)).float()
    return out
