"""Top-K oracle: the reference's torch-CPU op sequence, restated — TEST INFRASTRUCTURE ONLY.

Follows ``/root/reference/src/omnifed/hybrid/compression/``:

* ``topk_k``          ↔ ``max(1, int(numel * ratio))`` (topk.py:12)
* ``topk_sparse``     ↔ ``topk_sparse`` (topk.py:10-15): ``torch.topk(|x|, k, sorted=False)``
* ``topk_desparse``   ↔ ``topk_desparse`` (topk.py:18-21)
* ``TopKOracle``      ↔ ``TopKCompression.compress/decompress`` (topk.py:24-47) with
  ``ResidualUpdates`` error feedback (core.py:19-37, beta = gamma = 1)

``torch.topk``'s output order is implementation defined and ties are unspecified
(SURVEY.md §7 hard part 6), so tests compare index *sets* and decoded tensors.

The device's own order (include/omf_codec.h, omf_topk_encode: descending |t'| as the unsigned
integer ``bits(t') & 0x7fffffff``, ties by ascending index) is fully determined, so it has an
exact oracle too: ``topk_select_index_order`` and, with the error-feedback arithmetic of one
call in fp32 numpy, ``topk_ef_step``.
"""

from __future__ import annotations

import numpy as np
import torch


def topk_k(numel: int, ratio: float) -> int:
    return max(1, int(numel * float(ratio)))


def topk_sparse(t: torch.Tensor, ratio: float):
    flat = t.flatten()
    k = topk_k(flat.numel(), ratio)
    _, idx = torch.topk(flat.abs(), k, sorted=False)
    return torch.gather(flat, 0, idx), idx


def topk_desparse(values: torch.Tensor, indices: torch.Tensor, numel: int) -> torch.Tensor:
    out = torch.zeros(numel, dtype=values.dtype)
    out.scatter_(0, indices, values)
    return out


class TopKOracle:
    """TopKCompression with error feedback, CPU."""

    def __init__(self, compress_ratio: float = 0.01):
        self.compress_ratio = float(compress_ratio)
        self.residuals = {}

    def compress(self, t: torch.Tensor, name: str):
        t = t.detach().cpu()
        if name in self.residuals:
            t = 1.0 * self.residuals[name] + 1.0 * t
        numel, shape = t.numel(), t.size()
        values, indices = topk_sparse(t, self.compress_ratio)
        dec = topk_desparse(values, indices, numel).view(shape)
        self.residuals[name] = t - dec
        return (values, indices), (numel, shape)

    @staticmethod
    def decompress(tensors, ctx):
        numel, shape = ctx
        values, indices = tensors
        return topk_desparse(values, indices, numel).view(shape)


def mag_keys(t: np.ndarray) -> np.ndarray:
    """The magnitude key of every fp32 element: its bits without the sign, as an unsigned integer
    (NaN above inf above every finite magnitude; +0 and -0 tie)."""
    t = np.ascontiguousarray(t, np.float32)
    return t.view(np.uint32) & np.uint32(0x7FFFFFFF)


def topk_select_index_order(t: np.ndarray, k: int) -> np.ndarray:
    """Indices (int64) of the k largest magnitude keys of the fp32 array t: descending key, ties by
    ascending index (a stable sort of the negated key)."""
    key = mag_keys(t).astype(np.int64)
    return np.argsort(-key, kind="stable")[:int(k)].astype(np.int64)


def topk_ef_step(x: np.ndarray, residual, mode: int, alpha: float, k: int, rule: str = "index"):
    """One omf_topk_encode call on one tensor, in fp32 numpy: returns ``(values, indices, residual)``.

    ``a = fl32(alpha * x)``; modes 0 and 2: ``t' = a``; mode 1: ``t' = fl32(residual + a)`` (two
    roundings, no FMA).  ``rule``: "index" (``topk_select_index_order``) or "torch"
    (``torch.topk(|t'|, k, sorted=False)`` on the CPU, as ``topk_sparse``).  The new residual is t'
    with ``fl32(t' - t')`` on the selected slots: +0 for a finite t', the NaN itself for a NaN and
    the quiet NaN 0xffc00000 for an infinite one (the sign of inf - inf's NaN is the platform's: gfx950
    and the reference's x86 hosts set it, include/omf_codec.h; spelled out here so that the oracle
    does not depend on its host).  Mode 0 returns None for it.  The inputs are not modified."""
    if mode not in (0, 1, 2):
        raise ValueError("mode must be 0, 1 or 2")
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(all="ignore"):
        tp = (np.float32(alpha) * x).astype(np.float32)
        if mode == 1:
            tp = (np.ascontiguousarray(residual, np.float32) + tp).astype(np.float32)
    if rule == "index":
        idx = topk_select_index_order(tp, k)
    elif rule == "torch":
        _, ti = torch.topk(torch.from_numpy(tp).abs(), int(k), sorted=False)
        idx = ti.numpy().astype(np.int64)
    else:
        raise ValueError(f"rule must be 'index' or 'torch', not {rule!r}")
    values = tp[idx]
    if mode == 0:
        return values, idx, None
    res = tp.copy()
    inf_nan = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    res[idx] = np.where(np.isfinite(values), np.float32(0.0), np.where(np.isnan(values), values, inf_nan))
    return values, idx, res
