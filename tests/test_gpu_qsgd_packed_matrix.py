"""The two kernels every packed QSGD message goes through, omf_qsgd_pack and omf_qsgd_decode_packed, and
the K-client sum omf_qsgd_decode_sum_packed, held to numpy cell by cell at every code width b = 2..32.

Recipes and oracles: tests/golden/qsgd_packed_inputs.py (tests/test_qsgd_packed_host.py checks them without
a GPU).  Per b the levels L_lo = 2^(b-2) and L_hi = min(2^(b-1) - 1, 2^31 - 2); six layouts, among them
arenas whose first tensor does not start at element 0 (one leading padding group; a whole leading 8 Ki
block), arenas of less than one group, and one without padding that ends on an 8 Ki block.

* The pack: payloads with -L, +L, 0 and +-1 at every tensor and group edge and a filler that is no level in
  the padding; the WHOLE packed arena is compared with the oracle's words — every stream byte, the code-0
  tail of each tensor's last group, and the canary word in every padding group.
* The decoders: packed arenas no encoder made (random words, runs of all-zero and all-one words, codes above
  2L, which decode by the same formula with code - L taken as int32), norms 0, -0.0, 1, 0.37, 1e-40, 3e38,
  inf and NaN; plain and accumulating; the padding of y keeps its bytes.

No tolerance anywhere: words are compared as bytes, floats bit for bit with NaN positions coinciding.
"""

import ctypes

import numpy as np
import pytest
import torch

import qsgd_matrix_inputs as M
import qsgd_packed_inputs as P
from omnifed_amd import _lib, codec

pytestmark = pytest.mark.gpu

NAMES = list(P.LAYOUTS)
WORD_I32 = int(P.CANARY_WORD.view(np.int32))
GUARD_I32 = 0x5EA1ED00


def same_floats(got, want):
    """Bit-equal where the reference is not NaN, NaN exactly where it is."""
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all())


def _first(got, want):
    nan = np.isnan(want)
    bad = np.flatnonzero((np.isnan(got) != nan) | (~nan & (got.view(np.uint32) != want.view(np.uint32))))
    return None if not bad.size else (int(bad.size), int(bad[0]), float(got[bad[0]]), float(want[bad[0]]))


def _first_word(got, want):
    bad = np.flatnonzero(got != want)
    return None if not bad.size else (int(bad.size), int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])))


def _cells(b, bad):
    """Every failing cell in the message (a string: pytest abbreviates the repr of anything else)."""
    return f"b = {b}: {len(bad)} cells fail: " + "; ".join(str(c) for c in bad)


class Arenas:
    """One plan per layout, made once."""

    def __init__(self, gpu):
        self.gpu = gpu
        self.plans = {}
        for name in NAMES:
            lay = P.layout(name)
            plan = codec.Plan(lay.sizes, offsets=lay.offsets, device=gpu)
            assert plan.arena_end == lay.end
            self.plans[name] = plan

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.gpu)

    def words(self, w):
        return self.dev(w.view(np.int32))

    def canaries(self, lay):
        return torch.full((lay.end,), float(P.CANARY), dtype=torch.float32, device=self.gpu)


@pytest.fixture(scope="module")
def arenas(gpu):
    return Arenas(gpu)


# ------------------------------------------------------------------ 1. the pack

@pytest.mark.parametrize("b", P.WIDTHS)
def test_pack_cells(arenas, b):
    bad = []  # every failing cell, not the first alone
    for L in P.levels_of(b):
        for name in NAMES:
            lay, plan = P.layout(name), arenas.plans[name]
            assert plan.packed_words(L) == lay.words(b)
            for width in P.storage_widths(L):
                q = P.pack_payload(width, L, lay)
                want = P.pack_ref(q, L, lay)
                out = torch.full((lay.words(b),), WORD_I32, dtype=torch.int32, device=arenas.gpu)
                plan.qsgd_pack(arenas.dev(q), width, L, packed_out=out)
                got = out.cpu().numpy().view(np.uint32)
                if got.tobytes() != want.tobytes():
                    bad.append((L, name, width, _first_word(got, want)))
                if name == "EXACT":  # 8-byte, not 16-byte aligned, a guard word on each side
                    nw = lay.words(b)
                    big = torch.full((nw + 4,), GUARD_I32, dtype=torch.int32, device=arenas.gpu)
                    view = big[2:2 + nw]
                    assert view.data_ptr() % 16 == 8
                    view.fill_(WORD_I32)
                    plan.qsgd_pack(arenas.dev(q), width, L, packed_out=view)
                    bh = big.cpu().numpy()
                    if not ((bh[:2] == GUARD_I32).all() and (bh[2 + nw:] == GUARD_I32).all()):
                        bad.append((L, name, width, "a guard word of the 8-byte aligned view"))
                    if bh[2:2 + nw].tobytes() != want.tobytes():
                        bad.append((L, name, width, "8-byte aligned view"))
    assert not bad, _cells(b, bad)


# ------------------------------------------------------------------ 2. the decode

@pytest.mark.parametrize("b", P.WIDTHS)
def test_decode_packed_cells(arenas, b):
    bad = []
    for L in P.levels_of(b):
        for i, name in enumerate(NAMES):
            lay, plan = P.layout(name), arenas.plans[name]
            words = P.message(b, lay)
            norms = P.norms_for(lay, b)
            plain, acc = P.decode_want(words, L, lay, norms)
            nd = arenas.dev(norms)
            sources = [("aligned", arenas.words(words))]
            if i == b % len(NAMES):  # 4-byte, not 8-byte aligned: a [1:] view of a tensor holding the same words
                holder = torch.empty(words.size + 1, dtype=torch.int32, device=arenas.gpu)
                holder[1:] = arenas.words(words)
                assert holder[1:].data_ptr() % 8 == 4
                sources.append(("4-byte aligned", holder[1:]))
            for tag, pd in sources:
                y = arenas.canaries(lay)
                plan.qsgd_decode_packed(pd, L, nd, y_out=y)
                got = y.cpu().numpy()
                if not same_floats(got, plain) or got[lay.pad].tobytes() != plain[lay.pad].tobytes():
                    bad.append((L, name, tag, "plain", _first(got, plain)))
                y = arenas.dev(lay.prev)
                plan.qsgd_decode_packed(pd, L, nd, y_out=y, accumulate=True)
                got = y.cpu().numpy()
                if not same_floats(got, acc) or got[lay.pad].tobytes() != acc[lay.pad].tobytes():
                    bad.append((L, name, tag, "accumulate", _first(got, acc)))
    assert not bad, _cells(b, bad)


# ------------------------------------------------------------------ 3. the K-client sum on the new layouts

SUM_KS = (1, 2, 9)  # nine chains two launches, three at b > 10


@pytest.mark.parametrize("b", [6, 10, 11, 32])
def test_decode_sum_packed_on_the_new_layouts(arenas, b):
    for L in P.levels_of(b):
        for name in ("LEAD32", "LEADBLK", "TINY_LEAD", "EXACT"):
            lay, plan = P.layout(name), arenas.plans[name]
            msgs = [P.message(b, lay, seed=k) for k in range(max(SUM_KS))]
            norms = [P.norms_for(lay, b, k) for k in range(max(SUM_KS))]
            terms = [P.decode_terms(w, L, lay, nm) for w, nm in zip(msgs, norms)]
            pds = [arenas.words(w) for w in msgs]
            nds = [arenas.dev(nm) for nm in norms]
            for K in SUM_KS:
                for divisor in (None, 3.0):
                    want = P.sum_ref(lay, terms[:K], divisor=divisor)
                    y = arenas.canaries(lay)  # init=False never reads it
                    plan.qsgd_decode_sum_packed(pds[:K], L, nds[:K], y_out=y, divisor=divisor)
                    got = y.cpu().numpy()
                    assert same_floats(got, want), (b, L, name, K, divisor, _first(got, want))
                    assert (got[lay.pad].view(np.uint32) == 0).all(), (b, L, name, K, divisor, "padding is not +0")
                want = P.sum_ref(lay, terms[:K], start=lay.prev, divisor=37.0)
                y = arenas.dev(lay.prev)
                plan.qsgd_decode_sum_packed(pds[:K], L, nds[:K], y_out=y, init=True, divisor=37.0)
                got = y.cpu().numpy()
                assert same_floats(got, want), (b, L, name, K, "init", _first(got, want))
                assert got[lay.pad].tobytes() == lay.prev[lay.pad].tobytes(), (b, L, name, K, "init: padding written")


# ------------------------------------------------------------------ 4. where the two kernels meet

@pytest.mark.parametrize("b", [2, 7, 11, 31, 32])
def test_pack_then_decode_equals_decode_ref(arenas, b):
    lay, plan = P.layout("MIX"), arenas.plans["MIX"]
    norms = P.norms_for(lay, b)
    nd = arenas.dev(norms)
    for L in P.levels_of(b):
        for width in P.storage_widths(L):
            q = P.pack_payload(width, L, lay)
            packed = torch.full((lay.words(b),), WORD_I32, dtype=torch.int32, device=arenas.gpu)
            plan.qsgd_pack(arenas.dev(q), width, L, packed_out=packed)
            y = arenas.canaries(lay)
            plan.qsgd_decode_packed(packed, L, nd, y_out=y)
            got = y.cpu().numpy()
            for t, (o, n) in enumerate(lay.ranges):
                want = M.decode_ref(q[o:o + n], norms[t], L)
                assert same_floats(got[o:o + n], want), (b, L, width, t, _first(got[o:o + n], want))
            assert (got[lay.pad] == P.CANARY).all(), (b, L, width)


# ------------------------------------------------------------------ 5. refusals

def test_packed_einval(arenas):
    """Through the C ABI (the binding would refuse most of these first): OMF_EINVAL, nothing written."""
    lay, plan = P.layout("LEAD32"), arenas.plans["LEAD32"]
    lib = _lib.lib()
    L, b = 16, 6
    st = ctypes.c_void_p(torch.cuda.current_stream(arenas.gpu).cuda_stream)
    q8 = arenas.dev(P.pack_payload(8, L, lay))
    q32 = arenas.dev(P.pack_payload(32, L, lay))
    extra = 8  # room for the shifted pointers
    out = torch.full((lay.words(32) + extra,), WORD_I32, dtype=torch.int32, device=arenas.gpu)
    y = torch.full((lay.end + extra,), float(P.CANARY), dtype=torch.float32, device=arenas.gpu)
    msg = arenas.words(P.message(32, lay))  # long enough for every width
    nd = arenas.dev(P.norms_for(lay, b))
    one_p, one_n = (ctypes.c_void_p * 1)(msg.data_ptr()), (ctypes.c_void_p * 1)(nd.data_ptr())
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    pack, dec = lib.omf_qsgd_pack, lib.omf_qsgd_decode_packed
    assert pack(plan.handle, p(q8), 8, L, p(out), st) == _lib.OMF_OK  # the calls below differ from this in one thing
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[:lay.words(b)] != WORD_I32).any()
    out.fill_(WORD_I32)
    bad = [
        pack(plan.handle, p(q8), 8, 0, p(out), st),                       # levels 0
        pack(plan.handle, p(q32), 32, (1 << 31) - 1, p(out), st),         # levels 2^31 - 1
        pack(plan.handle, p(q8), 8, 128, p(out), st),                     # an int8 payload with levels 128
        pack(plan.handle, p(q8), 16, L, p(out), st),                      # width 16
        pack(plan.handle, p(q8), 8, L, p(out, 4), st),                    # packed_out 4-byte aligned only
        pack(plan.handle, p(q8, 4), 8, L, p(out), st),                    # q not 16-byte aligned
        pack(plan.handle, p(q32, 8), 32, L, p(out), st),
        dec(plan.handle, p(msg), 0, p(nd), p(y), 0, st),                  # levels 0
        dec(plan.handle, p(msg), (1 << 31) - 1, p(nd), p(y), 0, st),      # levels 2^31 - 1
        dec(plan.handle, p(msg), L, p(nd), p(y, 4), 0, st),               # y not 16-byte aligned
        dec(plan.handle, p(msg), L, p(nd), p(y, 8), 1, st),
        dec(plan.handle, p(msg, 2), L, p(nd), p(y), 0, st),               # packed not 4-byte aligned
        lib.omf_qsgd_decode_sum_packed(plan.handle, one_p, one_n, 1, (1 << 31) - 1, p(y), 0, 0.0, st),
    ]
    assert bad == [_lib.OMF_EINVAL] * len(bad), f"return codes, in the order above: {bad}"
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == WORD_I32).all()
    assert (y.cpu().numpy() == P.CANARY).all()
    with pytest.raises(ValueError):
        plan.qsgd_pack(q8, 8, 128)
    with pytest.raises(ValueError):
        plan.qsgd_decode_packed(msg, (1 << 31) - 1, nd)
