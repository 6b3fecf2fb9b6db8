"""The recipes and numpy oracles of the packed QSGD matrix (tests/golden/qsgd_packed_inputs.py) have the
properties tests/test_gpu_qsgd_packed_matrix.py relies on.  No GPU."""

import numpy as np
import pytest

import qsgd_matrix_inputs as M
import qsgd_packed_inputs as P
from oracle import bitpack
from omnifed_amd import codec

I32 = np.iinfo(np.int32)


def test_levels_give_every_width():
    assert P.WIDTHS == tuple(range(2, 33)) and len(P.ALL_LEVELS) == 61
    assert P.levels_of(2) == (1,) and P.levels_of(3) == (2, 3) and P.levels_of(32) == (1 << 30, (1 << 31) - 2)
    for b, L in P.ALL_LEVELS:
        assert bitpack.packed_bits(L) == b == codec.packed_bits(L), (b, L)
        assert 1 <= L <= I32.max - 1
    for b in P.WIDTHS:
        lo, hi = P.levels_of(b)[0], P.levels_of(b)[-1]
        assert lo & (lo - 1) == 0, "L_lo is a power of two"
        if b >= 4:
            assert hi & (hi - 1), "L_hi takes the division path"
        if b < 32:
            assert 2 * hi + 1 == (1 << b) - 1, "every b-bit code but one is a level"
    assert [w for L in (1, 127, 128) for w in P.storage_widths(L)] == [8, 32, 8, 32, 32]


def test_layouts_have_the_cases():
    import ast
    import os

    src = open(os.path.join(os.path.dirname(__file__), "test_gpu_decode_sum_packed.py")).read()
    consts = {n.targets[0].id: ast.literal_eval(n.value) for n in ast.parse(src).body
              if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") in ("SIZES", "OFFSETS")}
    assert consts == {"SIZES": P.MIX_SIZES, "OFFSETS": P.MIX_OFFSETS}
    for name in P.LAYOUTS:
        lay = P.layout(name)
        assert all(o % 32 == 0 for o in lay.offsets) and all(n > 0 for n in lay.sizes)
        assert all(o + n <= o2 for (o, n), o2 in zip(lay.ranges, lay.offsets[1:]))
        assert lay.end == lay.offsets[-1] + lay.sizes[-1] and lay.groups == -(-lay.end // 32)
    mix, lead, blk = P.layout("MIX"), P.layout("LEAD32"), P.layout("LEADBLK")
    tiny, tlead, exact = P.layout("TINY"), P.layout("TINY_LEAD"), P.layout("EXACT")
    assert mix.offsets[0] == 0 and mix.end == 77673
    assert lead.offsets[0] == 32, "exactly one leading padding group"
    assert lead.pad[:32].all() and not lead.pad[32] and lead.end > P.BLOCK // 2
    assert blk.offsets[0] > P.BLOCK and blk.offsets[0] % P.BLOCK, "block 0 is padding, and the gap goes on"
    assert blk.pad[:blk.offsets[0]].all() and blk.end > 2 * P.BLOCK
    assert tiny.end < 32 and tiny.groups == 1
    assert tlead.offsets[0] == 64 and tlead.groups == 3 and tlead.end % 32
    assert not exact.pad.any() and exact.end == 2 * P.BLOCK
    assert exact.offsets[1] == P.BLOCK, "a tensor boundary on the block boundary"


def _pack_by_words(q, L, lay, canary):
    """The pack on words: a group's 32 codes into one Python int, split into b 32-bit words."""
    b = (2 * L).bit_length()
    out = [int(canary)] * lay.words(b)
    for o, n in lay.ranges:
        for g in range(0, n, 32):
            big = 0
            for i in range(32):
                code = int(q[o + g + i]) + L if g + i < n else 0
                assert 0 <= code <= 2 * L
                big |= code << (i * b)
            w0 = (o + g) // 32 * b
            out[w0:w0 + b] = [(big >> (32 * j)) & 0xFFFFFFFF for j in range(b)]
    return np.array(out, np.uint64).astype(np.uint32)


SMALL = ("LEAD32", "TINY", "TINY_LEAD")
WORD_CHECK = [(b, L, name) for b, L in P.ALL_LEVELS for name in P.LAYOUTS
              if name in SMALL or (b in (2, 7, 11, 31, 32) and L == P.levels_of(b)[-1])]


def test_pack_oracle_equals_the_statement_on_words():
    for b, L, name in WORD_CHECK:
        lay = P.layout(name)
        for width in P.storage_widths(L):
            q = P.pack_payload(width, L, lay)
            got = P.pack_ref(q, L, lay)
            want = _pack_by_words(q, L, lay, P.CANARY_WORD)
            assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), (b, L, name, width)
            assert (got[~lay.written_words(b)] == P.CANARY_WORD).all()


@pytest.mark.parametrize("name", list(P.LAYOUTS))
def test_payloads_fill_edges_and_decode_back(name):
    """The filler is outside every tensor and nowhere else, the forced values are where the recipe says,
    every one of them at a first and at a last element over the matrix, and the decode oracle turns the
    pack oracle's words back into decode_ref of the levels (so the two oracles agree on the layout)."""
    lay = P.layout(name)
    edges = lay.edge_positions()
    assert all(not lay.pad[p] for p in edges)
    for o, n in lay.ranges:
        assert o in edges and o + n - 1 in edges
        for g in range(o + 32, o + n, 32):
            assert g - 1 in edges and g in edges
    seen_first, seen_last = set(), set()
    for b, L in P.ALL_LEVELS:
        for width in P.storage_widths(L):
            q = P.pack_payload(width, L, lay)
            assert q.dtype == (np.int8 if width == 8 else np.int32) and q.size == lay.payload_elems(width)
            inside = np.zeros(q.size, bool)
            inside[:lay.end] = ~lay.pad
            assert (q[~inside] == P.FILL[width]).all() and (np.abs(q[inside].astype(np.int64)) <= L).all()
            for j, p in enumerate(edges):
                kind = P.edge_kind(j, b, width)
                assert int(q[p]) == P.edge_value(kind, L), (b, L, width, p)
                if p == lay.offsets[0]:
                    seen_first.add(kind)
                if p == lay.end - 1:
                    seen_last.add(kind)
        q = P.pack_payload(32, L, lay)
        words = P.pack_ref(q, L, lay)
        norms = P.norms_for(lay, b)
        term = P.decode_terms(words, L, lay, norms)
        for t, (o, n) in enumerate(lay.ranges):
            codes = P.codes_ref(words, lay, t, b)
            assert (codes.astype(np.int64) - L == q[o:o + n]).all(), (b, L, t)
            assert _same(term[o:o + n], M.decode_ref(q[o:o + n], norms[t], L)), (b, L, t)
            # the code-0 tail of the last group
            w0, nw = lay.tensor_words(t, b)
            tail = np.unpackbits(words[w0:w0 + nw].view(np.uint8), bitorder="little")[n * b:]
            assert not tail.any()
    assert seen_first == set(P.EDGE) and seen_last == set(P.EDGE)


def _same(got, want):
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all())


def test_every_norm_meets_every_tensor_position():
    for name in P.LAYOUTS:
        lay = P.layout(name)
        met = [set() for _ in range(lay.nt)]
        for b in P.WIDTHS:
            for t, v in enumerate(P.norms_for(lay, b)):
                met[t].add(np.float32(v).tobytes())
        assert all(len(m) == len(M.DEC_NORMS) for m in met), name


def test_messages_hold_runs_and_codes_above_2L():
    for b in P.WIDTHS:
        for name in P.LAYOUTS:
            lay = P.layout(name)
            w = [P.message(b, lay, seed) for seed in range(2)]
            assert w[0].dtype == np.uint32 and w[0].size == lay.words(b)
            assert w[0].tobytes() != w[1].tobytes()
            for t in range(lay.nt):
                w0, nw = lay.tensor_words(t, b)
                for m in w:
                    part = m[w0:w0 + nw]
                    assert (part == 0).any() and (part == 0xFFFFFFFF).any(), (b, name, t)
                assert w[0][w0] != w[1][w0], "the ends alternate with the seed"
        if b >= 3:
            L = P.levels_of(b)[0]
            for name in ("MIX", "LEAD32", "LEADBLK", "EXACT"):
                lay = P.layout(name)
                codes = np.concatenate([P.codes_ref(P.message(b, lay), lay, t, b) for t in range(lay.nt)])
                above = float((codes > 2 * L).mean())
                assert 0.3 < above < 0.7, (b, name, above)  # L_lo: half of the b-bit codes, less one
            for name in ("TINY", "TINY_LEAD"):  # the all-one run gives the few elements one
                lay = P.layout(name)
                assert any((P.codes_ref(P.message(b, lay, s), lay, 0, b) > 2 * L).any() for s in range(2)), (b, name)


def test_codes_and_int32_wrap_against_python_ints():
    """codes_ref against shifts of one Python int per tensor, and levels_ref against Python's integers
    brought into int32 by hand, at b = 32 (where the wrap happens) and at two narrower widths."""
    for b in (32, 31, 11):
        lay = P.layout("LEAD32")
        words = P.message(b, lay)
        for L in P.levels_of(b):
            wrapped = 0
            for t, (o, n) in enumerate(lay.ranges):
                w0, nw = lay.tensor_words(t, b)
                big = sum(int(v) << (32 * j) for j, v in enumerate(words[w0:w0 + nw]))
                codes = [(big >> (i * b)) & ((1 << b) - 1) for i in range(n)]
                assert codes == [int(c) for c in P.codes_ref(words, lay, t, b)]
                want = []
                for c in codes:
                    v = c - L
                    if v > I32.max:
                        v -= 1 << 32
                        wrapped += 1
                    assert I32.min <= v <= I32.max
                    want.append(v)
                got = P.levels_ref(np.array(codes, np.uint64), L)
                assert got.dtype == np.int32 and got.tolist() == want
            assert (wrapped > 0) == (b == 32), (b, L, wrapped)


def test_sum_ref_orders_and_divides():
    lay = P.layout("TINY_LEAD")
    terms = [np.full(lay.end, v, np.float32) for v in (1e8, 1.0, -1e8)]
    assert P.sum_ref(lay, terms)[lay.offsets[0]] == 0.0 and P.sum_ref(lay, terms[::-1])[lay.offsets[0]] == 0.0
    assert P.sum_ref(lay, [terms[0], terms[2], terms[1]])[lay.offsets[0]] == 1.0
    got = P.sum_ref(lay, terms[1:2], divisor=3.0)
    assert got[lay.offsets[0]] == np.float32(1.0) / np.float32(3.0) and (got[lay.pad].view(np.uint32) == 0).all()
    got = P.sum_ref(lay, terms[1:2], start=lay.prev, divisor=37.0)
    assert (got[lay.pad] == P.CANARY).all()
