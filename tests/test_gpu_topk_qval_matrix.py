"""The three kernels of the opt-in quantised Top-K value wire — omf_topk_value_scales, omf_topk_quantize_values,
omf_topk_dequantize_values — held to the numpy oracle of tests/golden/topk_qval_inputs.py byte for byte, at every
s = 1..8.

One plan of 13 small tensors: k_t in {0, 1, 31, 32, 33, 4 097, 8 191, 8 193} (a partial group, a workgroup's run
of 256 groups = 8 192 values crossed inside a tensor, the Philox layout's 1 024- and 4 096-element periods),
values over many binades with +-0 and subnormals among them, then a tensor of zeros alone, one holding an
infinity, one a NaN, one whose maximum is above FLT_MAX / L, one of subnormals alone; one tensor's indices hold
n, -1 and 2^40.

* scales: every tensor's bits, the NaN and the infinity visible, 0 for the tensor without a value;
* quantise: the whole value arena against the oracle's words over a canary — the words of the three unusable
  tensors and the words past the arena keep the canary — and the whole residual arena, where only the slots the
  oracle stores to differ from the canary; the same codes with residual = NULL;
* dequantise: the sender's own words; then messages no encoder made — every code 0..2 L, a negative-scale tensor
  among live ones whose values stay as they were, every bit past a tensor's k b set — with a canary around the
  values;
* the all-zero count vector and the OMF_EINVAL cases.
"""

import ctypes

import numpy as np
import pytest
import torch

import topk_qval_inputs as Q
from omnifed_amd import _lib, codec

pytestmark = pytest.mark.gpu

SIZES, COUNTS = Q.MATRIX_SIZES, Q.MATRIX_COUNTS
NT, K = len(SIZES), sum(COUNTS)
KOFF = np.concatenate([[0], np.cumsum(COUNTS)]).tolist()
SEED, OFFSET = 0x1234_5678_9ABC_DEF0, 0x1_0000_0007  # the key's two words, a call counter above 32 bits
WORD_I32 = int(np.uint32(Q.CANARY_WORD).view(np.int32))


@pytest.fixture(scope="module")
def env(gpu):
    plan = codec.Plan(SIZES, device=gpu)
    vals, idx = Q.matrix_values(), Q.matrix_indices()
    dv = torch.from_numpy(np.concatenate(vals)).to(gpu)
    di = torch.from_numpy(np.concatenate(idx)).to(gpu)
    scales = plan.topk_value_scales(COUNTS, dv)
    return dict(plan=plan, vals=vals, idx=idx, dv=dv, di=di, scales=scales)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return None if not bad.size else (int(bad.size), int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])))


def test_recipe_covers_what_it_claims():
    assert set(COUNTS) >= {0, 1, 31, 32, 33, 4097, 8191, 8193}
    goff = Q.group_offsets(COUNTS)
    assert goff[-1] > 2 * 256  # more than two workgroups
    t = max(t for t in range(NT) if goff[t] <= 256)  # the first workgroup ends inside this tensor
    assert goff[t] < 256 < goff[t + 1]
    vals = Q.matrix_values()
    assert [bool(Q.usable(Q.scale_of(v), 1)) for v in vals] == [t not in Q.UNUSABLE for t in range(NT)]
    assert [codec.topk_scale_usable(float(Q.scale_of(v)), 8) for v in vals] == [t not in Q.UNUSABLE for t in range(NT)]
    assert Q.scale_of(vals[Q.T_ZEROS]) == 0 and np.signbit(vals[Q.T_ZEROS]).any()
    assert 0 < Q.scale_of(vals[Q.T_SUB]) < np.finfo(np.float32).tiny
    big = vals[5]
    assert (big == 0).any() and np.signbit(big[big == 0]).any() and ((big != 0) & (np.abs(big) < 1e-38)).any()
    idx = Q.matrix_indices()
    assert all(np.unique(i).size == i.size for i in idx)
    assert ((idx[Q.T_BADIDX] < 0) | (idx[Q.T_BADIDX] >= SIZES[Q.T_BADIDX])).sum() == 3


def test_scales(env):
    want = np.array([Q.scale_of(v) for v in env["vals"]], np.float32)
    got = u32(env["scales"])
    assert first_bad(got, want.view(np.uint32)) is None
    assert np.isnan(want[Q.T_NAN]) and np.isinf(want[Q.T_INF]) and want[0] == 0
    # into a buffer that held something else, from a stream of its own: the call clears before it takes maxima
    out = torch.full((NT + 2,), 7.0, device=env["dv"].device)
    env["plan"].topk_value_scales(COUNTS, env["dv"], scales_out=out)
    oh = u32(out)
    assert first_bad(oh[:NT], want.view(np.uint32)) is None and (out[NT:].cpu() == 7.0).all()


@pytest.mark.parametrize("s", range(1, 9))
def test_quantize_cells(gpu, env, s):
    plan, vals, idx = env["plan"], env["vals"], env["idx"]
    b = Q.code_bits(s)
    words = Q.group_offsets(COUNTS)[-1] * b
    assert plan.topk_value_words(COUNTS, s) == words
    assert plan.topk_value_layout(COUNTS, s) == (b, [g * b for g in Q.group_offsets(COUNTS)[:-1]], words)
    qs, es, codes = [], [], []
    for t, v in enumerate(vals):
        m, q, _d, e = Q.quantize(v, s, SEED, OFFSET, t)
        assert (q is None) == (t in Q.UNUSABLE)
        qs.append(q)
        codes.append(None if q is None else q + 2**s)
        es.append(None if (q is None or m == 0) else e)
    assert es[Q.T_ZEROS] is None and es[0] is None  # scale 0: nothing stored
    canary = np.full(words + 4, Q.CANARY_WORD, np.uint32)
    want = Q.value_arena(COUNTS, codes, s, base=canary)
    assert (want[words:] == Q.CANARY_WORD).all() and (want[:words] == Q.CANARY_WORD).sum() >= 3 * 2 * b
    res0 = np.full(plan.arena_end, Q.CANARY_FLOAT, np.float32)
    want_res = Q.residual_after(res0, plan.offsets, SIZES, idx, es)
    # ---- with the residual
    out = torch.full((words + 4,), WORD_I32, dtype=torch.int32, device=gpu)
    res = torch.from_numpy(res0.copy()).to(gpu)
    got = plan.topk_quantize_values(COUNTS, env["dv"], env["di"], env["scales"], s, SEED, OFFSET, residual=res,
                                    packed_out=out)
    assert got.data_ptr() == out.data_ptr()
    assert first_bad(u32(out), want) is None
    assert first_bad(u32(res), want_res.view(np.uint32)) is None
    touched = np.flatnonzero(want_res.view(np.uint32) != res0.view(np.uint32)).size
    assert touched <= sum(COUNTS[t] for t in range(NT) if es[t] is not None) - 3
    # ---- residual = NULL (and no indices): the same codes
    out2 = torch.full((words + 4,), WORD_I32, dtype=torch.int32, device=gpu)
    plan.topk_quantize_values(COUNTS, env["dv"], None, env["scales"], s, SEED, OFFSET, packed_out=out2)
    assert first_bad(u32(out2), want) is None
    # ---- another call counter, another tensor stream: other codes (the draws are used)
    if s >= 2:
        out3 = torch.full((words + 4,), WORD_I32, dtype=torch.int32, device=gpu)
        plan.topk_quantize_values(COUNTS, env["dv"], None, env["scales"], s, SEED, OFFSET + 1, packed_out=out3)
        assert (u32(out3) != want).any()
    # ---- the sender's own words back: d for the quantised tensors, the canary elsewhere
    back = torch.full((K + 3,), float(Q.CANARY_FLOAT), device=gpu)
    sc = env["scales"].clone()
    sc[list(Q.UNUSABLE)] = -1.0
    plan.topk_dequantize_values(COUNTS, out[:max(words, 1)], sc, s, values_out=back)
    want_back = np.full(K + 3, Q.CANARY_FLOAT, np.float32)
    for t, q in enumerate(qs):
        if q is not None:
            want_back[KOFF[t]:KOFF[t + 1]] = Q.dequantize(q, Q.scale_of(vals[t]), s)
    assert first_bad(u32(back), want_back.view(np.uint32)) is None


@pytest.mark.parametrize("s", range(1, 9))
def test_dequantize_foreign_messages(gpu, env, s):
    """Codes no encoder chose: every code 0..2 L in turn (and, below a power of two, the codes above 2 L a b-bit
    field can hold: decoded by the same linear rule), scales of the receiver's choosing — a negative one marks a
    tensor to leave alone — and every bit past a tensor's k b set."""
    plan = env["plan"]
    L, b = 2**s, Q.code_bits(s)
    rng = np.random.default_rng(80 + s)
    scales = np.array([0.0, 1.5, -1.0, 3.0, 1e-40, -2.5, Q.FLT_MAX / L, 0.1, 0.0, 0.25, 7.0, -1.0, 2.0**-126], np.float32)
    skip = [t for t in range(NT) if scales[t] < 0]
    assert skip == [2, 5, 11]
    codes = []
    for t, k in enumerate(COUNTS):
        c = (np.arange(k, dtype=np.int64) + t) % (2 * L + 1)
        if t == 7:
            c = rng.integers(0, 2**b, k)
        codes.append(c.astype(np.uint64))
    words = Q.value_arena(COUNTS, codes, s, pad_ones=True)
    assert (words != Q.value_arena(COUNTS, codes, s)).any()
    have = rng.standard_normal(K + 5).astype(np.float32)
    want = have.copy()
    for t in range(NT):
        if t not in skip:
            want[2 + KOFF[t]:2 + KOFF[t + 1]] = Q.dequantize(codes[t].astype(np.int64) - L, scales[t], s)
    buf = torch.from_numpy(have.copy()).to(gpu)
    view = buf[2:]
    plan.topk_dequantize_values(COUNTS, torch.from_numpy(words.view(np.int32)).to(gpu), torch.from_numpy(scales).to(gpu),
                                s, values_out=view)
    assert first_bad(u32(buf), want.view(np.uint32)) is None


def test_scale_at_the_overflow_edge(gpu):
    """m = FLT_MAX / L is the largest usable scale, the next float above it is not."""
    for s in (1, 4, 8):
        edge = np.float32(Q.FLT_MAX / 2**s)
        over = np.nextafter(edge, np.float32(np.inf))
        plan = codec.Plan([8, 8], device=gpu)
        vals = [np.array([edge, -edge / 3, 0.0], np.float32), np.array([over, 1.0, -2.0], np.float32)]
        counts = [3, 3]
        dv = torch.from_numpy(np.concatenate(vals)).to(gpu)
        sc = plan.topk_value_scales(counts, dv)
        assert u32(sc).tolist() == [int(edge.view(np.uint32)), int(over.view(np.uint32))]
        assert codec.topk_scale_usable(float(edge), s) and not codec.topk_scale_usable(float(over), s)
        assert Q.usable(edge, s) and not Q.usable(over, s)
        b = Q.code_bits(s)
        out = torch.full((2 * b,), WORD_I32, dtype=torch.int32, device=gpu)
        plan.topk_quantize_values(counts, dv, None, sc, s, 1, 2, packed_out=out)
        _m, q, _d, _e = Q.quantize(vals[0], s, 1, 2, 0)
        want = Q.value_arena(counts, [q + 2**s, None], s, base=np.full(2 * b, Q.CANARY_WORD, np.uint32))
        assert first_bad(u32(out), want) is None


def test_all_zero_counts_touch_nothing(gpu, env):
    plan = env["plan"]
    counts = [0] * NT
    assert plan.topk_value_words(counts, 4) == 0
    words = torch.full((8,), WORD_I32, dtype=torch.int32, device=gpu)
    vals = torch.full((8,), 5.0, device=gpu)
    sc = torch.full((NT,), 9.0, device=gpu)
    plan.topk_quantize_values(counts, vals, None, sc, 4, 1, 2, packed_out=words)
    plan.topk_dequantize_values(counts, words, sc, 4, values_out=vals)
    assert (words.cpu().numpy() == WORD_I32).all() and (vals.cpu() == 5.0).all()
    plan.topk_value_scales(counts, vals, scales_out=sc)
    assert (sc.cpu() == 0.0).all()  # a tensor without a value has scale 0
    arr = (ctypes.c_int64 * NT)(*counts)
    L = _lib.lib()
    assert L.omf_topk_quantize_values(plan.handle, arr, None, None, None, 4, 0, 0, None, None, None) == _lib.OMF_OK
    assert L.omf_topk_dequantize_values(plan.handle, arr, None, None, 4, None, None) == _lib.OMF_OK


def test_einval_cases(gpu, env):
    plan = env["plan"]
    L = _lib.lib()
    E = _lib.OMF_EINVAL
    s = 4
    words = plan.topk_value_words(COUNTS, s)
    arr = (ctypes.c_int64 * NT)(*COUNTS)
    vals = torch.zeros(K + 2, device=gpu)
    idx = torch.zeros(K + 2, dtype=torch.int64, device=gpu)
    pk = torch.zeros(words + 2, dtype=torch.int32, device=gpu)
    sc = torch.ones(NT + 2, device=gpu)
    res = torch.zeros(plan.arena_end + 2, device=gpu)
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    vp, ip, pp, sp, rp = (t.data_ptr() for t in (vals, idx, pk, sc, res))

    def P(x):
        return None if x is None else ctypes.c_void_p(x)

    def quant(a=arr, v=vp, i=ip, sc_=sp, bw=s, r=rp, p=pp, h=plan.handle):
        return L.omf_topk_quantize_values(h, a, P(v), P(i), P(sc_), bw, 1, 2, P(r), P(p), st)

    def deq(a=arr, p=pp, sc_=sp, bw=s, v=vp, h=plan.handle):
        return L.omf_topk_dequantize_values(h, a, P(p), P(sc_), bw, P(v), st)

    def scl(a=arr, v=vp, sc_=sp, h=plan.handle):
        return L.omf_topk_value_scales(h, a, P(v), P(sc_), st)

    assert (quant(), deq(), scl()) == (0, 0, 0)
    assert quant(i=None, r=None) == 0 and quant(r=None) == 0   # no residual: indices optional
    assert (quant(h=None), deq(h=None), scl(h=None)) == (E, E, E)
    assert (quant(a=None), deq(a=None), scl(a=None)) == (E, E, E)
    for bw in (0, 9, -1):
        assert (quant(bw=bw), deq(bw=bw)) == (E, E)
        assert L.omf_topk_value_words(plan.handle, arr, bw) == -1
    assert quant(v=None) == E and quant(sc_=None) == E and quant(p=None) == E and quant(i=None) == E
    assert deq(p=None) == E and deq(sc_=None) == E and deq(v=None) == E
    assert scl(v=None) == E and scl(sc_=None) == E
    assert quant(v=vp + 2) == E and quant(p=pp + 2) == E and quant(sc_=sp + 2) == E and quant(r=rp + 2) == E
    assert quant(i=ip + 4) == E
    assert deq(p=pp + 2) == E and deq(v=vp + 2) == E and deq(sc_=sp + 2) == E
    assert scl(v=vp + 2) == E and scl(sc_=sp + 2) == E
    assert quant(v=vp + 4, i=ip + 8, p=pp + 4, sc_=sp + 4, r=rp + 4) == 0  # 4 and 8 bytes are enough
    assert quant(p=vp + 4 * K - 4) == E          # the codes start inside the values
    assert quant(p=ip + 8 * K - 4) == E          # ... inside the indices
    assert quant(p=rp) == E and quant(p=sp) == E
    assert quant(r=vp) == E                      # the residual over the values
    assert deq(v=pp) == E and deq(v=sp) == E
    assert scl(sc_=vp) == E
    for t, k in ((0, -1), (3, SIZES[3] + 1)):
        bad = list(COUNTS)
        bad[t] = k
        a = (ctypes.c_int64 * NT)(*bad)
        assert (quant(a=a), deq(a=a), scl(a=a)) == (E, E, E)
        assert L.omf_topk_value_words(plan.handle, a, s) == -1
    assert L.omf_topk_value_words(None, arr, s) == -1 and L.omf_topk_value_words(plan.handle, None, s) == -1
    assert L.omf_topk_value_words(plan.handle, arr, s) == words
    # the Python face checks its arguments before the call
    with pytest.raises(ValueError):
        plan.topk_quantize_values(COUNTS, vals[:K - 1], idx, sc, s, 1, 2)
    with pytest.raises(ValueError):
        plan.topk_quantize_values(COUNTS, vals, idx.to(torch.int32), sc, s, 1, 2, residual=res)
    with pytest.raises(ValueError):
        plan.topk_quantize_values(COUNTS, vals, None, sc, s, 1, 2, residual=res)
    with pytest.raises(ValueError):
        plan.topk_quantize_values(COUNTS, vals, idx, sc, 9, 1, 2)
    with pytest.raises(ValueError):
        plan.topk_dequantize_values(COUNTS, pk[:words - 1], sc, s)
    with pytest.raises(ValueError):
        plan.topk_value_scales(COUNTS, vals, scales_out=sc[:NT - 1])
    with pytest.raises(ValueError):
        plan.topk_value_words(COUNTS, 0)
    torch.cuda.synchronize(gpu)
