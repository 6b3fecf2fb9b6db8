"""The two kernels of the opt-in bit-packed Top-K index wire, omf_topk_pack_indices and omf_topk_unpack_indices,
held to the numpy oracle of tests/golden/topk_packed_inputs.py word for word and index for index.

One plan: the 18 tensor sizes at the edges of the width rule (1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 257, 65 535,
65 536, 65 537, 2^20, 2^20 + 1, 2^25, 2^25 + 1) and 13 more, one for each width below 26 those leave out, so every
b = 1..26 runs on the device (widths 27..32 are held by the host check of the same group routines,
tests/test_topk_packed_host.py); no arena is allocated, only indices move.  Count vectors
from {0, 1, 31, 32, 33, min(n, 1000), n for n <= 257}: whole and partial last groups, tensors without a value at
the start, inside and at the end, more than one workgroup.  A second plan of 4 100 small tensors takes the
kernels' tensor search past the LDS table (17 workgroups, a partial group in nearly every tensor).

* pack: the whole packed arena equals the oracle's words (the 0 codes after a tensor's last index included) and
  a canary word past the arena is intact;
* unpack: from the oracle's words with every bit past a tensor's k b set, the indices are exact and a canary
  past K is intact — also into a buffer that is 8-byte but not 16-byte aligned;
* the all-zero count vector touches neither buffer; the OMF_EINVAL cases.
"""

import ctypes

import numpy as np
import pytest
import torch

import topk_packed_inputs as P
from omnifed_amd import _lib, codec

pytestmark = pytest.mark.gpu

WORD_I32 = int(np.uint32(P.CANARY_WORD).view(np.int32))
IDX_CANARY = int(P.CANARY_INDEX)
VECTORS = P.count_vectors()
MANY_SIZES = [[1, 2, 3, 5, 31, 33, 64, 65, 257, 1000][t % 10] for t in range(4100)]


@pytest.fixture(scope="module")
def plans(gpu):
    return {"matrix": codec.Plan(P.MATRIX_SIZES, device=gpu), "many": codec.Plan(MANY_SIZES, device=gpu)}


def many_counts():
    rng = np.random.default_rng(41)
    return [int(rng.choice(P.count_choices(n))) if t % 7 else 0 for t, n in enumerate(MANY_SIZES)]


def cases():
    out = [("matrix", v, c) for v, c in enumerate(VECTORS)]
    out.append(("many", 0, many_counts()))
    return out


def test_recipes_cover_what_they_claim():
    assert P.MATRIX_SIZES[:18] == [1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 257, 65535, 65536, 65537, 2**20, 2**20 + 1,
                                   2**25, 2**25 + 1]
    assert sorted({P.index_bits(n) for n in P.MATRIX_SIZES}) == list(range(1, 27))
    for t, n in enumerate(P.MATRIX_SIZES):
        assert {v[t] for v in VECTORS} >= set(P.count_choices(n)), n
    assert any(P.arena_layout(P.MATRIX_SIZES, v).goff[-1] > 256 for v in VECTORS)  # more than one workgroup
    assert len(MANY_SIZES) > 4096 and P.arena_layout(MANY_SIZES, many_counts()).goff[-1] > 16 * 256


@pytest.mark.parametrize("name, v, counts", cases(), ids=[f"{n}{v}" for n, v, _ in cases()])
def test_pack_and_unpack_cells(gpu, plans, name, v, counts):
    plan = plans[name]
    sizes = plan.sizes
    lay = P.arena_layout(sizes, counts)
    K = lay.koff[-1]
    assert plan.topk_packed_words(counts) == lay.words
    assert plan.topk_packed_layout(counts) == (lay.bits, lay.woff[:-1], lay.words)
    idx = P.draw_indices(sizes, counts, seed=500 + v)
    want = P.pack_arena(sizes, counts, idx)
    # ---- pack: the whole arena, then a canary word
    out = torch.full((lay.words + 4,), WORD_I32, dtype=torch.int32, device=gpu)
    got = plan.topk_pack_indices(counts, torch.from_numpy(idx).to(gpu), packed_out=out)
    assert got.data_ptr() == out.data_ptr()
    oh = out.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(oh[:lay.words] != want)
    assert not bad.size, (int(bad.size), int(bad[0]), hex(int(oh[bad[0]])), hex(int(want[bad[0]])))
    assert (oh[lay.words:] == P.CANARY_WORD).all()
    # ---- unpack: every bit past a tensor's k b set; a canary past K; 16-byte and 8-byte aligned outputs
    dirty = P.pack_arena(sizes, counts, idx, pad_ones=True)
    assert K == 0 or (dirty != want).any()
    dd = torch.from_numpy(dirty.view(np.int32)).to(gpu)
    for shift in (0, 1):
        big = torch.full((K + 5,), IDX_CANARY, dtype=torch.int64, device=gpu)
        view = big[2 + shift:]
        assert view.data_ptr() % 16 == 8 * shift
        plan.topk_unpack_indices(counts, dd, indices_out=view)
        bh = big.cpu().numpy()
        got_idx = bh[2 + shift:2 + shift + K]
        bad = np.flatnonzero(got_idx != idx)
        assert not bad.size, (shift, int(bad.size), int(bad[0]), int(got_idx[bad[0]]), int(idx[bad[0]]))
        assert (bh[:2 + shift] == IDX_CANARY).all() and (bh[2 + shift + K:] == IDX_CANARY).all(), shift
    # the device round trip of the sender's own words
    back = plan.topk_unpack_indices(counts, out[:max(lay.words, 1)])
    assert (back[:K].cpu().numpy() == idx).all()


def test_all_zero_counts_touch_nothing(gpu, plans):
    plan = plans["matrix"]
    counts = [0] * plan.nt
    assert plan.topk_packed_words(counts) == 0
    words = torch.full((8,), WORD_I32, dtype=torch.int32, device=gpu)
    idx = torch.full((8,), IDX_CANARY, dtype=torch.int64, device=gpu)
    plan.topk_pack_indices(counts, idx, packed_out=words)
    plan.topk_unpack_indices(counts, words, indices_out=idx)
    assert (words.cpu().numpy() == WORD_I32).all() and (idx.cpu().numpy() == IDX_CANARY).all()
    arr = (ctypes.c_int64 * plan.nt)(*counts)
    L = _lib.lib()
    assert L.omf_topk_pack_indices(plan.handle, arr, None, None, None) == _lib.OMF_OK  # nothing to launch
    assert L.omf_topk_unpack_indices(plan.handle, arr, None, None, None) == _lib.OMF_OK


def test_einval_cases(gpu, plans):
    plan = plans["matrix"]
    L = _lib.lib()
    counts = VECTORS[0]
    lay = P.arena_layout(plan.sizes, counts)
    K = lay.koff[-1]
    arr = (ctypes.c_int64 * plan.nt)(*counts)
    idx = torch.zeros(K + 2, dtype=torch.int64, device=gpu)
    words = torch.zeros(lay.words + 2, dtype=torch.int32, device=gpu)
    ip, wp = idx.data_ptr(), words.data_ptr()
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def both(a, i, w, h=plan.handle):
        i = None if i is None else ctypes.c_void_p(i)
        w = None if w is None else ctypes.c_void_p(w)
        return (L.omf_topk_pack_indices(h, a, i, w, st), L.omf_topk_unpack_indices(h, a, w, i, st))

    E = _lib.OMF_EINVAL
    assert both(arr, ip, wp) == (0, 0)
    assert both(arr, ip, wp, None) == (E, E)            # no plan
    assert both(None, ip, wp) == (E, E)                 # no counts
    assert both(arr, None, wp) == (E, E) and both(arr, ip, None) == (E, E)
    assert both(arr, ip, wp + 2) == (E, E)              # packed: 4 bytes
    assert both(arr, ip + 4, wp) == (E, E)              # indices: 8 bytes
    assert both(arr, ip + 8, wp + 4) == (0, 0)          # 8-byte indices and 4-byte words are enough
    assert both(arr, ip, ip + 8 * K - 4) == (E, E)      # the packed arena starts inside the indices
    assert both(arr, wp + 4 * (lay.words & ~1) - 8, wp) == (E, E)  # the indices start inside the packed arena
    for t, k in ((0, -1), (3, plan.sizes[3] + 1)):
        bad = list(counts)
        bad[t] = k
        a = (ctypes.c_int64 * plan.nt)(*bad)
        assert both(a, ip, wp) == (E, E)
        assert L.omf_topk_packed_words(plan.handle, a) == -1
    assert L.omf_topk_packed_words(None, arr) == -1 and L.omf_topk_packed_words(plan.handle, None) == -1
    assert L.omf_topk_packed_words(plan.handle, arr) == lay.words
    assert [L.omf_topk_index_bits(n) for n in (0, 1, 2, 3, 5, 2**32, 2**32 + 1)] == [-1, 1, 1, 2, 3, 32, -1]
    # the Python face checks its buffers before the call
    with pytest.raises(ValueError):
        plan.topk_pack_indices(counts, idx[:K - 1].contiguous() if K > 1 else idx[:0])
    with pytest.raises(ValueError):
        plan.topk_pack_indices(counts, idx.to(torch.int32))
    with pytest.raises(ValueError):
        plan.topk_unpack_indices(counts, words[:lay.words - 1])
    with pytest.raises(ValueError):
        plan.topk_unpack_indices(counts, words, indices_out=idx[:K - 1])
    with pytest.raises(ValueError):
        plan.topk_packed_words(list(counts)[:-1])
    torch.cuda.synchronize(gpu)
