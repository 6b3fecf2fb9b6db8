"""The Top-K receive matrix (tests/test_gpu_topk_recv_matrix.py) without a GPU: what the matrix assumes
of its inputs (tests/golden/topk_recv_inputs.py) and its numpy oracle against plainer statements of the
same rules (oracle.topk_desparse, numpy indexing raising IndexError, np.unique)."""

import numpy as np
import pytest
import torch

import oracle
import topk_recv_inputs as R

DECODE_KEYS = [(name, c, p) for name, L in R.LAYOUTS.items() for c, p in R.message_keys(L)]


def test_layouts_are_what_the_matrix_says():
    A = R.LAYOUTS["aligned"]
    assert A.arena_end % 4 != 0 and A.arena_end < 1_700_000
    assert any(o % R.SUPER for o in A.offsets) and R.SUPER in A.sizes
    T = R.LAYOUTS["tight"]
    assert all(o % 4 == 0 for o in T.offsets)
    shared_f4 = [t for t in range(T.nt - 1) if T.offsets[t + 1] - (T.offsets[t] + T.sizes[t]) < 4]
    shared_word = [t for t in range(T.nt - 1) if (T.offsets[t] + T.sizes[t] - 1) >> 5 == T.offsets[t + 1] >> 5]
    assert len(shared_f4) == T.nt - 1 and shared_word
    assert R.LAYOUTS["tiny"].sizes == [3] and R.LAYOUTS["tiny"].arena_end == 3
    G = R.LAYOUTS["large"]
    assert 2_100_000 < sum(G.sizes) < 2_300_000
    for name, L in R.LAYOUTS.items():
        assert L.nt <= 4096 and (name == "large" or L.arena_end < 1_700_000)
        for cname, counts in R.count_vectors(L).items():
            assert len(counts) == L.nt and all(0 <= c <= n for c, n in zip(counts, L.sizes)), (name, cname)
        for cname, ratio in R.RATIOS.items():
            if cname in R.count_vectors(L):
                assert R.count_vectors(L)[cname] == [oracle.topk_k(n, ratio) for n in L.sizes]


def test_count_vectors_have_their_zeros():
    for name in ("aligned", "tight", "many", "large"):
        cv = R.count_vectors(R.LAYOUTS[name])
        assert cv["zeros_lead"][0] == 0 and cv["zeros_lead"][-1] > 0
        assert cv["zeros_trail"][-1] == 0 and cv["zeros_trail"][0] > 0
        z = cv["zeros_mid"]
        assert z[0] > 0 and z[-1] > 0 and 0 in z
        assert not any(cv["none"])


@pytest.mark.parametrize("layout,cname,profile", DECODE_KEYS, ids=["-".join(k) for k in DECODE_KEYS])
def test_decode_profiles_unique_and_in_range(layout, cname, profile):
    L = R.LAYOUTS[layout]
    m = R.message(L, cname, profile)
    koff = R.koff_of(m.counts)
    assert m.ktot == koff[-1] == m.values.size
    assert (m.profile == "skipped") == bool(m.skipped.any())
    for t, n in enumerate(L.sizes):
        i = m.indices[koff[t]:koff[t + 1]]
        keep = ~m.skipped[koff[t]:koff[t + 1]]
        assert ((i[keep] >= 0) & (i[keep] < n)).all()
        assert np.unique(i[keep]).size == keep.sum()
        out = i[~keep]
        assert ((out < 0) | (out >= n)).all()
        if out.size and out.size >= 6 * 2:  # every skipped kind is present in a tensor with room for them
            low = out & 0xFFFFFFFF
            assert (out == -1).any() and (out == n).any() and (out == n + 3).any() and (out == -n - 1).any()
            assert ((out >= R.TWO32) & (low < n)).any() and ((out <= -R.TWO32 + n) & (low < n)).any()
    if m.ktot >= 8:
        bits = set(m.values.view(np.uint32).tolist())
        assert set(R.SPECIAL_BITS) <= bits


def test_skipped_aliases_point_at_unselected_elements():
    """An index valid only after truncation to 32 bits aliases an element no other entry selects: a
    decoder that truncated would change a byte the oracle leaves alone."""
    L = R.LAYOUTS["aligned"]
    m = R.message(L, "r05", "skipped")
    koff = R.koff_of(m.counts)
    seen = 0
    for t, n in enumerate(L.sizes):
        i = m.indices[koff[t]:koff[t + 1]]
        alias = i[(np.abs(i) >= R.TWO32 - n)] & 0xFFFFFFFF
        seen += alias.size
        assert not np.isin(alias, i).any()
    assert seen > 100


def test_clustered_overflows_an_unstaged_bucket():
    L = R.LAYOUTS["aligned"]
    s = R.cluster_super(L)
    for cname in ("clu20k", "r05"):
        m = R.message(L, cname, "clustered")
        caps, got = R.caps_ref(L, m.counts), R.super_counts(L, m.counts, m.indices)
        assert got[s] > caps[s] > R.DEC_STAGE, (cname, got[s], caps[s])
        i = m.per[R.CLUSTER_TENSOR] + L.offsets[R.CLUSTER_TENSOR]
        assert (i >> R.SUPER_BITS == s).all()
        assert (np.bincount((i >> R.SUB_BITS) & 3, minlength=4) > 0).all()
    m = R.message(L, "clu20k", "clustered")
    caps, got = R.caps_ref(L, m.counts), R.super_counts(L, m.counts, m.indices)
    assert caps[s] == 2756 and m.counts[R.CLUSTER_TENSOR] == 20000
    assert 17_000 <= int(np.maximum(got - caps, 0).sum()) <= 17_500
    # the uniform message of the same counts stays inside every bucket, staged
    u = R.message(L, "clu20k", "uniform")
    assert (R.super_counts(L, u.counts, u.indices) <= np.minimum(caps, R.DEC_STAGE)).all()


def test_ratio_001_buckets_are_all_staged():
    """Why the unstaged path needs a crafted message: a ratio-0.01 bucket holds about 2 * 655 + 256
    entries (a little more where small tensors round their k up to 1), fewer than a workgroup stages."""
    for L in R.LAYOUTS.values():
        assert max(R.caps_ref(L, L.ks(0.01))) <= 2 * 655 + 256 + 8 < R.DEC_STAGE


def test_full_tensor_reaches_the_clamp():
    for name, t in R.FULL_TENSOR.items():
        L = R.LAYOUTS[name]
        m = R.message(L, "full", "uniform")
        caps, got = R.caps_ref(L, m.counts), R.super_counts(L, m.counts, m.indices)
        inside = [s for s in range(L.nsuper)
                  if L.offsets[t] <= s << R.SUPER_BITS and (s + 1) << R.SUPER_BITS <= L.offsets[t] + L.sizes[t]]
        assert inside and all(caps[s] == R.SUPER == got[s] for s in inside)
        assert (got <= caps).all()  # full, not overflowing


def test_many_has_a_place_block_over_512_tensors():
    L = R.LAYOUTS["many"]
    for cname in ("r01", "r05", "edges"):
        m = R.message(L, cname, "uniform" if cname != "edges" else "edges_of_tiles")
        koff = R.koff_of(m.counts)
        tensor_of = lambda j: int(np.searchsorted(koff[:L.nt], j, side="right")) - 1  # noqa: E731
        spans = [tensor_of(min(j0 + R.DEC_CHUNK, m.ktot) - 1) - tensor_of(j0) for j0 in range(0, m.ktot, R.DEC_CHUNK)]
        assert max(spans) >= R.DEC_WIN, (cname, spans)


def test_large_passes_the_scatter_cap():
    L = R.LAYOUTS["large"]
    m = R.message(L, "most", "uniform")
    assert m.ktot >= 1_100_000 and m.ktot > R.SCATTER_CAP
    assert max(m.counts) >= 1_100_000 and max(m.counts) > R.SCATTER_CAP  # the per-tensor decode passes it too
    assert sum(R.check_counts(L)) > 2048 * R.CHECK_BLOCK  # and the index check its own cap


def test_edges_of_tiles_touch_every_edge():
    for L in R.LAYOUTS.values():
        m = R.message(L, "edges", "edges_of_tiles")
        koff = R.koff_of(m.counts)
        pos = np.concatenate([o + m.indices[koff[t]:koff[t + 1]] for t, o in enumerate(L.offsets)])
        assert L.arena_end - 1 in pos
        inside = ~R.padding_mask(L)
        for edge in range(0, L.arena_end, R.SUB):
            for p in (edge, edge - 1):
                if 0 <= p and inside[p]:
                    assert p in pos, (L.name, p)
        for o, n in zip(L.offsets, L.sizes):
            assert o in pos and o + n - 1 in pos


def test_base_keeps_an_unselected_negative_zero():
    L = R.LAYOUTS["aligned"]
    base = R.make_base(L)
    pad = R.padding_mask(L)
    assert (base[pad] == np.float32(R.CANARY)).all()
    bits = base.view(np.uint32)
    for b in R.BASE_BITS:
        assert (bits[~pad] == b).sum() >= 8
    m = R.message(L, "r05", "uniform")
    got = R.decode_ref(2, base, L, m.counts, m.values, m.indices)
    untouched = got.view(np.uint32) == bits
    assert (untouched & (bits == 0x80000000)).sum() >= 4  # mode 2 leaves these -0.0 (an add of +0 would not)
    assert (base + np.float32(0.0)).view(np.uint32)[bits == 0x80000000].max() == 0


def test_decode_ref_mode0_equals_topk_desparse():
    for name, L in R.LAYOUTS.items():
        for cname, profile in R.message_keys(L):
            if profile == "skipped":
                continue
            m = R.message(L, cname, profile)
            got = R.decode_ref(0, None, L, m.counts, m.values, m.indices)
            assert not got[R.padding_mask(L)].view(np.uint32).any()
            koff = R.koff_of(m.counts)
            for t, (o, n) in enumerate(zip(L.offsets, L.sizes)):
                v, i = m.values[koff[t]:koff[t + 1]], m.indices[koff[t]:koff[t + 1]]
                want = oracle.topk_desparse(torch.from_numpy(v.copy()), torch.from_numpy(i.copy()), n).numpy()
                assert got[o:o + n].tobytes() == want.tobytes(), (name, cname, profile, t)


def test_decode_ref_modes_touch_nothing_else():
    L = R.LAYOUTS["tight"]
    base = R.make_base(L)
    m = R.message(L, "r05", "skipped")
    koff = R.koff_of(m.counts)
    sel = np.zeros(L.arena_end, bool)
    for t, (o, n) in enumerate(zip(L.offsets, L.sizes)):
        i = m.indices[koff[t]:koff[t + 1]]
        sel[o + i[(i >= 0) & (i < n)]] = True
    for mode in (1, 2):
        got = R.decode_ref(mode, base, L, m.counts, m.values, m.indices)
        assert (got.view(np.uint32)[~sel] == base.view(np.uint32)[~sel]).all()
    one = R.decode_ref(1, base, L, m.counts, m.values, m.indices)
    zero = R.decode_ref(0, None, L, m.counts, m.values, m.indices)
    assert (one.view(np.uint32)[sel] == zero.view(np.uint32)[sel]).all()
    # mode 2, element by element in Python floats rounded once to fp32
    two = R.decode_ref(2, base, L, m.counts, m.values, m.indices)
    for t, (o, n) in enumerate(zip(L.offsets, L.sizes)):
        for j in range(koff[t], koff[t + 1]):
            i = int(m.indices[j])
            if 0 <= i < n:
                with np.errstate(all="ignore"):
                    want = np.float32(float(base[o + i]) + float(m.values[j]))
                assert np.isnan(want) == np.isnan(two[o + i])
                assert np.isnan(want) or want.tobytes() == two[o + i].tobytes()


def _numpy_index_check(n, idx):
    """Plain numpy: does dense[i] = v raise for any entry, and where does each valid one land."""
    bad, where = False, []
    for i in idx.tolist():
        d = np.zeros(n, np.int8)
        try:
            d[i] = 1
            where.append(int(np.flatnonzero(d)[0]))
        except IndexError:
            bad = True
            where.append(i)
    return bad, where


def test_check_ref_equals_numpy_indexing():
    for name in ("tight", "tiny", "many"):
        L = R.LAYOUTS[name]
        for mname, (counts, idx) in R.check_messages(L).items():
            wrapped, bad = R.check_ref(L, counts, idx)
            koff = R.koff_of(counts)
            want_bad = R.NO_BAD
            for t, n in enumerate(L.sizes):
                if n > 600:
                    continue  # (small cases: a dense array per entry)
                b, where = _numpy_index_check(n, idx[koff[t]:koff[t + 1]])
                assert wrapped[koff[t]:koff[t + 1]].tolist() == where, (name, mname, t)
                if b:
                    want_bad = min(want_bad, t)
            if all(n <= 600 for t, n in enumerate(L.sizes) if counts[t]):
                assert bad == want_bad, (name, mname)


def test_check_messages_have_their_cases():
    for name, L in R.LAYOUTS.items():
        msgs = R.check_messages(L)
        res = {k: R.check_ref(L, c, i) for k, (c, i) in msgs.items()}
        for k in ("clean", "wrap_only", "none"):
            assert res[k][1] == R.NO_BAD, (name, k)
        counts, idx = msgs["clean"]
        assert (res["clean"][0] == idx).all() and (res["wrap_only"][0] != msgs["wrap_only"][1]).any()
        live = [t for t, c in enumerate(counts) if c]
        assert res["last_only"][1] == live[-1]
        a, b, c = R.multi_bad_tensors(L)
        assert res["multi_bad"][1] == a and a <= b <= c
        assert res["extremes"][1] == live[len(live) // 2]
        e = msgs["extremes"][1]
        if max(counts) >= 4:
            assert R.I64_MIN in e and R.I64_MAX in e and (e >= R.TWO32).any() and (e <= -R.TWO32 + max(L.sizes)).any()
        if name in ("aligned", "many", "tight"):
            assert 0 in counts[1:-1] and a < b < c  # zero-count tensors between non-empty ones
            assert sum(counts) > R.CHECK_BLOCK      # more than one workgroup
            koff = R.koff_of(counts)
            gx = -(-sum(counts) // R.CHECK_BLOCK)
            wg = lambda j: (int(j) // 256) % gx  # noqa: E731
            # the lowest bad tensor's one bad entry is its last (not the message's first bad entry), in
            # another workgroup than the middle tensor's; the last tensor's are in several workgroups
            assert wg(koff[a + 1] - 1) != wg(koff[b]), (name, gx)
            assert wg(koff[c]) not in (wg(koff[a + 1] - 1), wg(koff[b])) or counts[c] > 512, (name, gx)
            if counts[c] > 512:
                assert len({wg(j) for j in range(koff[c], koff[c + 1], 3)}) > 1, (name, gx)


def test_dup_ref_equals_np_unique():
    for name, L in R.LAYOUTS.items():
        for mname, (counts, idx, clean) in R.dup_messages(L).items():
            flags = R.dup_ref(L, counts, idx)
            koff = R.koff_of(counts)
            for t, n in enumerate(L.sizes):
                i = idx[koff[t]:koff[t + 1]]
                wrapped_valid = [x for x in i.tolist() if 0 <= x < n]
                _, cnt = np.unique(np.array(wrapped_valid, np.int64), return_counts=True)
                assert flags[t] == int(cnt.size > 0 and cnt.max() > 1), (name, mname, t)
            assert not R.dup_ref(L, counts, clean).any(), (name, mname)
            # clean selects exactly the positions of the message
            for t, n in enumerate(L.sizes):
                i, c = idx[koff[t]:koff[t + 1]], clean[koff[t]:koff[t + 1]]
                assert set(i[(i >= 0) & (i < n)].tolist()) == set(c[(c >= 0) & (c < n)].tolist())
            want = {"none": False, "oor": False, "shared_word": False, "wave": True, "far": True}[mname]
            assert bool(flags.any()) == want, (name, mname)


def test_dup_messages_have_their_cases():
    counts, idx, _ = R.dup_messages(R.LAYOUTS["large"])["far"]
    assert idx[R.FAR_A] == idx[R.FAR_B] and R.FAR_B - R.FAR_A >= R.DUP_TRIP and R.FAR_B < counts[0]
    assert R.FAR_B - R.FAR_A >= 600_000
    T = R.LAYOUTS["tight"]
    counts, idx, _ = R.dup_messages(T)["shared_word"]
    assert counts == T.sizes  # the last element of every tensor and the first of the next: each once
    for name, L in R.LAYOUTS.items():
        msgs = R.dup_messages(L)
        if "wave" in msgs:
            counts, idx, _ = msgs["wave"]
            koff = R.koff_of(counts)
            flagged = np.flatnonzero(R.dup_ref(L, counts, idx))
            assert flagged.size >= 1 and all(idx[koff[t]] == idx[koff[t] + 1] for t in flagged)
            assert any(koff[t] // 64 == (koff[t] + 1) // 64 for t in flagged)  # both in one wave
        if "oor" in msgs:
            counts, idx, _ = msgs["oor"]
            koff = R.koff_of(counts)
            reps = 0
            for t, n in enumerate(L.sizes):
                i = idx[koff[t]:koff[t + 1]]
                out = i[(i < 0) | (i >= n)]
                reps += out.size - np.unique(out).size
            assert reps > 0


def test_caps_ref_formula():
    L = R.LAYOUTS["aligned"]
    caps = R.caps_ref(L, R.count_vectors(L)["none"])
    assert caps == [256] * L.nsuper
    caps = R.caps_ref(L, L.ks(1.0))
    assert max(caps) == R.SUPER
