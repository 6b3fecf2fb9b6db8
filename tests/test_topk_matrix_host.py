"""The Top-K oracle matrix (tests/test_gpu_topk_matrix.py) without a GPU: the index-order oracle
(oracle/topk.py: topk_select_index_order, topk_ef_step) against a brute-force selection, torch.topk and
the reference's golden outputs, and what the matrix assumes of its inputs
(tests/golden/topk_matrix_inputs.py).
"""

import ctypes
import hashlib

import numpy as np
import torch

import oracle
import topk_matrix_inputs as M
from omnifed_amd.hybrid.communicator import global_grpc_pb2 as pb

NAN = np.array([M.NAN_BITS], np.uint32).view(np.float32)[0]

# SHA-256 of each plan's first-call arena (the recipes are part of what the matrix checks)
ARENA_SHA = {
    "edges": "72a30c091a8d3b58e595a33138be9fab6bebdb2eb2ac20075914b322948f148f",
    "sampled": "1e1ff19f5118e98c23050784af37d2254807b8f1c27c8083725d43550a7ad8bf",
    "many": "f7e8e6d9835a734e3918e51716f98c58f88dd74f929b5f116053739a3aed3fce",
    "tight": "61431e2f86ebf662023c4e7679f460a79539ca9342bf017f7437b41afc578284",
}


def _brute(t, k):
    """k times: the largest remaining key, the lowest index among equals (pure Python)."""
    keys = [int(b) & 0x7FFFFFFF for b in np.asarray(t, np.float32).view(np.uint32)]
    left, out = set(range(len(keys))), []
    for _ in range(k):
        best = max(keys[i] for i in left)
        i = min(i for i in left if keys[i] == best)
        out.append(i)
        left.remove(i)
    return out


def _small_arrays():
    rng = np.random.default_rng(1)
    yield np.array([0.0], np.float32)
    yield np.array([-0.0, 0.0, -0.0, 0.0], np.float32)
    yield np.array([1.0, -1.0, 1.0, -2.0, 2.0, 0.0, -0.0], np.float32)
    yield np.array([np.inf, NAN, -np.inf, NAN, 3.0, M.FLT_MAX, -M.FLT_MAX, 1e-45, -1e-45, 0.0], np.float32)
    for n in (2, 3, 17, 64):
        yield (np.rint(2.0 * rng.standard_normal(n)) / 2.0).astype(np.float32)
        yield rng.standard_normal(n).astype(np.float32)
    spec = M.PLANS["many"]
    for t in range(14):  # sizes 1, 7, 100 of every basic kind among them
        if spec.sizes[t] <= 100:
            yield M.make_tensor(spec, t)


def test_select_equals_brute_force():
    for a in _small_arrays():
        for k in sorted({1, a.size // 3 or 1, a.size - 1 or 1, a.size}):
            got = oracle.topk_select_index_order(a, k)
            assert got.dtype == np.int64 and got.tolist() == _brute(a, k), (a.tolist(), k)


def test_select_magnitudes_equal_torch_topk():
    spec = M.PLANS["edges"]
    for t, n in enumerate(spec.sizes):
        a = M.make_tensor(spec, t)
        for ratio in spec.ratios:
            k = oracle.topk_k(n, ratio)
            idx = oracle.topk_select_index_order(a, k)
            want, _ = torch.topk(torch.from_numpy(a).abs(), k, sorted=True)
            # (NaN != NaN: compare the bits; |NaN| keeps the payload, torch.topk ranks NaN first too)
            assert np.abs(a[idx]).tobytes() == want.numpy().tobytes(), (spec.names[t], ratio)


def _layer(golden, key):
    L = pb.LayerState()
    L.ParseFromString(golden[key].tobytes())
    return L


def test_oracle_against_reference_goldens(golden, golden_index):
    """The reference's three error-feedback calls per case: topk_ef_step(rule="torch") reproduces its
    values, indices and residual bytes, and wherever the k-th magnitude is unique the index-order
    selection is the same set."""
    unique_cases = 0
    for c in golden_index["topk"]:
        n, k = c["n"], oracle.topk_k(c["n"], c["ratio"])
        res = None
        for call in c["calls"]:
            key = f"topk/{c['id']}/{call}"
            x = golden[key + "/x"].reshape(-1)
            G = _layer(golden, key + "/layer")
            gidx = np.frombuffer(G.indices_data, np.int64)
            gval = np.frombuffer(G.values_data, np.float32)
            v, i, new = oracle.topk_ef_step(x, res, 2 if res is None else 1, 1.0, k, "torch")
            assert i.tobytes() == gidx.tobytes(), key
            assert v.tobytes() == gval.tobytes(), key
            assert new.tobytes() == golden[key + "/residual"].tobytes(), key
            tp = x if res is None else (res + x).astype(np.float32)
            keys = np.sort(oracle.mag_keys(tp))[::-1]
            if k == n or keys[k - 1] != keys[k]:
                unique_cases += 1
                v2, i2, new2 = oracle.topk_ef_step(x, res, 2 if res is None else 1, 1.0, k, "index")
                assert set(i2.tolist()) == set(gidx.tolist()), key
                assert new2.tobytes() == new.tobytes(), key
            res = new
    assert unique_cases == 15, unique_cases  # every call of every case, as the fixture stands


def test_ef_step_arithmetic():
    """Two roundings (no FMA) against fp64 arithmetic rounded twice, t' - t' on the selection, the
    inputs untouched."""
    rng = np.random.default_rng(2)
    n = 4096
    x = (rng.uniform(0.5, 2.0, n) * np.where(rng.random(n) < 0.5, -1, 1)).astype(np.float32)
    r = (rng.uniform(0.5, 2.0, n) * np.where(rng.random(n) < 0.5, -1, 1)).astype(np.float32)
    x0, r0 = x.copy(), r.copy()
    a64 = np.float64(np.float32(0.3))
    prod = (a64 * x.astype(np.float64)).astype(np.float32)               # exact in fp64, rounded once
    two = (r.astype(np.float64) + prod.astype(np.float64)).astype(np.float32)  # exact in fp64, rounded once
    fused = (r.astype(np.float64) + a64 * x.astype(np.float64)).astype(np.float32)
    assert (two != fused).any()  # the inputs tell the two apart
    v, i, new = oracle.topk_ef_step(x, r, 1, 0.3, n, "index")
    tp = np.empty(n, np.float32)
    tp[i] = v
    assert tp.tobytes() == two.tobytes()
    assert new.tobytes() == np.zeros(n, np.float32).tobytes()  # +0 on every selected slot
    v, i, new = oracle.topk_ef_step(x, r, 2, 0.3, 7, "index")
    assert v.tobytes() == prod[i].tobytes() and np.delete(new, i).tobytes() == np.delete(prod, i).tobytes()
    assert x.tobytes() == x0.tobytes() and r.tobytes() == r0.tobytes()
    assert oracle.topk_ef_step(x, None, 0, 1.0, 1)[2] is None
    # a non-finite t' leaves NaN on its selected slot: itself, or inf - inf's NaN as gfx950 and x86 write it
    s = np.array([1.0, -np.inf, NAN, 2.0], np.float32)
    v, i, new = oracle.topk_ef_step(s, None, 2, 1.0, 3, "index")
    assert i.tolist() == [2, 1, 3]
    assert new.view(np.uint32).tolist() == [0x3F800000, 0xFFC00000, M.NAN_BITS, 0]


# ------------------------------------------------------------------ the inputs

def test_inputs_are_pinned():
    for name, spec in M.PLANS.items():
        a, b = M.make_arena(spec), M.make_arena(spec)
        assert a.tobytes() == b.tobytes()
        assert hashlib.sha256(a.tobytes()).hexdigest() == ARENA_SHA[name], name
        pad = M.padding_mask(spec)
        assert pad.any() and (a[pad] == np.float32(M.CANARY)).all()
        fin = a[~pad][np.isfinite(a[~pad])]
        assert np.abs(fin[np.abs(fin) < M.FLT_MAX]).max() < abs(M.CANARY)  # only +-FLT_MAX itself is larger
        for call in (1, 2):
            x = M.make_arena(spec, call)
            assert np.isfinite(x).all() and (x[pad] == np.float32(M.CANARY)).all()
    nan = M.make_arena(M.PLANS["edges"])
    nan = nan[np.isnan(nan)]
    assert nan.size >= 3 and (nan.view(np.uint32) == M.NAN_BITS).all()  # one payload: NaN ties go by index


def test_plans_cover_the_edges():
    e, s, m = (M.PLANS[p] for p in ("edges", "sampled", "many"))
    assert e.sizes == [1, 2, 3, 5, 100, 101, 511, 512, 513, 4095, 4096, 4097, 16383, 16384, 16385]
    assert set(e.kinds) == set(M.BASIC)  # every basic kind lands on a tensor of edges
    assert s.sizes == [70_001, 65_536, 262_144, 262_147, 1 << 20]
    assert len(m.sizes) == 300 and set(m.sizes) == {1, 7, 100, 513, 5000}
    assert {(k, n) for k, n in zip(m.kinds, m.sizes)} == {(k, n) for k in M.BASIC for n in (1, 7, 100, 513, 5000)}
    assert oracle.topk_k(100, 0.29) == 28  # 0.29 * 100 truncates
    for spec in (e, s, m):
        assert spec.arena_end <= 2_600_000
        assert all(o % 64 == 0 for o in spec.offsets)
        assert all(a + n <= b for a, n, b in zip(spec.offsets, spec.sizes, spec.offsets[1:]))
        for ratio in spec.ratios:
            assert all(1 <= k <= n for k, n in zip(spec.ks(ratio), spec.sizes))
    assert e.ks(1.0) == e.sizes  # k == n
    t = M.PLANS["tight"]  # the closest packing the ABI allows: starts at the next multiple of 4
    assert t.sizes == e.sizes and t.kinds == e.kinds
    assert t.offsets[0] == 0 and all(b == (a + n + 3) // 4 * 4 for a, n, b in zip(t.offsets, t.sizes, t.offsets[1:]))
    assert all(M.make_tensor(t, i).tobytes() == M.make_tensor(e, i).tobytes() for i in range(len(t.sizes)))


def test_topk_k_equals_the_library():
    from omnifed_amd import _lib
    from omnifed_amd.build import build

    build()
    L = _lib.lib()
    for spec in M.PLANS.values():
        for ratio in spec.ratios:
            for n in set(spec.sizes):
                assert L.omf_topk_k(ctypes.c_int64(n), ctypes.c_double(ratio)) == oracle.topk_k(n, ratio) \
                    == M.topk_k(n, ratio), (n, ratio)


def _kth_tie(a, k):
    """(keys equal to the k-th inside the top k, keys equal to it in the tensor)."""
    keys = oracle.mag_keys(a)
    kth = np.sort(keys)[::-1][k - 1]
    return int(k - (keys > kth).sum()), int((keys == kth).sum())


def test_basic_kinds_have_their_properties():
    for spec in M.PLANS.values():
        straddle = {r: [0, 0] for r in spec.ratios}  # quantised tensors (k < n): ties across rank k, all
        for t, (kind, n) in enumerate(zip(spec.kinds, spec.sizes)):
            a = M.make_tensor(spec, t)
            assert a.dtype == np.float32 and a.shape == (n,)
            keys = oracle.mag_keys(a)
            for ratio in spec.ratios:
                k = oracle.topk_k(n, ratio)
                inside, equal = _kth_tie(a, k)
                if kind == "gauss":
                    assert equal == 1  # no tie at rank k (fp32 normals of 5000 draws may collide elsewhere)
                elif kind == "quantised" and k < n:
                    straddle[ratio][0] += equal > inside  # the tie straddles rank k
                    straddle[ratio][1] += 1
                    # (plan many's 60 small quantised tensors: rank k may fall on a tie's last element)
                    assert equal > inside or spec.name == "many", (spec.names[t], ratio)
                elif kind == "all_equal":
                    assert np.unique(keys).size == 1 and (n < 3 or (a > 0).any() and (a < 0).any())
                elif kind == "sparse":
                    assert np.count_nonzero(a) < k, (spec.names[t], ratio)
                    zeros = a[a == 0]
                    assert n < 2 or (np.signbit(zeros).any() and not np.signbit(zeros).all())
                elif kind == "ramp_up":
                    assert set(oracle.topk_select_index_order(a, k).tolist()) == set(range(n - k, n))
                elif kind == "ramp_down":
                    assert oracle.topk_select_index_order(a, k).tolist() == list(range(k))
            if kind == "quantised":
                assert n < 16 or np.unique(keys).size < 64  # ties everywhere
            if kind == "specials" and n >= 16:
                assert np.isnan(a).sum() == 3 and np.isposinf(a).sum() == 2 and np.isneginf(a).sum() == 1
                assert (np.abs(a) == M.FLT_MAX).sum() == 2
                sub = (keys > 0) & (keys < 0x00800000)
                assert sub.sum() == 4 and (keys == 0).sum() == 3 and np.signbit(a[keys == 0]).sum() == 2
        for ratio, (yes, every) in straddle.items():
            assert (every >= 1 or ratio == 1.0) and yes >= 0.75 * every, (spec.name, ratio, yes, every)


def test_sampled_kinds_reach_their_paths():
    """The crafted tensors, by the sampler's own positions (sample_runs = 2048)."""
    spec = M.PLANS["sampled"]
    # sample_is_top: every sampled position carries the top magnitude; fewer of them than k at 0.1
    t = spec.tensor_of("sample_is_top")
    n, a = spec.sizes[t], M.make_tensor(spec, t)
    sp = M._sample_positions(n, t, M.SAMPLE_RUNS)
    assert (a[sp] == 10.0).all() and (a == 10.0).sum() == sp.size == 4096 and (np.delete(a, sp) == 1.0).all()
    assert sp.size < oracle.topk_k(n, 0.1)                  # the redo
    assert 2048 < sp.size <= 4096 and oracle.topk_k(n, 0.01) < sp.size  # one big fine bin at 0.01
    # under_sampled: more than k elements above twice the largest sampled magnitude
    t = spec.tensor_of("under_sampled")
    n, a = spec.sizes[t], np.abs(M.make_tensor(spec, t))
    sp = M._sample_positions(n, t, M.SAMPLE_RUNS)
    k = oracle.topk_k(n, 0.01)
    assert ((a[sp] >= 1.0) & (a[sp] < 2.0)).sum() == M.UNDER_SAMPLED_HI and (a[sp] < 2.0).all()
    assert (a[sp] < 0.5).sum() == sp.size - M.UNDER_SAMPLED_HI
    assert (a > 2.0 * a[sp].max()).sum() == M.UNDER_SAMPLED_TOP > k
    # ... and the sample's own threshold (k S / n + 6 sigma + 32 samples from the top) lies in [1, 2)
    S = sp.size
    m = k * S / n
    assert m + 6.0 * np.sqrt(m) + 32.0 < M.UNDER_SAMPLED_HI
    # cluster: more than a bucket's 4096 equal keys inside the top k at 0.1, below every kept key at 0.01
    t = spec.tensor_of("cluster")
    n, a = spec.sizes[t], np.abs(M.make_tensor(spec, t))
    eq = (a == M.CLUSTER_MAG).sum()
    assert eq == M.CLUSTER_N > 4096
    assert (a > M.CLUSTER_MAG).sum() + eq <= oracle.topk_k(n, 0.1)
    # at 0.01 the threshold sits near rank k (1 + 6 / sqrt(m)) + 32 n / S < 2 k: far above the cluster
    assert (a > 1.1 * M.CLUSTER_MAG).sum() > 2 * oracle.topk_k(n, 0.01)
    # the other two hold what their kinds promise at this size
    assert np.isnan(M.make_tensor(spec, spec.tensor_of("specials"))).sum() == 3
