"""The bucketed PS step (omf_ps_sum_encode_bucketed): K clients' bucketed payloads summed onto the accumulator,
averaged and re-encoded in one launch, held to a plain numpy fp32 loop, to the CPU oracle's levels and to the
calls it replaces; its fallbacks, its refusals and the aggregator's routing.

One plan per output bucket size d with tensors of less than a quad, around a 32-element group, a bucket and a
4 Ki block, a partial group inside a partial bucket in a block's second row and more than one 16 Ki item; one
client's norms zeroed on one tensor, one tensor of the start arena -0.0; canaries in the padding of avg_out /
sum_out and in the unwritten packed groups, guards round every output."""

import itertools

import numpy as np
import pytest
import torch

import oracle
from omnifed_amd import codec
from omnifed_amd.hybrid.communicator.global_grpc_compression import build_global_compressor, encode_updates_dict
from omnifed_amd.ps import DeviceAggregator
from oracle import bitpack

pytestmark = pytest.mark.gpu

SEED, OFF, DIV = 0xB0C, 3, 7.0
GUARD = 64
FCANARY, ICANARY = 3e4, 0x5A5A5A5A
D_CASES = ((64, 64), (512, 512), (4096, 4096), (256, 1024))               # (d_in, d_out)
WIRES = ((8, 4), (32, 8), (0, 1), (0, 4), (0, 8), (0, 14))               # (width_in, s_in): packed b = 3, 6, 10, 16
K_START = ((0, True), (1, False), (3, True), (8, False), (9, True))
OUTS = ((4, False), (8, False), (4, True), (8, True))                    # (s_out, packed)
CASES = [(*dd, *w, *K_START[i % 5], *OUTS[i % 4]) for i, (dd, w) in enumerate(itertools.product(D_CASES, WIRES))]


def _sizes(d):
    return [1, 3, 31, 32, 33, d - 1, d, d + 1, 2 * d + 5, 4095, 4096, 4097, 4096 + d + 1, 16383, 16384 + d // 2 + 3]


def _bidx(plan, d):
    """Every arena element's index into the bucket-norm arena of size d."""
    bidx = np.zeros(plan.arena_end, dtype=np.int64)
    for o, n, b in zip(plan.offsets, plan.sizes, plan.bucket_layout(d)[0]):
        bidx[o:o + n] = b + np.arange(n) // d
    return bidx


@pytest.fixture(scope="module")
def arenas(gpu):
    """d_out -> (plan, mask of the tensors' elements, start arena: canary padding, tensor 3 all -0.0)."""
    out = {}
    for d in sorted({dd[1] for dd in D_CASES}):
        plan = codec.Plan(_sizes(d), device=gpu)
        mask = torch.zeros(plan.arena_end, dtype=torch.bool)
        acc = torch.full((plan.arena_end,), FCANARY, device=gpu)
        g = torch.Generator(device=gpu).manual_seed(d)
        for o, n in zip(plan.offsets, plan.sizes):
            mask[o:o + n] = True
            acc[o:o + n] = torch.randn(n, device=gpu, generator=g) * 1e-3
        acc[plan.offsets[3]:plan.offsets[3] + plan.sizes[3]] = -0.0
        out[d] = (plan, mask, acc)
    return out


def _clients(plan, gpu, K, width, s, d):
    """K clients' (payload, norms, levels as an int64 arena) from the project's encoders, one seed each; client
    0's norms zeroed on tensor 5 (a tensor absent from its message)."""
    out = []
    boff, _ = plan.bucket_layout(d)
    for c in range(K):
        x = torch.randn(plan.arena_end, device=gpu, generator=torch.Generator(device=gpu).manual_seed(100 + c)) * 1e-3
        enc = plan.qsgd_encode_bucketed_packed if width == 0 else plan.qsgd_encode_bucketed
        q, bn = enc(x, s, d, seed=c + 1)
        if c == 0:
            bn[boff[5]:boff[6]] = 0.0
        lv = np.zeros(plan.arena_end, dtype=np.int64)
        qh = q.cpu().numpy()
        for o, n in zip(plan.offsets, plan.sizes):
            b = s + 2
            lv[o:o + n] = (bitpack.unpack(qh.view(np.uint8)[o * b // 8:o * b // 8 + (n * b + 7) // 8].tobytes(), n, 2 ** s)
                           if width == 0 else qh[o:o + n])
        out.append((q, bn, lv))
    return out


def _written(plan, mask, b):
    """The mask of a packed arena's words whose 32-element group holds a tensor element."""
    groups = -(-plan.arena_end // 32)
    m = torch.zeros(groups * 32, dtype=torch.bool)
    m[:plan.arena_end] = mask
    return m.view(groups, 32).any(dim=1).repeat_interleave(b)


def _outputs(plan, gpu, s_out, d_out, packed):
    """Guard-banded, canary-filled (avg, sum, q, bnorm) buffers and the views the call writes."""
    A, nb = plan.arena_end, plan.bucket_layout(d_out)[1]
    width = codec.storage_width(2 ** s_out)
    nq = plan.packed_words(2 ** s_out) if packed else plan.payload_elems(width)
    bufs = {"avg": torch.full((A + 2 * GUARD,), FCANARY, device=gpu), "sum": torch.full((A + 2 * GUARD,), FCANARY, device=gpu),
            "q": torch.full((nq + 2 * GUARD,), ICANARY if packed or width == 32 else 0x55,
                            dtype=torch.int32 if packed or width == 32 else torch.int8, device=gpu),
            "bn": torch.full((nb + 2 * GUARD,), -7.0, device=gpu)}
    views = {k: v[GUARD:GUARD + n] for (k, v), n in zip(bufs.items(), (A, A, nq, nb))}
    return bufs, views


def _guards_kept(bufs, views):
    return all(bool((b[:GUARD] == b[0]).all()) and bool((b[GUARD + views[k].numel():] == b[0]).all()) for k, b in bufs.items())


def _the_calls(plan, acc, cl, width, s_in, d_in, s_out, d_out, packed, start):
    """The sequence the call replaces: (sum, avg, payload, norms)."""
    y = acc.clone() if start else torch.zeros_like(acc)
    if cl and width == 0:
        plan.qsgd_decode_sum_bucketed_packed([c[0] for c in cl], 2 ** s_in, d_in, [c[1] for c in cl], y_out=y, init=True)
    elif cl:
        plan.qsgd_decode_sum_bucketed([c[0] for c in cl], width, 2 ** s_in, d_in, [c[1] for c in cl], y_out=y, init=True)
    avg = codec.div_(y.clone(), DIV)
    enc = plan.qsgd_encode_bucketed_packed if packed else plan.qsgd_encode_bucketed
    return (y, avg, *enc(avg, s_out, d_out, seed=SEED, offset=OFF))


@pytest.mark.parametrize("d_in,d_out,width,s_in,K,start,s_out,packed", CASES)
def test_fused_step_against_numpy_and_the_calls(gpu, arenas, d_in, d_out, width, s_in, K, start, s_out, packed):
    plan, mask, acc0 = arenas[d_out]
    m, A = mask.to(gpu), plan.arena_end
    cl = _clients(plan, gpu, K, width, s_in, d_in)
    acc = acc0.clone()
    keep = [t.clone() for c in cl for t in c[:2]]
    bufs, out = _outputs(plan, gpu, s_out, d_out, packed)
    in_place = start and K % 2 == 1  # sum_out is the accumulator itself
    avg, q, bn = plan.ps_sum_encode_bucketed(
        acc if start else None, [c[0] for c in cl], [c[1] for c in cl], width, 2 ** s_in, d_in, DIV, s_out, d_out,
        pack_out=packed, sum_out=acc if in_place else out["sum"], avg_out=out["avg"], seed=SEED, offset=OFF,
        q_out=out["q"], bnorm_out=out["bn"])
    assert plan.last_encoder == "bucketed_ps"
    torch.cuda.synchronize()
    # the plain numpy loop, in client order
    bi = _bidx(plan, d_in)
    s = acc0.cpu().numpy().copy() if start else np.zeros(A, dtype=np.float32)
    for _, nrm, lv in cl:
        term = ((nrm.cpu().numpy()[bi] * lv.astype(np.float32)).astype(np.float32) / np.float32(2 ** s_in)).astype(np.float32)
        s = (s + term).astype(np.float32)
    want_avg = (s / np.float32(DIV)).astype(np.float32)
    got_sum = (acc if in_place else out["sum"]).cpu().numpy()
    mh = mask.numpy()
    assert np.array_equal(got_sum.view(np.int32)[mh], s.view(np.int32)[mh])
    assert np.array_equal(avg.cpu().numpy().view(np.int32)[mh], want_avg.view(np.int32)[mh])
    # padding, unwritten groups, guards and inputs
    assert bool((avg[~m] == FCANARY).all()) and bool((torch.from_numpy(got_sum).to(gpu)[~m] == FCANARY).all())
    assert _guards_kept(bufs, out)
    if not in_place:
        assert torch.equal(acc.view(torch.int32), acc0.view(torch.int32))
    assert all(torch.equal(c, k) for c, k in zip([t for c in cl for t in c[:2]], keep))
    L, b = 2 ** s_out, s_out + 2
    wr = _written(plan, mask, b).to(gpu) if packed else torch.cat([m, torch.zeros(q.numel() - A, dtype=torch.bool, device=gpu)])
    assert bool((q[~wr] == (ICANARY if q.dtype == torch.int32 else 0x55)).all())
    # the norms: the bucketed encoder's bits, and close to the float64 norm of each bucket of avg
    assert torch.equal(bn.view(torch.int32), plan.qsgd_norms_bucketed(avg, d_out).view(torch.int32))
    bo, (boff, nb) = _bidx(plan, d_out), plan.bucket_layout(d_out)
    exact = np.sqrt(np.bincount(bo[mh], weights=want_avg.astype(np.float64)[mh] ** 2, minlength=nb))
    bn_h = bn.cpu().numpy()
    assert (np.abs(bn_h - exact) <= 2.0 ** -20 * exact).all()
    # the payload: the oracle's levels bucket by bucket against the kernel's norms and the Philox draws
    av, qh = torch.from_numpy(want_avg), q.cpu().numpy()
    for t, (o, n) in enumerate(zip(plan.offsets, plan.sizes)):
        u = torch.from_numpy(oracle.philox_uniforms(SEED, OFF, t, n))
        lv = np.concatenate([oracle.qsgd_quantize(av[o + j * d_out:o + min((j + 1) * d_out, n)], s_out,
                                                  norm=float(bn_h[boff[t] + j]), u=u[j * d_out:min((j + 1) * d_out, n)])[0]
                             .long().numpy() for j in range(-(-n // d_out))])
        if packed:
            assert qh.view(np.uint8)[o * b // 8:o * b // 8 + (n * b + 7) // 8].tobytes() == bitpack.pack(lv, L), t
        else:
            assert np.array_equal(qh[o:o + n].astype(np.int64), lv), t
    # the calls it replaces
    _, avg2, q2, bn2 = _the_calls(plan, acc0, cl, width, s_in, d_in, s_out, d_out, packed, start)
    assert torch.equal(avg.view(torch.int32)[m], avg2.view(torch.int32)[m])
    assert torch.equal(q[wr], q2[wr]) and torch.equal(bn.view(torch.int32), bn2.view(torch.int32))


@pytest.mark.parametrize("width,s_in,levels_in,s_out,packed,enc", (
    (8, None, 12, 4, False, "bucketed"), (0, 20, None, 4, True, "bucketed_packed"), (8, 4, None, 20, True, "bucketed_packed")))
def test_fallbacks_give_the_same_bytes(gpu, arenas, width, s_in, levels_in, s_out, packed, enc):
    d = 512
    plan, mask, acc0 = arenas[d]
    m = mask.to(gpu)
    cl = _clients(plan, gpu, 3, width, s_in if s_in is not None else 3, d)  # levels_in = 12: levels of [-8, 8] read at 12
    L_in = levels_in or 2 ** s_in
    bufs, out = _outputs(plan, gpu, s_out, d, packed)
    avg, q, bn = plan.ps_sum_encode_bucketed(acc0, [c[0] for c in cl], [c[1] for c in cl], width, L_in, d, DIV, s_out, d,
                                             pack_out=packed, sum_out=out["sum"], avg_out=out["avg"], seed=SEED, offset=OFF,
                                             q_out=out["q"], bnorm_out=out["bn"])
    assert plan.last_encoder == enc
    y = acc0.clone()
    if width == 0:
        plan.qsgd_decode_sum_bucketed_packed([c[0] for c in cl], L_in, d, [c[1] for c in cl], y_out=y, init=True)
    else:
        plan.qsgd_decode_sum_bucketed([c[0] for c in cl], width, L_in, d, [c[1] for c in cl], y_out=y, init=True)
    avg2 = codec.div_(y.clone(), DIV)
    q2, bn2 = (plan.qsgd_encode_bucketed_packed if packed else plan.qsgd_encode_bucketed)(avg2, s_out, d, seed=SEED, offset=OFF)
    wr = _written(plan, mask, s_out + 2).to(gpu) if packed else torch.cat([m, torch.zeros(q.numel() - plan.arena_end, dtype=torch.bool, device=gpu)])
    assert torch.equal(out["sum"].view(torch.int32)[m], y.view(torch.int32)[m])
    assert torch.equal(avg.view(torch.int32)[m], avg2.view(torch.int32)[m])
    assert torch.equal(q[wr], q2[wr]) and torch.equal(bn.view(torch.int32), bn2.view(torch.int32))
    assert bool((avg[~m] == FCANARY).all()) and bool((out["sum"][~m] == FCANARY).all()) and _guards_kept(bufs, out)


# case -> (what the C call gets wrong, the same mistake through the wrapper where tensors can express it)
REFUSED = {
    "bad bucket_in": (dict(bucket_in=100), lambda acc, out: dict(bucket_in=100)),
    "bad bucket_out": (dict(bucket_out=8192), lambda acc, out: dict(bucket_out=8192)),
    "no client, no acc": (dict(no_acc=True, n=0), lambda acc, out: dict(acc=None, n=0)),
    "avg_out is acc": (dict(alias="acc"), lambda acc, out: dict(avg_out=acc)),
    "avg_out is sum_out": (dict(alias="sum"), lambda acc, out: dict(sum_out=out["avg"])),
    "misaligned avg_out": (dict(shift="avg"), lambda acc, out: dict(avg_out=torch.zeros_like(acc)[1:])),
    "misaligned sum_out": (dict(shift="sum"), None), "misaligned payload": (dict(shift="q_in"), None),
    "avg_out overlaps a norm arena": (dict(alias="bn_in"), None), "avg_out overlaps a payload": (dict(alias="q_in"), None),
    "a NULL entry": (dict(null_entry=True), None), "nclients < 0": (dict(n=-1), None),
}


@pytest.mark.parametrize("case", REFUSED)
def test_refused_arguments(gpu, arenas, case):
    import ctypes

    from omnifed_amd import _lib
    d, (kw, py) = 512, REFUSED[case]
    plan, mask, acc0 = arenas[d]
    A = plan.arena_end
    cl = _clients(plan, gpu, 2, 32, 8, d)
    bufs, out = _outputs(plan, gpu, 4, d, False)
    before = {k: v.clone() for k, v in bufs.items()}
    big = torch.zeros(2 * A + 8, device=gpu)  # stands in for a norm arena or a payload that avg_out overlaps
    ptr = {"acc": acc0.data_ptr(), "sum": out["sum"].data_ptr(), "avg": out["avg"].data_ptr(),
           "q_in": [c[0].data_ptr() for c in cl], "bn_in": [c[1].data_ptr() for c in cl]}
    if kw.get("shift") in ("avg", "sum"):
        ptr[kw["shift"]] += 4
    if kw.get("shift") == "q_in":
        ptr["q_in"][1] += 4
    if kw.get("alias") in ("acc", "sum"):
        ptr["avg"] = ptr[kw["alias"]]
    if kw.get("alias") == "bn_in":
        ptr["bn_in"][1] = ptr["avg"] = big.data_ptr()
    if kw.get("alias") == "q_in":
        ptr["q_in"][0], ptr["avg"] = big.data_ptr(), big.data_ptr() + 16
    if kw.get("null_entry"):
        ptr["bn_in"][0] = None
    rc = _lib.lib().omf_ps_sum_encode_bucketed(
        plan._h, None if kw.get("no_acc") else ptr["acc"], (ctypes.c_void_p * 2)(*ptr["q_in"]),
        (ctypes.c_void_p * 2)(*ptr["bn_in"]), kw.get("n", 2), 32, 256, kw.get("bucket_in", d), ptr["sum"], DIV, ptr["avg"], 4,
        kw.get("bucket_out", d), 0, SEED, OFF, out["q"].data_ptr(), out["bn"].data_ptr(), None)
    assert rc == _lib.OMF_EINVAL, case
    if py is not None:  # raises as the sibling wrappers do
        a = dict(acc=acc0, n=2, bucket_in=d, bucket_out=d, sum_out=out["sum"], avg_out=out["avg"])
        a.update(py(acc0, out))
        with pytest.raises((ValueError, codec.CodecError)):
            plan.ps_sum_encode_bucketed(a["acc"], [c[0] for c in cl][:a["n"]], [c[1] for c in cl][:a["n"]], 32, 256, a["bucket_in"],
                                        DIV, 4, a["bucket_out"], sum_out=a["sum_out"], avg_out=a["avg_out"], q_out=out["q"],
                                        bnorm_out=out["bn"])
    torch.cuda.synchronize()
    assert all(torch.equal(bufs[k], before[k]) for k in bufs) and not bool(big.any())


@pytest.mark.parametrize("packed", (False, True))
def test_device_aggregator_routes_bucketed_rounds(gpu, packed):
    d, s = 256, 4
    shapes = {"w": (37, 129), "b": (1000,), "c": (4097,)}

    def comp(client=None):
        c = build_global_compressor(enabled=True, scheme="qsgd", bit_width=s, bucket_size=d, bucket_packed=packed, device=gpu)
        c.client_id = 77 if client is None else client
        c._instance = 0  # the Philox key's creation index: every downlink compressor below draws the same stream
        return c

    g = torch.Generator(device=gpu).manual_seed(5)
    updates = [(encode_updates_dict({k: torch.randn(sh, device=gpu, generator=g) * 1e-3 for k, sh in shapes.items()}, comp(c)), 10 + c)
               for c in range(3)]
    twin = DeviceAggregator(list(shapes.items()), device=gpu)
    twin.fuse_bucketed_step = False  # the parent's path: the sum, copy, divide, encode_updates_dict of the average
    twin.accumulate_many(updates)
    want_avg, want = twin.apply_and_encode(comp())
    assert twin.plan.last_encoder == ("bucketed_packed" if packed else "bucketed")

    def same(agg, got, stale=False):
        avg, layers = got
        assert agg.plan.last_encoder == "bucketed_ps"
        assert [L.SerializeToString() for L in layers] == [L.SerializeToString() for L in want]  # every field
        assert all(torch.equal(avg[n].view(torch.int32), want_avg[n].view(torch.int32)) for n in shapes)
        assert (agg.update_count, agg.total_samples, agg._stale) == (3, 33, stale)
        if stale:
            with pytest.raises(RuntimeError):
                agg.apply()
        else:
            assert torch.equal(agg.acc.view(torch.int32), twin.acc.view(torch.int32))

    agg = DeviceAggregator(list(shapes.items()), device=gpu)
    same(agg, agg.sum_apply_encode(updates, comp()))
    for keep_sum in (True, False):
        agg = DeviceAggregator(list(shapes.items()), device=gpu)
        agg.accumulate_many(updates[:2])
        same(agg, agg.accumulate_apply_encode(*updates[2], comp(), keep_sum=keep_sum), stale=not keep_sum)
    agg = DeviceAggregator(list(shapes.items()), device=gpu)
    agg.accumulate_many(updates)
    same(agg, agg.apply_and_encode(comp()))
