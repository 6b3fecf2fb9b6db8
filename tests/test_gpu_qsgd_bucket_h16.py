"""Bucketed QSGD from bf16 / fp16 arenas (omf_qsgd_*_bucketed*_h16): the norm bits and payload bytes are the fp32
bucketed encoders' on the exact upcast of the arena, the levels the CPU oracle's bucket by bucket, and the public
path encodes 16-bit tensors in place.

One plan per bucket size d with the fp32 test's tensor sizes — the odd ones end in a dword with one element and a
quad with 1-3 — an all-zero bucket, a bucket with one non-zero element, a bucket of fp16 subnormals, the format's
NaN in the padding (a padding element that reaches a sum makes the norm NaN) and canaries around the outputs."""

import numpy as np
import pytest
import torch

import oracle
from omnifed_amd import codec
from omnifed_amd.hybrid.communicator.global_grpc_compression import (build_global_compressor, decode_updates_dict,
                                                                     encode_updates_dict)
from omnifed_amd.hybrid.compression.qsgd import encode_bucketed

pytestmark = pytest.mark.gpu

SIZES = codec.BUCKET_SIZES
FORMATS = (torch.bfloat16, torch.float16)
SEED, OFF, GUARD = 0xB16, 3, 64


@pytest.fixture(scope="module")
def arenas(gpu):
    """(dtype, d) -> (plan, x16, mask, words): the NaN-padded 16-bit arena, the mask of its tensors' elements and
    the mask of the 6-bit packed arena's words whose 32-element group holds a tensor element."""
    out = {}
    for d in SIZES:
        sizes = [1, 3, d - 1, d, d + 1, 2 * d + 5, 4095, 4096, 4096 + d + 1, 16384 - 1, 16384 + d // 2 + 3]
        plan = codec.Plan(sizes, device=gpu)
        mask = torch.zeros(-(-plan.arena_end // 32) * 32, dtype=torch.bool, device=gpu)
        for o, n in zip(plan.offsets, sizes):
            mask[o:o + n] = True
        words = mask.view(-1, 32).any(dim=1).repeat_interleave(6)
        for dt in FORMATS:
            g = torch.Generator(device=gpu).manual_seed(d)
            x = torch.full((plan.arena_end,), float("nan"), dtype=dt, device=gpu)
            for o, n in zip(plan.offsets, sizes):
                x[o:o + n] = (torch.randn(n, device=gpu, generator=g) * 1e-3).to(dt)
            o = plan.offsets[5]  # 2 d + 5 elements: bucket 0 all zero, bucket 1 one non-zero element
            x[o:o + 2 * d] = 0.0
            x[o + d + 7] = -2.5e-3
            if dt is torch.float16:  # bucket 1 of the 4096 + d + 1 elements: subnormal patterns of either sign
                pat = (torch.arange(d, device=gpu) % 1023 + 1 + 0x8000 * (torch.arange(d, device=gpu) % 3 == 0))
                x[plan.offsets[8] + d:plan.offsets[8] + 2 * d] = pat.to(torch.int16).view(torch.float16)
            out[dt, d] = (plan, x, mask[:plan.arena_end], words)
    return out


CASES = [(wire, draws, alpha) for wire in ("int8", "int32", "packed") for draws in ("philox", "u") for alpha in (1.0, 3.0)]
CASES.append(("int8", "bnorm_in", 1.0))


@pytest.mark.parametrize("wire,draws,alpha", CASES)
@pytest.mark.parametrize("d", SIZES)
@pytest.mark.parametrize("dt", FORMATS)
def test_bits_equal_the_fp32_path_on_the_exact_upcast(gpu, arenas, dt, d, wire, draws, alpha):
    plan, x16, mask, words = arenas[dt, d]
    x32, before = x16.float(), x16.clone()
    packed, s = wire == "packed", 8 if wire == "int32" else 4
    _, nb = plan.bucket_layout(d)
    kw = {"alpha": alpha, "seed": SEED, "offset": OFF}
    if draws == "u":
        kw["u"] = torch.rand(plan.arena_end, device=gpu, generator=torch.Generator(device=gpu).manual_seed(7))
    if draws == "bnorm_in":
        kw["bnorm_in"] = plan.qsgd_norms_bucketed(x32, d, alpha=alpha) * 1.25
    enc = plan.qsgd_encode_bucketed_packed if packed else plan.qsgd_encode_bucketed
    n_out = plan.packed_words(2 ** s) if packed else plan.payload_elems(codec.storage_width(2 ** s))
    obuf = torch.full((n_out + 2 * GUARD,), 0x55, dtype=torch.int8 if wire == "int8" else torch.int32, device=gpu)
    nbuf = torch.full((nb + 2 * GUARD,), -7.0, device=gpu)
    got, bn = enc(x16, s, d, bnorm_out=nbuf[GUARD:GUARD + nb],
                  **{"packed_out" if packed else "q_out": obuf[GUARD:GUARD + n_out]}, **kw)
    assert plan.last_encoder == ("bucketed_packed_h16" if packed else "bucketed_h16")
    want, want_bn = enc(x32, s, d, **kw)
    assert plan.last_encoder == ("bucketed_packed" if packed else "bucketed")
    # the norms: the fp32 path's bits (or the caller's), and the norms-only call's
    assert not bool(bn.isnan().any())
    assert torch.equal(bn.view(torch.int32), want_bn.view(torch.int32))
    if draws == "bnorm_in":
        assert torch.equal(bn.view(torch.int32), kw["bnorm_in"].view(torch.int32))
    else:
        for x in (x32, x16):
            assert torch.equal(plan.qsgd_norms_bucketed(x, d, alpha=alpha).view(torch.int32), bn.view(torch.int32))
    # the payload: equal where it is written, untouched elsewhere; guards and the arena untouched
    wr = words if packed else torch.cat([mask, torch.zeros(n_out - plan.arena_end, dtype=torch.bool, device=gpu)])
    assert torch.equal(got[wr], want[wr])
    assert bool((got[~wr] == 0x55).all())
    assert bool((obuf[:GUARD] == 0x55).all()) and bool((obuf[GUARD + n_out:] == 0x55).all())
    assert bool((nbuf[:GUARD] == -7.0).all()) and bool((nbuf[GUARD + nb:] == -7.0).all())
    assert torch.equal(x16.view(torch.int16), before.view(torch.int16))


@pytest.mark.parametrize("d", SIZES)
@pytest.mark.parametrize("dt", FORMATS)
def test_levels_and_decode_equal_the_oracle_per_bucket(gpu, arenas, dt, d):
    """The norm bound is the fp32 test's: any fp32 summation order of d non-negative squares has relative error
    <= d 2^-24, the square root halves it and rounds once more: (d + 4) 2^-25."""
    plan, x16, _, _ = arenas[dt, d]
    s, L, alpha = 4, 16, 3.0
    boff, _ = plan.bucket_layout(d)
    q, bn = plan.qsgd_encode_bucketed(x16, s, d, alpha=alpha, seed=SEED, offset=OFF)
    y = plan.qsgd_decode_bucketed(q, 8, L, d, bn).cpu()
    xs = x16.cpu().float() * torch.tensor(alpha, dtype=torch.float32)  # fl32(alpha float(x16))
    bn_h, q_h = bn.cpu(), q.cpu()
    for t, (o, n) in enumerate(zip(plan.offsets, plan.sizes)):
        u = torch.from_numpy(oracle.philox_uniforms(SEED, OFF, t, n))
        for j in range(-(-n // d)):
            lo, hi = o + j * d, o + min((j + 1) * d, n)
            v, norm = xs[lo:hi], float(bn_h[boff[t] + j])
            exact = float(np.sqrt(np.sum(v.double().numpy() ** 2)))
            assert abs(norm - exact) <= (d + 4) * 2.0 ** -25 * exact, (t, j, norm, exact)
            want, *_ = oracle.qsgd_quantize(v, s, norm=norm, u=u[lo - o:hi - o])
            assert torch.equal(q_h[lo:hi].long(), want.long()), (t, j)
            dec = oracle.qsgd_dequantize(want, norm, L, v.shape)
            assert torch.equal(y[lo:hi].view(torch.int32), dec.float().view(torch.int32)), (t, j)


@pytest.mark.parametrize("d", SIZES)
@pytest.mark.parametrize("dt", FORMATS)
def test_eight_rows_give_the_default_bits(gpu, arenas, dt, d):
    plan, x16, mask, _ = arenas[dt, d]
    q, bn = plan.qsgd_encode_bucketed(x16, 4, d, alpha=3.0, seed=SEED, offset=OFF)
    try:
        plan.set_bucket_rows(8)
        q2, bn2 = plan.qsgd_encode_bucketed(x16, 4, d, alpha=3.0, seed=SEED, offset=OFF)
    finally:
        plan.set_bucket_rows(4)
    assert torch.equal(bn.view(torch.int32), bn2.view(torch.int32))
    assert torch.equal(q[:plan.arena_end][mask], q2[:plan.arena_end][mask])


@pytest.mark.parametrize("kind", ("bf16_views", "fp16_separate", "mixed"))
@pytest.mark.parametrize("packed", (False, True))
@pytest.mark.parametrize("d", (64, 1024))
def test_public_path_encodes_16_bit_tensors_as_their_upcast(gpu, d, packed, kind):
    """Every layer equals the one the same compressor makes, at the same call index, of the upcast dict.  The draws
    of a dtype group are keyed by the group's index and the tensor's index in the group, so the second group of
    the mixed dict is held to ``encode_bucketed`` of its upcast members at that group's key instead."""
    shapes = {"a": (37, 29), "b": (300,), "c": (5, 411), "e": (1500,)}
    numel = {k: int(np.prod(sh)) for k, sh in shapes.items()}
    g = torch.Generator(device=gpu).manual_seed(5)
    if kind == "bf16_views":  # views of one flat buffer at the plan's offsets: encoded in place
        offs, end = codec.arena_layout(list(numel.values()))
        flat = (torch.randn(end, device=gpu, generator=g) * 1e-3).to(torch.bfloat16)
        upd = {k: flat[o:o + numel[k]].view(shapes[k]) for k, o in zip(shapes, offs)}
    else:
        dts = (torch.float32, torch.float32, torch.bfloat16, torch.bfloat16) if kind == "mixed" else (torch.float16,) * 4
        upd = {k: (torch.randn(shapes[k], device=gpu, generator=g) * 1e-3).to(dt) for k, dt in zip(shapes, dts)}
    up32 = {k: v.float() for k, v in upd.items()}
    comp = build_global_compressor(enabled=True, scheme="qsgd", bit_width=4, bucket_size=d, bucket_packed=packed,
                                   device=gpu)
    layers = encode_updates_dict(upd, comp)
    comp._calls = 0  # the same call index again
    ref = encode_updates_dict(up32, comp)
    second = [k for k in upd if kind == "mixed" and upd[k].dtype != torch.float32]
    for L, R in zip(layers, ref):
        assert (L.layer_name, L.compression_type, L.meta_tensor) == (R.layer_name, R.compression_type, R.meta_tensor)
        assert L.compression_type and (L.layer_name in second or L.values_data == R.values_data)
    if second:
        (plan, q, _, _), = encode_bucketed([up32[k].reshape(-1) for k in second], 4, d, gpu, 0,
                                           key=comp.philox_key() + 1, packed=packed)
        raw, b = q.cpu().numpy().view(np.uint8), (6 if packed else 8)
        for k, o in zip(second, plan.offsets):
            L = layers[list(upd).index(k)]
            assert L.values_data == raw[o * b // 8:o * b // 8 + (numel[k] * b + 7) // 8].tobytes(), k
    dec = decode_updates_dict(layers, device=gpu)
    for L in layers:
        bound = float(np.frombuffer(L.meta_tensor, dtype=np.float32).max()) / 16
        assert float((dec[L.layer_name].float() - up32[L.layer_name]).abs().max()) <= bound, L.layer_name
