"""QSGD encode of bf16 / fp16 tensors from an arena of their own dtype (omf_qsgd_encode_h16): no fp32
upcast.  One plan per dtype with tensors at the sizes the 16-bit loads can get wrong (1-3 elements of
a quad, half a dword, one less / exactly / one more than an encode item, several items with a partial
last quad), canaries in the arena's padding and around the outputs.  Every case is held to a float64
norm, to the CPU oracle given that norm, and bit for bit to the encode of the fp32 upcast."""

import numpy as np
import pytest
import torch

import oracle
from omnifed_amd import codec
from omnifed_amd.hybrid.communicator.global_grpc_compression import encode_updates_dict
from omnifed_amd.hybrid.compression.qsgd import QSGDQuantCompression

pytestmark = pytest.mark.gpu

DTYPES = {1: torch.bfloat16, 2: torch.float16}
NORM_TOL = {1: 2.0 ** -7, 2: 2.0 ** -10}  # half an ulp of the format plus fp32 accumulation
SEED, OFF = 0x516, 5
GUARD = 64


@pytest.fixture(scope="module")
def arenas(gpu):
    """fmt -> (plan, x16, mask): the canary-padded 16-bit arena and the mask of its tensors' elements."""
    item = codec.Plan([1], device=gpu).ring_info["chunk"]
    out = {}
    for fmt, dt in DTYPES.items():
        sizes = [1, 2, 3, 5, 63, 64, 65, 4099, item - 1, item, item + 1, 3 * item + item // 2 + 3]
        if fmt == 2:
            sizes.append(70001)  # |v| ~ 300: the fp16 norm overflows to inf
        plan = codec.Plan(sizes, device=gpu)
        g = torch.Generator(device=gpu).manual_seed(40 + fmt)
        x = torch.full((plan.arena_end,), 3e4, device=gpu).to(dt)
        mask = torch.zeros(plan.arena_end, dtype=torch.bool, device=gpu)
        for o, n in zip(plan.offsets, sizes):
            x[o:o + n] = (torch.randn(n, device=gpu, generator=g) * 1e-3).to(dt)
            mask[o:o + n] = True
        if fmt == 2:
            x[plan.offsets[-1]:] = (torch.randn(70001, device=gpu, generator=g).sign() * 300).to(dt)
        out[fmt] = (plan, x, mask)
    return out


CASES = [(fmt, s, alpha, draws) for fmt in (1, 2) for s, alpha in ((4, 1.0), (3, 3.0), (8, 1.0))
         for draws in ("philox", "u")] + [(1, 4, 1.0, "norm_in")]


@pytest.mark.parametrize("fmt,s,alpha,draws", CASES)
def test_h16_encode_equals_oracle_and_upcast_path(gpu, arenas, fmt, s, alpha, draws):
    dt = DTYPES[fmt]
    plan, x, mask = arenas[fmt]
    x_before = x.clone()
    L, width = 2 ** s, codec.storage_width(2 ** s)
    kw = {"alpha": alpha, "seed": SEED, "offset": OFF}
    if draws == "u":
        kw["u"] = torch.rand(plan.arena_end, device=gpu, generator=torch.Generator(device=gpu).manual_seed(7))
    if draws == "norm_in":
        kw["norm_in"] = plan.qsgd_norms(x, alpha=alpha) * 1.25
    np_q = plan.payload_elems(width)
    qbuf = torch.full((np_q + GUARD,), 0x55, dtype=torch.int8 if width == 8 else torch.int32, device=gpu)
    nbuf = torch.full((plan.nt + GUARD,), -7.0, device=gpu)
    q, norms = plan.qsgd_encode(x, s, q_out=qbuf[:np_q], norm_out=nbuf[:plan.nt], **kw)
    assert plan.last_encoder == "h16"
    assert plan.check()
    # nothing outside the tensors is written, the arena is only read
    assert bool((qbuf[:plan.arena_end][~mask] == 0x55).all()) and bool((qbuf[plan.arena_end:] == 0x55).all())
    assert bool((nbuf[plan.nt:] == -7.0).all())
    assert torch.equal(x.view(torch.int16), x_before.view(torch.int16))
    # the one-payload invariant: the encode of the exact fp32 upcast, bit for bit
    q2, norms2 = plan.qsgd_encode(x.float(), s, value_format=fmt, **kw)
    assert plan.last_encoder != "h16"
    assert torch.equal(norms.view(torch.int32), norms2.view(torch.int32))
    assert torch.equal(q[:plan.arena_end][mask], q2[:plan.arena_end][mask])
    if draws != "norm_in":
        assert torch.equal(plan.qsgd_norms(x, alpha=alpha).view(torch.int32), norms.view(torch.int32))
    try:  # the 16-byte loads with the lane-pair swap, 8 rows per workgroup: the same bits
        plan.set_h16(wide_loads=1, rows=8)
        q3, norms3 = plan.qsgd_encode(x, s, **kw)
    finally:
        plan.set_h16(wide_loads=0, rows=4)
    assert torch.equal(norms3.view(torch.int32), norms.view(torch.int32))
    assert torch.equal(q3[:plan.arena_end][mask], q[:plan.arena_end][mask])
    y = plan.qsgd_decode(q, width, L, norms)
    xh, qh, yh, nh = x.cpu(), q.cpu().numpy(), y.cpu().numpy(), norms.cpu().numpy()
    for t, (o, n) in enumerate(zip(plan.offsets, plan.sizes)):
        v = xh[o:o + n] if alpha == 1.0 else torch.mul(xh[o:o + n], alpha)  # the weighting in the tensor's dtype
        if draws == "norm_in":
            assert nh[t] == float(kw["norm_in"][t])
        else:
            ref = float(torch.norm(v.double()))
            print(f"tensor {t} n={n}: norm {nh[t]!r} ref {ref!r}")
            if fmt == 2 and ref > 65504:
                assert np.isinf(nh[t]), (t, nh[t], ref)
            else:
                assert abs(float(nh[t]) - ref) <= NORM_TOL[fmt] * ref, (t, nh[t], ref)
                assert float(torch.tensor(float(nh[t])).to(dt)) == float(nh[t]), (t, nh[t])
        u = kw["u"][o:o + n].cpu() if draws == "u" else torch.from_numpy(oracle.philox_uniforms(SEED, OFF, t, n))
        want, _, _, _ = oracle.qsgd_quantize(v, s, norm=float(nh[t]), u=u)
        assert qh[o:o + n].tobytes() == want.numpy().tobytes(), (t, n)
        want_y = oracle.qsgd_dequantize(want, float(nh[t]), L, (n,)).numpy()
        assert np.array_equal(yh[o:o + n], want_y, equal_nan=True), (t, n)  # an inf norm decodes to NaN


@pytest.mark.parametrize("fmt", [1, 2])
def test_tensors_off_16_byte_boundaries_take_8_byte_loads(gpu, fmt):
    """Offsets that are multiples of 4 but not of 8 elements: a request for 16-byte loads is served by the
    8-byte ones, the same bits."""
    sizes, offsets = [5, 4099, 40003], [4, 12, 4116]
    plan = codec.Plan(sizes, offsets, device=gpu)
    plan.set_h16(wide_loads=1)
    x = torch.full((plan.arena_end,), 3e4, device=gpu).to(DTYPES[fmt])
    g = torch.Generator(device=gpu).manual_seed(fmt)
    for o, n in zip(offsets, sizes):
        x[o:o + n] = (torch.randn(n, device=gpu, generator=g) * 1e-3).to(DTYPES[fmt])
    q, norms = plan.qsgd_encode(x, 4, alpha=3.0, seed=SEED, offset=OFF)
    assert plan.last_encoder == "h16"
    q2, norms2 = plan.qsgd_encode(x.float(), 4, alpha=3.0, seed=SEED, offset=OFF, value_format=fmt)
    assert torch.equal(norms.view(torch.int32), norms2.view(torch.int32))
    for o, n in zip(offsets, sizes):
        assert torch.equal(q[o:o + n], q2[o:o + n]), (o, n)


def test_contradicting_value_format_is_refused(gpu, arenas):
    plan, x, _ = arenas[1]
    with pytest.raises(ValueError, match="value_format"):
        plan.qsgd_encode(x, 4, value_format=2)


def test_plugin_encodes_a_bf16_dict_from_its_16_bit_arena(gpu):
    """Tensors that are views of one flat bf16 buffer at the plan's offsets (a flat parameter buffer): the
    route that takes the 16-bit arena at every size (separate tensors do from 2^25 elements on)."""
    shapes = {"w": (300, 70), "b": (70,), "e": (33000,)}
    offsets, end = codec.arena_layout([int(np.prod(sh)) for sh in shapes.values()])
    g = torch.Generator(device=gpu).manual_seed(3)
    buf = (torch.randn(end, device=gpu, generator=g) * 1e-3).bfloat16()
    upd = {name: buf[o:o + int(np.prod(sh))].view(sh) for (name, sh), o in zip(shapes.items(), offsets)}
    comp = QSGDQuantCompression(bit_width=4, device=gpu)
    key, call = comp.philox_key(), comp._calls
    layers = encode_updates_dict(upd, comp)
    assert codec.Plan.get([t.numel() for t in upd.values()], device=gpu).last_encoder == "h16"
    for t, (layer, (name, x)) in enumerate(zip(layers, upd.items())):
        norm = float(np.frombuffer(layer.meta_tensor, dtype=np.float32)[0])
        ref = float(torch.norm(x.double()))
        assert abs(norm - ref) <= NORM_TOL[1] * ref, (name, norm, ref)
        u = torch.from_numpy(oracle.philox_uniforms(key, call, t, x.numel()))
        want, _, _, _ = oracle.qsgd_quantize(x.reshape(-1).cpu(), 4, norm=norm, u=u)
        assert layer.layer_name == name and layer.values_data == want.numpy().tobytes(), name
