"""The bracketed pass's bits (omf_qsgd_bracket.hip qsgd_spec_quant*, qsgd_spec_finish) across a rewrite of
its instruction schedule, wave reduction and integer paths.

* Norms and payload against ``tests/golden/spec_parent_bits.npz``: ``norm_out`` (bit patterns) and
  the payload's SHA-256 as the build before the rewrite produced them on an MI355X
  (``tests/golden/make_spec_parent_bits.py`` wrote the file from ``parent_bits_cases`` below).  The
  second input spreads twelve decades, so fp64 additions of the wave partials round and a changed
  pairing tree of the wave sum changes the norm's bits.
* Payload against the oracle, as test_gpu_spec.py does, on an input in which every level -L..L,
  -0.0 and a partial last quad occur, s = 1..4.
"""

import hashlib
import os

import numpy as np
import pytest
import torch

import oracle
from omnifed_amd import codec

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SIZES = [8197, 16385, 70001, 1 << 20]
BITS = (1, 4)
ALPHAS = (1.0, 3.0)
INPUTS = ("small", "decades")
SEED, OFFSET = 29, 5


def _bracket_plan(gpu, sizes):
    plan = codec.Plan(sizes, device=gpu)
    plan.set_encode_strategy("bracket")
    return plan


def make_input(kind, n):
    """N(0,1) 1e-3, or N(0,1) 10^U(-6,6) per element (computed in fp64, rounded once to fp32)."""
    rng = np.random.default_rng(1234 if kind == "small" else 4321)
    z = rng.standard_normal(n)
    if kind == "small":
        return (z * 1e-3).astype(np.float32)
    return (z * np.power(10.0, rng.uniform(-6.0, 6.0, n))).astype(np.float32)


def parent_bits_cases(gpu):
    """{key: array} of every case: the input's SHA-256, norm_out's bit patterns, the payload's SHA-256
    (tensor ranges only: the padding between tensors is never written)."""
    plan = _bracket_plan(gpu, SIZES)
    out = {}
    for kind in INPUTS:
        x = make_input(kind, plan.arena_end)
        out[f"x_{kind}"] = np.frombuffer(hashlib.sha256(x.tobytes()).digest(), np.uint8).copy()
        xd = torch.from_numpy(x).to(gpu)
        for s in BITS:
            for alpha in ALPHAS:
                q, norms = plan.qsgd_encode(xd, s, alpha=alpha, seed=SEED, offset=OFFSET)
                assert plan.check()
                qh = q.cpu().numpy()
                h = hashlib.sha256()
                for o, n in zip(plan.offsets, plan.sizes):
                    h.update(qh[o:o + n].tobytes())
                key = f"{kind}_s{s}_a{int(alpha)}"
                out[f"norm_{key}"] = norms.cpu().numpy().view(np.uint32).copy()
                out[f"sha_{key}"] = np.frombuffer(h.digest(), np.uint8).copy()
    return out


@pytest.fixture(scope="module")
def bits(gpu):
    return parent_bits_cases(gpu)


@pytest.fixture(scope="module")
def parent():
    return np.load(GOLDEN + "/spec_parent_bits.npz")


@pytest.mark.parametrize("kind", INPUTS)
def test_inputs_are_the_fixtures(bits, parent, kind):
    assert bits[f"x_{kind}"].tobytes() == parent[f"x_{kind}"].tobytes(), "the input differs from the one recorded"


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("s", BITS)
@pytest.mark.parametrize("kind", INPUTS)
def test_norms_and_payload_equal_parent_build(bits, parent, kind, s, alpha):
    key = f"{kind}_s{s}_a{int(alpha)}"
    assert bits[f"norm_{key}"].tolist() == parent[f"norm_{key}"].tolist(), key
    assert bits[f"sha_{key}"].tobytes() == parent[f"sha_{key}"].tobytes(), key


def _level_tensor(rng, n, r, sign):
    """One element at sign r of the norm (level ceil(r L - u)), one that carries the rest of the
    norm, -0.0 and noise of 1e-5 elsewhere; the last element (in the partial last quad) is -0.0."""
    x = (rng.standard_normal(n) * 1e-5).astype(np.float32)
    x[rng.choice(n, n // 16, replace=False)] = -0.0
    p, p2 = rng.choice(n - 1, 2, replace=False)
    x[p] = sign * r
    x[p2] = -sign * np.sqrt(max(0.0, 1.0 - r * r))
    x[n - 1] = -0.0
    return x


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_payload_every_level_equals_oracle(gpu, s):
    L = 2 ** s
    rng = np.random.default_rng(50 + s)
    # tensors of at most 16 Ki elements have an exact bracket, so the pass itself decides their levels
    small = [8197, 4099, 16383, 12290, 5, 4097]
    extra, vals = [], []
    for j in range(1, L + 1):
        for sign in (1.0, -1.0):
            n = small[len(extra) % len(small)]
            assert n % 4  # a partial last quad
            extra.append(n)
            vals.append(_level_tensor(rng, n, (j - 0.01) / L, sign))
    sizes = SIZES + extra
    plan = _bracket_plan(gpu, sizes)
    x = np.zeros(plan.arena_end, np.float32)
    for t, (o, n) in enumerate(zip(plan.offsets, sizes)):
        x[o:o + n] = make_input("small", n) if t < len(SIZES) else vals[t - len(SIZES)]
    assert np.signbit(x[x == 0.0]).any()
    q, norms = plan.qsgd_encode(torch.from_numpy(x).to(gpu), s, seed=SEED + s, offset=OFFSET)
    assert plan.check()
    qh, nh = q.cpu().numpy(), norms.cpu().numpy()
    seen = set()
    for t, (o, n) in enumerate(zip(plan.offsets, sizes)):
        p = x[o:o + n]
        ref = float(np.sqrt(np.sum(p.astype(np.float64) ** 2)))
        assert nh[t] == pytest.approx(ref, rel=2e-6), (t, n)
        u = oracle.philox_uniforms(SEED + s, OFFSET, t, n)
        want, *_ = oracle.qsgd_quantize(torch.from_numpy(np.ascontiguousarray(p)), s, norm=float(nh[t]),
                                        u=torch.from_numpy(u))
        want = want.numpy()
        assert qh[o:o + n].tobytes() == want.tobytes(), (t, n, s)
        seen.update(np.unique(want).tolist())
    assert seen == set(range(-L, L + 1)), sorted(seen)
