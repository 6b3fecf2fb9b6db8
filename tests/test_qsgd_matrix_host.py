"""What the QSGD oracle matrix (tests/test_gpu_qsgd_matrix.py, tests/test_gpu_qsgd_decode_matrix.py)
assumes of its own inputs and reference helpers (tests/golden/qsgd_matrix_inputs.py), checked on the
oracle alone: no GPU.
"""

import hashlib

import numpy as np
import pytest
import torch

import oracle
import qsgd_matrix_inputs as M

# SHA-256 of every input (fp32 tensors of the encoder arena, then the side inputs)
INPUT_SHA = {
    "one": "2f0d6f3d65a7e28c4223e4389106e46f1e9010a2bd724d35f9794cb8a86d7c68",
    "five": "5d048408e9ccf1984780e5e35d0d1e092748b5608b6d337b5e4bb15e3d587ade",
    "gauss": "8d72111fcd4d80ce455f3ab8dd82cbce35992fcd82b5cc7fe860de39bc6be409",
    "dominant": "65b6b32dc1ad1a708d729caedf533acedea555114ce0686f32e4c749fe6a5229",
    "heavy": "775da7b89148f89ca43a3692016f190edc93ce720d9e2757b48549e95f3b610f",
    "zero": "110b97be60a55b4ef7d0fb52768fb86609fc5f45615d0036792d639843e5f06b",
    "tiny": "987cd8afdd31d0c39d6358d500474b85accc2b80e4ff5649e606c5a5d76eeed3",
    "minus": "8a2f645174133c511da32a6b5670ef64b78f926d3bd49253f3bce3ca0b2d4e7b",
    "level0": "c46812a6b3295ba65b4573161f3cfb4d522ee503d4a532f405d26463abe6d249",
    "level1": "a8453c8d20ae197914b945729d091eeb18757bbee0131259f4675b3bacc57a98",
    "level2": "887f8f6f6bb518c21b245e519cea96134972a69b94ed7920b67d5e29b2636f26",
    "level3": "9c6e263d94b6b2f86d9b8a3d770ceda4ffa8e8ac95364fb3ca595b87fc5a4c56",
    "level4": "9d286ff6f55829f9d9a145eb4f04d6f20e76a379dc7b88a6d86de4923c2d95c4",
    "level5": "d0a8ed4ad4f0e461d7e25282158dda8b4197700d0d18b96a67a143420bc076de",
    "level6": "4e66452f8f8c419f8356093ea4f56d76d4fe025a8b21300b6943c457c4d7885f",
    "level7": "5d623ce38c4e4ccaefdfc0920796a6017ab7b1acaac51eca064d759c5d310233",
    "level8": "9a5b8ee815983a18e2712ead2a64340e22ae3f75bbc14b2bf600a4c7ecb23bff",
    "level9": "518c1f586e9531f1b04e2478f27812801ef365f09168804619a7932a8260bfc7",
    "level10": "87f2e17c10934f6acfb2d455ff24cb978e6f9391f184bd7428c58873cd9548c8",
    "level11": "26d74c00d2f7c16e3235670d88210759288ccc526b3a9421dcd403b5112b01d0",
    "level12": "12b3507316a125e9af5e9c410b8a15ca85696d6d40f805e8dd43552520dc1526",
    "u": "040988b16eff6b8115fce264fd60c86c3ba42f45e8d18cbc5e0b4691c785c2c1",
    "norm_in": "9bebe2ff4d625170d68e8eab91a84d8c7a3d58452cda6ab16de6e1754f15fca2",
    "anorm": "08edfa5895fb8cfc7ce7cbca3754444631e823c576a1889ec0a02fc365a74302",
    "q8": "c65f55e72719e4a4cafa298d289c61128836655983567e0d12de6cf36afa26e9",
    "q32": "51b7ba16e2d3cafc0c2542a4183d00e020740409782f4b24c74a28164a266ae9",
}
DEC_PAYLOAD_SHA = "0a38248d4b186fac383aaf6090035a605dd0357309331539caab38e04a3f81c8"


@pytest.fixture(scope="module", autouse=True)
def one_torch_thread():
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(old)


@pytest.fixture(scope="module")
def tensors():
    return [M.make_tensor(t) for t in range(len(M.SIZES))]


@pytest.fixture(scope="module")
def philox():
    return [torch.from_numpy(oracle.philox_uniforms(M.SEED, M.OFFSET, t, n)) for t, n in enumerate(M.SIZES)]


def test_inputs_are_pinned(tensors):
    got = {name: M.sha(x) for name, x in zip(M.NAMES, tensors)}
    got.update({k: M.sha(v) for k, v in M.make_side_inputs().items()})
    assert got == INPUT_SHA
    h = hashlib.sha256()
    for w in (8, 32):
        for lv in M.DEC_LEVELS[w]:
            h.update(M.dec_payload(w, lv, M.dec_layout()[1]).tobytes())
    assert h.hexdigest() == DEC_PAYLOAD_SHA
    x = M.make_arena()
    for t, (o, n) in enumerate(zip(M.OFFSETS, M.SIZES)):
        assert x[o:o + n].tobytes() == tensors[t].tobytes() and o % M.ALIGN == 0


def test_arena_shape(tensors):
    assert sum(M.SIZES) <= M.ARENA_END <= 120_000
    assert M.SEED >> 32 and M.OFFSET
    assert [n for n in M.SIZES if n % 4 == 0] == [] and M.SIZES[0] == 1  # a partial last quad everywhere but n = 1
    x = M.make_arena()
    assert np.signbit(x[x == 0.0]).any()
    for name in ("gauss", "dominant", "zero"):
        v = tensors[M.NAMES.index(name)]
        assert np.signbit(v[-1]) and v[-1] == 0.0, name                       # -0.0 closes the partial quad
        assert np.count_nonzero(np.signbit(v) & (v == 0.0)) >= v.size // 17, name
    assert -(-M.SIZES[M.HEAVY_T] // 16384) >= 5                                # ring chunks of 64 KiB
    d = tensors[M.NAMES.index("dominant")]
    assert np.abs(d).max() >= 0.99 * M.norm64(d)
    assert not tensors[M.ZERO_T].any()
    t = tensors[M.TINY_T]
    assert (np.square(t[t != 0]) >= np.finfo(np.float32).tiny).all()          # the fp32 squares are normal
    assert not torch.from_numpy(t).half().float().numpy().any()               # fp16: a second zero tensor
    side = M.make_side_inputs()
    assert side["q8"].min() == -128 and side["q8"].max() == 127
    assert side["q32"].min() == np.iinfo(np.int32).min and side["q32"].max() == np.iinfo(np.int32).max
    assert (np.abs(side["q32"].astype(np.int64)) > 1000).any()
    assert np.count_nonzero(side["anorm"] == 0) == 1 and side["anorm"][M.ZERO_T] == 0


@pytest.mark.parametrize("s", [0, 1, 2, 3, 4])
def test_every_level_occurs(tensors, philox, s):
    L, seen = 2 ** s, set()
    for t, v in enumerate(tensors):
        norm = float(np.float32(M.norm64(v)))
        q, *_ = oracle.qsgd_quantize(torch.from_numpy(v.copy()), s, norm=norm, u=philox[t])
        seen.update(np.unique(q.numpy()).tolist())
    assert seen == set(range(-L, L + 1)), sorted(set(range(-L, L + 1)) - seen)


def test_widest_levels(tensors, philox):
    """s = 30: +-2^30 occur, and levels above 2^24 (no fraction left: the conversion must be exact)."""
    L, seen_big, ends = 1 << 30, 0, set()
    for t, v in enumerate(tensors):
        norm = float(np.float32(M.norm64(v)))
        q, *_ = oracle.qsgd_quantize(torch.from_numpy(v.copy()), 30, norm=norm, u=philox[t])
        q = q.numpy().astype(np.int64)
        ends.update(np.unique(q[np.abs(q) == L]).tolist())
        seen_big += int(np.count_nonzero((np.abs(q) > 1 << 24) & (np.abs(q) < L)))
    assert ends == {-L, L} and seen_big > 0


@pytest.mark.parametrize("s", [16, 17, 24, 30])
def test_fp16_inf_rule(tensors, philox, s):
    """fp16 |vn| L >= 65520 is inf in the reference and gives level 0; below it the ordinary level."""
    L = 2 ** s
    for t, x in enumerate(tensors):
        v = torch.from_numpy(x.copy()).half()
        norm = torch.norm(v).item()
        q, _, width, _ = oracle.qsgd_quantize(v, s, norm=norm, u=philox[t])
        if norm == 0:
            assert width == -1 and t in (M.ZERO_T, M.TINY_T)
            continue
        q = q.numpy().astype(np.int64)
        vn = (v / norm).float().numpy().astype(np.float64)   # the fp16 quotient, exactly
        a = np.abs(vn) * L                                     # exact: 11 bits times a power of two
        inf = a >= 65520.0
        assert not q[inf].any(), (M.NAMES[t], "inf rule")
        if s == 16:
            if t == 0:                                         # the 1-element tensor: |vn| = 1
                assert inf.all()
        else:
            assert inf.any(), (M.NAMES[t], "no element reaches the inf rule")
        lo = np.floor(a[~inf])
        want = np.minimum(lo + (philox[t].numpy()[~inf].astype(np.float64) < a[~inf] - lo), L) * np.sign(vn[~inf])
        assert (q[~inf] == want.astype(np.int64)).all(), M.NAMES[t]


@pytest.mark.parametrize("fmt,dt", [("bf16", torch.bfloat16), ("fp16", torch.float16)])
def test_half_norm_interval_accepts_torch_norm(tensors, fmt, dt):
    for t, x in enumerate(tensors):
        for alpha in (1.0, 3.0) if fmt == "bf16" else (1.0,):  # the matrix weights bf16 only
            v = torch.mul(torch.from_numpy(x.copy()).to(dt), alpha)
            ref = M.norm64(v.float().numpy())
            norm = torch.norm(v).item()
            assert M.half_norm_ok(norm, ref, fmt), (M.NAMES[t], alpha, norm, M.half_norm_bounds(ref, fmt))
            lo, hi = M.half_norm_bounds(ref, fmt)
            if ref:  # the interval is a few values of the format wide at the most, and rejects a neighbour
                eps = 2.0 ** (-8 if fmt == "bf16" else -11)
                assert hi - lo <= 2 * eps * ref
                assert not M.half_norm_ok(M.round_to_format(ref * (1 + 4 * eps), fmt), ref, fmt)
                assert not M.half_norm_ok(float(np.float32(ref)) * (1 + 2.0 ** -20), ref, fmt)  # not of the format
    assert M.round_to_format(1.0 + 2.0 ** -8, "bf16") == 1.0 and M.round_to_format(1.0 + 3 * 2.0 ** -8, "bf16") == 1.0 + 2.0 ** -6
    assert M.round_to_format(1.0 + 2.0 ** -11, "fp16") == 1.0 and M.round_to_format(65520.0, "fp16") == float("inf")
    for val in (0.1, 3.14159, 57167.7, 5.58e-11, 1e-3):
        assert M.round_to_format(val, "bf16") == torch.tensor(val, dtype=torch.float64).to(torch.float32).bfloat16().item()


def test_decode_reference_equals_oracle_and_fixtures(golden, golden_index):
    """decode_ref is oracle.qsgd_dequantize's sequence, and reproduces the decoded floats of the
    reference-generated fixtures (the cases of test_gpu_qsgd.py::test_golden_cases_injected)."""
    assert golden_index["qsgd"]
    for c in golden_index["qsgd"]:
        key = f"qsgd/{c['id']}"
        q = golden[key + "/q"].reshape(-1).view(np.int8 if c["width"] == 8 else np.int32)  # stored as bytes
        want = golden[key + "/y"].reshape(-1)
        got = M.decode_ref(q, c["norm"], c["level"])
        assert got.tobytes() == want.astype(np.float32).tobytes(), key
    _, end = M.dec_layout()
    for w in (8, 32):
        for lv in M.DEC_LEVELS[w]:
            q = M.dec_payload(w, lv, end)
            assert q.min() == np.iinfo(q.dtype).min
            for norm in M.DEC_NORMS:
                want = oracle.qsgd_dequantize(torch.from_numpy(q), norm, lv, (end,)).numpy()
                got = M.decode_ref(q, norm, lv)
                nan = np.isnan(want)
                assert (np.isnan(got) == nan).all() and got[~nan].tobytes() == want[~nan].tobytes(), (w, lv, norm)
    q32 = M.dec_payload(32, 1 << 24, end)
    assert q32.max() == np.iinfo(np.int32).max and (np.abs(q32.astype(np.int64)) == (1 << 24) + 1).any()
    assert np.float32(1e-40) != 0 and np.float32((1 << 24) + 1) == np.float32(1 << 24)
