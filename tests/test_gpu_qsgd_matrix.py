"""Every QSGD encoder cell against the CPU oracle: strategy variant x bit width x mode on one small
arena and one plan (tests/golden/qsgd_matrix_inputs.py: tiny, odd, signed-zero, dominant, heavy-tailed,
zero and level tensors; tests/test_qsgd_matrix_host.py checks what the matrix assumes of them).

A cell is never compared with another GPU call or a recorded build.  Per cell:

* ``plan.check()`` is truthy;
* ``norm_out``: fp32 formats within NORM_RTOL of the fp64 norm of the oracle's input (x alpha in the
  tensor's dtype; the expected average for the PS modes); bf16 / fp16 a value of the format between
  round(ref (1 - 2e-6)) and round(ref (1 + 2e-6)); caller norms bit-equal to ``norm_in``;
* payload over each tensor's range byte-equal to ``oracle.qsgd_quantize`` of that input given the GPU's
  norm and the Philox (or caller) uniforms; all zero where the norm is zero;
* PS modes: the average byte-equal to numpy's fp32 ``acc / divisor``; fused last client: the sum
  ``acc + (norm q) / levels_in`` and its average likewise, ``acc`` untouched unless it is ``acc_out``;
* nothing outside a tensor's range changes in ``q_out`` (0x55 bytes; an int8 payload may zero the rest
  of a tensor's last dword), ``avg_out`` and ``acc_out`` (a canary; the inputs' padding holds it too, so
  an encoder that read padding as data would miss its norm).

The only combinations left out are the PS and last-client modes with a half format: the ABI has no
format argument there.  After the cells, the matrix's own coverage is asserted.
"""

import hashlib
from collections import Counter

import numpy as np
import pytest
import torch

import oracle
import qsgd_matrix_inputs as M
from omnifed_amd import codec

pytestmark = pytest.mark.gpu

NORM_RTOL = 2e-6  # the project's bound (tests/test_gpu_spec.py): fp32 squares, fp64 partials
CANARY = -12345.5

# (name, strategy, ring hold_max, wide levels, fused bracket)
VARIANTS = [("resident", "resident", 0, 1, 1), ("ordered", "ordered", 0, 1, 1), ("ring", "ring", 0, 1, 1),
            ("grid", "grid", 0, 1, 1), ("ring_hold1", "ring", 1, 1, 1)]
VARIANTS += [(f"bracket_w{w}_f{f}", "bracket", 0, w, f) for w in (0, 1) for f in (0, 1)]
BITS = M.BITS
# mode: (kind, value format, alpha) | ("ps", in place) | ("acc", width_in, levels_in, where the sum goes)
MODES = {
    "dev": ("enc", "fp32", 1.0), "dev_a3": ("enc", "fp32", 3.0), "u": ("enc", "fp32", 1.0),
    "norm_in": ("enc", "fp32", 1.0), "bf16": ("enc", "bf16", 1.0), "fp16": ("enc", "fp16", 1.0),
    "bf16_a3": ("enc", "bf16", 3.0), "ps": ("ps", False), "ps_inplace": ("ps", True),
    "acc8_16": ("acc", 8, 16, "other"), "acc8_10": ("acc", 8, 10, "acc"),
    "acc32_256": ("acc", 32, 256, "none"), "acc32_1000": ("acc", 32, 1000, "other"),
}
FMT = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
ENCODERS = set(codec.STRATEGIES) | {"norm_in"}

RAN = Counter()        # cells run, by last_encoder
SPEC = Counter()       # bracket cells with whole / deferred / listed > 0
CELLS = set()


@pytest.fixture(scope="module", autouse=True)
def one_torch_thread():
    """The oracle's tensors are small: torch's intra-op pool costs more than it saves."""
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(old)


class Ctx:
    """The plan, the inputs on the device and, per mode, the oracle's per-tensor input (in its dtype),
    its fp64 norm and the expected sum / average arenas.  None of it depends on the cell."""

    def __init__(self, gpu):
        self.gpu = gpu
        self.plan = plan = codec.Plan(M.SIZES, device=gpu)
        assert plan.offsets == M.OFFSETS and plan.arena_end == M.ARENA_END
        self.ranges = list(zip(M.OFFSETS, M.SIZES))
        x = M.make_arena()
        side = M.make_side_inputs()
        self.side = side
        inside = np.zeros(M.ARENA_END, bool)
        for o, n in self.ranges:
            inside[o:o + n] = True
        self.pad = ~inside
        # int8 payloads: round_up(arena_end, 4) bytes; the rest of a tensor's last dword may be zeroed
        n8 = plan.payload_elems(8)
        self.pad8 = np.ones(n8, bool)
        self.dword8 = np.zeros(n8, bool)
        for o, n in self.ranges:
            self.pad8[o:o + n] = False
            self.dword8[o + n:(o + n + 3) & ~3] = True
        self.pad8 &= ~self.dword8
        self.philox = [torch.from_numpy(oracle.philox_uniforms(M.SEED, M.OFFSET, t, n)) for t, n in enumerate(M.SIZES)]
        self.caller_u = [torch.from_numpy(side["u"][o:o + n].copy()) for o, n in self.ranges]

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)

        xc = x.copy()
        xc[self.pad] = CANARY  # padding is never read as data
        xt = torch.from_numpy(xc)
        self.x_dev = {"fp32": dev(xc), "bf16": xt.bfloat16().float().to(gpu), "fp16": xt.half().float().to(gpu)}
        self.u_dev = dev(side["u"])
        self.norm_in_dev = dev(side["norm_in"])
        self.anorm_dev = dev(side["anorm"])
        self.q_in_dev = {8: dev(side["q8"]), 32: dev(side["q32"])}
        self.acc_dev = self.x_dev["fp32"]  # the accumulator of the PS modes: the arena itself
        self.acc_host = xc
        self.mode = {}
        div = np.float32(M.DIVISOR)
        for name, spec in MODES.items():
            m = {"sum": None, "avg": None}
            if spec[0] == "enc":
                _, fmt, alpha = spec
                dt = FMT[fmt][1]
                vs = []
                for o, n in self.ranges:
                    v = torch.from_numpy(x[o:o + n].copy()).to(dt)
                    if alpha != 1.0:
                        v = torch.mul(v, alpha)  # the client weighting, in the tensor's dtype
                    vs.append(v)
            else:
                src = x
                if spec[0] == "acc":
                    _, wi, lv, _ = spec
                    sm = np.full(M.ARENA_END, CANARY, np.float32)
                    for t, (o, n) in enumerate(self.ranges):
                        y = M.decode_ref(side["q8" if wi == 8 else "q32"][o:o + n], side["anorm"][t], lv)
                        sm[o:o + n] = x[o:o + n] + y
                    m["sum"] = src = sm
                avg = np.full(M.ARENA_END, CANARY, np.float32)
                for o, n in self.ranges:
                    avg[o:o + n] = src[o:o + n] / div
                m["avg"] = avg
                vs = [torch.from_numpy(avg[o:o + n].copy()) for o, n in self.ranges]
            m["v"] = vs
            m["ref"] = [M.norm64(v.float().numpy()) for v in vs]
            self.mode[name] = m
        self.want = {}  # (mode, s, tensor, norm bits) -> digest of the oracle's payload

    def configure(self, strategy, hold, wide, fused):
        p = self.plan
        p.set_encode_strategy(strategy)
        p.set_ring(hold_max=hold)
        p.set_wide_levels(bool(wide))
        p.set_fused_bracket(bool(fused))
        if hold:
            assert p.ring_info["two_pass_tensors"] >= 1  # the large tensors take two passes

    def oracle_q(self, mode, s, t, norm, qdt):
        """The oracle's payload of tensor t (numpy, the payload's dtype)."""
        u = self.caller_u[t] if mode == "u" else self.philox[t]
        q, _, width, _ = oracle.qsgd_quantize(self.mode[mode]["v"][t], s, norm=norm, u=u)
        if width == -1:  # zero norm: the reference sends the tensor dense; the payload is all zero
            return np.zeros(M.SIZES[t], qdt)
        return q.numpy()


@pytest.fixture(scope="module")
def ctx(gpu):
    return Ctx(gpu)


def _digest(a):
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).digest()


def run_cell(c, variant, s, mode):
    """Launch one cell, then assert everything the module's docstring lists for it."""
    plan, gpu, spec = c.plan, c.gpu, MODES[mode]
    width = codec.storage_width(2 ** s)
    qdt, qnp = (torch.int8, np.int8) if width == 8 else (torch.int32, np.int32)
    q = torch.full((plan.payload_elems(width),), 0x55 if width == 8 else 0x55555555, dtype=qdt, device=gpu)
    norms = torch.full((plan.nt,), CANARY, dtype=torch.float32, device=gpu)
    kw = dict(q_out=q, norm_out=norms, seed=M.SEED, offset=M.OFFSET)
    avg = acc = acc_out = None
    if spec[0] == "enc":
        _, fmt, alpha = spec
        plan.qsgd_encode(c.x_dev[fmt], s, alpha=alpha, value_format=FMT[fmt][0],
                         u=c.u_dev if mode == "u" else None, norm_in=c.norm_in_dev if mode == "norm_in" else None, **kw)
    elif spec[0] == "ps":
        if spec[1]:
            avg = acc = c.acc_dev.clone()
        else:
            acc, avg = c.acc_dev, torch.full((M.ARENA_END,), CANARY, dtype=torch.float32, device=gpu)
        plan.ps_apply_encode(acc, M.DIVISOR, s, avg_out=avg, **kw)
    else:
        _, wi, lv, keep = spec
        acc = c.acc_dev.clone() if keep == "acc" else c.acc_dev
        acc_out = {"acc": acc, "none": None}.get(keep, torch.full((M.ARENA_END,), CANARY, dtype=torch.float32, device=gpu))
        avg = torch.full((M.ARENA_END,), CANARY, dtype=torch.float32, device=gpu)
        plan.ps_accumulate_apply_encode(acc, c.q_in_dev[wi], wi, lv, c.anorm_dev, M.DIVISOR, s, acc_out=acc_out,
                                        avg_out=avg, **kw)
    assert plan.check(), (mode, "an encoder recomputed a norm")  # a RuntimeError (timeout) fails the test here
    enc = plan.last_encoder
    assert enc in ENCODERS, enc
    RAN[enc] += 1
    if enc == "bracket":
        st = plan.spec_stats()
        for k in ("whole", "deferred", "listed"):
            SPEC[k] += st[k] > 0
    qh, nh = q.cpu().numpy(), norms.cpu().numpy()
    m = c.mode[mode]
    fmt = spec[1] if spec[0] == "enc" else "fp32"
    for t, (o, n) in enumerate(c.ranges):
        where = (mode, s, M.NAMES[t])
        ref, norm = m["ref"][t], float(nh[t])
        if mode == "norm_in":
            assert nh[t].tobytes() == c.side["norm_in"][t].tobytes(), where
        elif fmt == "fp32":
            assert abs(norm - ref) <= NORM_RTOL * ref, (where, norm, ref)
        else:
            assert M.half_norm_ok(norm, ref, fmt, NORM_RTOL), (where, norm, ref, M.half_norm_bounds(ref, fmt, NORM_RTOL))
        got = qh[o:o + n]
        if norm == 0.0:
            assert not got.any(), (where, "a zero norm needs an all-zero payload")
        key = (mode, s, t, nh[t].tobytes())
        if key not in c.want:
            c.want[key] = _digest(c.oracle_q(mode, s, t, norm, qnp))
        if _digest(got) != c.want[key]:
            want = c.oracle_q(mode, s, t, norm, qnp)
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{where} ({enc}): {bad.size} of {n} levels differ from the oracle, first at "
                                 f"{bad[:4].tolist()}: got {got[bad[:4]].tolist()}, want {want[bad[:4]].tolist()}")
    # padding of the payload
    if width == 8:
        raw = qh.view(np.uint8)
        assert (raw[c.pad8] == 0x55).all(), (mode, s, "int8 payload: padding written")
        assert np.isin(raw[c.dword8], (0x55, 0)).all(), (mode, s, "int8 payload: a tensor's last dword")
    else:
        assert (qh[c.pad] == 0x55555555).all(), (mode, s, "int32 payload: padding written")
    if avg is not None:
        ah = avg.cpu().numpy()
        assert ah.tobytes() == m["avg"].tobytes(), (mode, s, "average", _first_diff(c, ah, m["avg"]))
    if spec[0] == "ps" and not spec[1]:
        assert acc.cpu().numpy().tobytes() == c.acc_host.tobytes(), (mode, s, "acc changed")
    if spec[0] == "acc":
        keep = spec[3]
        if keep != "none":
            sh = acc_out.cpu().numpy()
            assert sh.tobytes() == m["sum"].tobytes(), (mode, s, "sum", _first_diff(c, sh, m["sum"]))
        if keep != "acc":
            assert acc.cpu().numpy().tobytes() == c.acc_host.tobytes(), (mode, s, "acc changed")
    CELLS.add((variant, s, mode))


def _first_diff(c, got, want):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    if not bad.size:
        return None
    i = int(bad[0])
    return {"n": int(bad.size), "at": i, "padding": bool(c.pad[i]), "got": float(got[i]), "want": float(want[i])}


@pytest.mark.parametrize("s", BITS)
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_cells_equal_oracle(ctx, variant, s):
    name, strategy, hold, wide, fused = variant
    ctx.configure(strategy, hold, wide, fused)
    failed = []
    for mode in MODES:
        try:
            run_cell(ctx, name, s, mode)
        except AssertionError as e:  # every failing cell of the test is named; a RuntimeError ends it at once
            failed.append(f"{name} s={s} {mode}: {str(e)[:400]}")
    assert not failed, f"{len(failed)} cells failed:\n" + "\n".join(failed)


def test_matrix_coverage(ctx):
    """Conditions on the matrix itself (the cells above must all have run in this session)."""
    missing = [(v[0], s, mode) for v in VARIANTS for s in BITS for mode in MODES if (v[0], s, mode) not in CELLS]
    assert not missing, f"{len(missing)} cells did not run (or failed), first {missing[:3]}"
    assert set(RAN) == ENCODERS, dict(RAN)
    for k in ("whole", "deferred", "listed"):
        assert SPEC[k] > 0, (k, dict(SPEC))
    print("cells per encoder:", dict(RAN), "bracket cells with whole / deferred / listed:", dict(SPEC))
