"""QSGD encode of a bf16 / fp16 model update, A/B in one process on the Llama-400M and ResNet-18 tensor
lists at s = 4: the route through an fp32 upcast arena against the 16-bit-arena encoder.

  a      gather_arena into a fresh fp32 arena (one copy kernel per tensor) + omf_qsgd_encode_ex on it
  b      the 16-bit arena + omf_qsgd_encode_h16 with 16-byte loads and the lane-pair swap
  c      the same with 8-byte loads
  b_r4, c_r4   b and c with 4 instead of 8 rows per quantise workgroup (c_r4 is the library's default)
  a_enc  omf_qsgd_encode_ex alone on an fp32 arena made beforehand (what DESIGN.md §3.5 quoted so far)

Two layouts of the 16-bit tensors: "separate" (each its own allocation: b and c gather them into a 16-bit
arena, one copy kernel per tensor as a does) and "shared" (views of one 16-bit buffer at the plan's
offsets: b and c encode it in place, a still has to upcast).

The sides alternate: five rounds, each ten calls of every side in turn, every call between its own pair
of device events; a round's figure is the median of its ten calls.  Before any timing the norms and the
payload of all sides are compared bit for bit at the timed size.  Per case the JSON holds each side's
median of round medians, its rounds and their max - min, and the counted bytes per element
(a: 2 + 4 for the upcast, 4 + 1 for the single-read encode; b, c: 2 + 2 + 1).  ``faster``: the side's
slowest round is faster than a's fastest.

    python scripts/h16_encode_ab.py [--out profiles/h16_encode_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omnifed_amd import codec, shapes  # noqa: E402
from omnifed_amd.build import source_digest  # noqa: E402
from omnifed_amd.hybrid.compression.core import gather_arena  # noqa: E402

ROUNDS, CALLS, WARMUP = 5, 10, 3
S = 4
BYTES_PER_ELEMENT = {"a": 2 + 4 + 4 + 1, "a_enc": 4 + 1, "b": 2 + 2 + 1, "c": 2 + 2 + 1, "b_r4": 2 + 2 + 1, "c_r4": 2 + 2 + 1}
H16 = {"b": (1, 8), "c": (0, 8), "b_r4": (1, 4), "c_r4": (0, 4)}  # (16-byte loads, rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/h16_encode_ab.json")
    ap.add_argument("--models", default="llama400m,resnet18")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("h16_encode_ab: no GPU visible (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    out = {"s": S, "rounds": ROUNDS, "calls": CALLS, "device": torch.cuda.get_device_name(dev),
           "source_digest": source_digest(), "bytes_per_element": BYTES_PER_ELEMENT, "cases": []}
    for model in args.models.split(","):
        sizes = [shapes.numel(sh) for _, sh in shapes.model_shapes(model)]
        plan = codec.Plan(sizes, device=dev)
        N = plan.arena_end
        for fmt, dt in ((1, torch.bfloat16), (2, torch.float16)):
            g = torch.Generator(device=dev).manual_seed(1000 + fmt)
            arena16 = (torch.randn(N, device=dev, generator=g) * 1e-3).to(dt)
            arena32 = arena16.float()
            q = {k: torch.empty(plan.payload_elems(8), dtype=torch.int8, device=dev) for k in BYTES_PER_ELEMENT}
            nrm = {k: torch.empty(plan.nt, device=dev) for k in BYTES_PER_ELEMENT}
            for layout in ("separate", "shared"):
                views = [arena16[o:o + n] for o, n in zip(plan.offsets, sizes)]
                flats = [v.clone() for v in views] if layout == "separate" else views

                def side(k):
                    if k == "a":
                        return lambda: plan.qsgd_encode(gather_arena(flats, dev, plan), S, q_out=q[k], norm_out=nrm[k],
                                                        seed=9, offset=1, value_format=fmt)
                    if k == "a_enc":
                        return lambda: plan.qsgd_encode(arena32, S, q_out=q[k], norm_out=nrm[k], seed=9, offset=1,
                                                        value_format=fmt)
                    wide, rows = H16[k]

                    def run():
                        plan.set_h16(wide, rows)
                        plan.qsgd_encode(gather_arena(flats, dev, plan, dt), S, q_out=q[k], norm_out=nrm[k], seed=9,
                                         offset=1)
                    return run

                sides = {k: side(k) for k in BYTES_PER_ELEMENT}
                for fn in sides.values():
                    fn()
                torch.cuda.synchronize()
                plan.check()
                # The 16-bit sides among themselves: every bit.  Against a: the fp32 encoders fold a norm's
                # partials over other chunk sizes than the two-pass order b and c keep, so a norm may round
                # to the neighbouring bf16 / fp16 value; the payload is compared where the norms agree.
                same = (nrm["b"].view(torch.int32) == nrm["a"].view(torch.int32)).tolist()
                equal = all(torch.equal(nrm[k].view(torch.int32), nrm["b"].view(torch.int32)) and
                            all(torch.equal(q[k][o:o + n], q["b"][o:o + n]) for o, n in zip(plan.offsets, sizes))
                            for k in H16)
                equal = equal and torch.equal(nrm["a"].view(torch.int32), nrm["a_enc"].view(torch.int32)) and all(
                    torch.equal(q["b"][o:o + n], q[k][o:o + n])
                    for k in ("a", "a_enc") for o, n, ok in zip(plan.offsets, sizes, same) if ok)
                case = {"model": model, "dtype": str(dt), "layout": layout, "elements": sum(sizes), "tensors": plan.nt,
                        "fp32_strategy": plan.strategy, "norms_equal_to_a": sum(same), "bits_equal": bool(equal)}
                out["cases"].append(case)
                if not equal:
                    raise SystemExit(f"h16_encode_ab: sides differ; nothing timed\n{json.dumps(case)}")

                def timed(fn):
                    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
                    for a, b in evs:
                        a.record(st)
                        fn()
                        b.record(st)
                    torch.cuda.synchronize()
                    return statistics.median(a.elapsed_time(b) for a, b in evs)  # ms

                for _ in range(WARMUP):
                    for fn in sides.values():
                        fn()
                torch.cuda.synchronize()
                rounds = {k: [] for k in sides}
                for _ in range(ROUNDS):
                    for k, fn in sides.items():
                        rounds[k].append(timed(fn))
                for k, r in rounds.items():
                    case[k] = {"ms": round(statistics.median(r), 4), "rounds_ms": [round(v, 4) for v in r],
                               "spread_ms": round(max(r) - min(r), 4)}
                    if k != "a":
                        case[k]["faster"] = bool(max(r) < min(rounds["a"]))
                print(json.dumps(case), flush=True)
        plan.set_h16(0, 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}), flush=True)


if __name__ == "__main__":
    main()
