"""The PS's K-client aggregate of PACKED payloads (the opt-in bit-packed QSGD wire), A/B in one process on
the Llama-400M arena, at s = 4 (6-bit codes) and s = 8 (10-bit codes) for K = 2, 4, 8:

  (a) loop      the sequence available before omf_qsgd_decode_sum_packed: zero the accumulator, K
                accumulating packed decodes (omf_qsgd_decode_packed), divide;
  (b) packed    ONE omf_qsgd_decode_sum_packed call;
  (c) unpacked  for information: ONE omf_qsgd_decode_sum call on the same levels unpacked (int8 / int32).

The method is scripts/decode_sum_ab.py's.  The sides alternate: five rounds, each ten calls of one side,
then of the next, every call between its own pair of device events; a round's figure is the median of its
ten calls.  Before any timing the three outputs are compared byte for byte at the timed size.  Per (s, K)
the JSON holds each side's median (of the five round medians), its round medians and their max - min, and
the algorithmic bytes per element each side moves: (a) 4 + K·(b/8 + 8) + 8, (b) K·b/8 + 4, (c) K·w + 4.
``bar``: the packed call's slowest round is faster than the loop's fastest.  Against (c) there is no bar.

    python scripts/decode_sum_packed_ab.py [--out profiles/decode_sum_packed_ab.json] [--model llama400m]
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

HBM_PEAK = 8.0e12  # bytes per second (MI355X HBM3E, datasheet)
ROUNDS, CALLS, WARMUP = 5, 10, 3
KS = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/decode_sum_packed_ab.json")
    ap.add_argument("--model", default="llama400m")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_sum_packed_ab: no GPU visible (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    sizes = [shapes.numel(sh) for _, sh in shapes.model_shapes(args.model)]
    plan = codec.Plan(sizes, device=dev)
    N = plan.arena_end
    st = torch.cuda.current_stream(dev)
    g = torch.Generator(device=dev).manual_seed(1000)
    x = torch.randn(N, device=dev, generator=g) * 1e-3
    total = 36.0
    out = {"model": args.model, "elements": sum(sizes), "arena_elements": N, "rounds": ROUNDS, "calls": CALLS,
           "device": torch.cuda.get_device_name(dev), "source_digest": source_digest(), "cases": []}
    ya, yb, yc = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(3))
    for s in (4, 8):
        levels = 2 ** s
        width = codec.storage_width(levels)
        w = width // 8
        bits = codec.packed_bits(levels)
        clients = [plan.qsgd_encode(x, s, alpha=float(k + 1), seed=77, offset=k) for k in range(max(KS))]
        plan.check()
        packed = [plan.qsgd_pack(q, width, levels) for q, _ in clients]
        for K in KS:
            qs, ns, ps = [c[0] for c in clients[:K]], [c[1] for c in clients[:K]], packed[:K]

            def loop():
                ya.zero_()
                for p, nm in zip(ps, ns):
                    plan.qsgd_decode_packed(p, levels, nm, y_out=ya, accumulate=True)
                codec.div_(ya, total)

            def one():
                plan.qsgd_decode_sum_packed(ps, levels, ns, y_out=yb, divisor=total)

            def unpacked():
                plan.qsgd_decode_sum(qs, width, levels, ns, y_out=yc, divisor=total)

            sides = (("loop", loop), ("packed", one), ("unpacked", unpacked))
            for _, fn in sides:
                fn()
            torch.cuda.synchronize()
            equal = bool(torch.equal(ya.view(torch.int32), yb.view(torch.int32))
                         and torch.equal(yc.view(torch.int32), yb.view(torch.int32)))
            case = {"s": s, "bits": bits, "width": width, "K": K, "bytes_equal": equal,
                    "bytes_per_element": {"loop": 4 + K * (bits / 8 + 8) + 8, "packed": K * bits / 8 + 4,
                                          "unpacked": K * w + 4}}
            out["cases"].append(case)
            if not equal:
                raise SystemExit(f"decode_sum_packed_ab: outputs differ at s={s} K={K}; nothing timed\n{json.dumps(out)}")

            def timed(fn):
                evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
                for a, b in evs:
                    a.record(st)
                    fn()
                    b.record(st)
                torch.cuda.synchronize()
                return statistics.median(a.elapsed_time(b) for a, b in evs)  # ms

            for _ in range(WARMUP):
                for _, fn in sides:
                    fn()
            rounds = {name: [] for name, _ in sides}
            for _ in range(ROUNDS):
                for name, fn in sides:
                    rounds[name].append(timed(fn))
            med = {name: statistics.median(v) for name, v in rounds.items()}
            for name, v in rounds.items():
                case[f"{name}_ms"] = round(med[name], 4)
                case[f"{name}_rounds_ms"] = [round(t, 4) for t in v]
                case[f"{name}_spread_ms"] = round(max(v) - min(v), 4)
            packed_bytes = case["bytes_per_element"]["packed"] * N
            case.update({
                "packed_bytes_per_s": round(packed_bytes / (med["packed"] * 1e-3), 0),
                "packed_share_of_hbm_peak": round(packed_bytes / (med["packed"] * 1e-3) / HBM_PEAK, 4),
                "speedup_over_loop": round(med["loop"] / med["packed"], 3),
                "packed_over_unpacked": round(med["packed"] / med["unpacked"], 3),
                "bar": bool(max(rounds["packed"]) < min(rounds["loop"])),
            })
            print(json.dumps(case), flush=True)
        del clients, packed
    out["bar_everywhere"] = all(c["bar"] for c in out["cases"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "bar_everywhere": out["bar_everywhere"]}), flush=True)


if __name__ == "__main__":
    main()
