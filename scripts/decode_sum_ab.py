"""The PS's K-client aggregate, A/B in one process on the Llama-400M arena: today's sequence (zero the
accumulator, K accumulating decodes, divide) against ONE omf_qsgd_decode_sum call, at s = 4 (int8
payloads) and s = 8 (int32) for K = 2, 4, 8.

The two sides alternate: five rounds, each ten calls of one side then ten of the other, every call
between its own pair of device events; a round's figure is the median of its ten calls.  Before any
timing the two outputs are compared byte for byte at the timed size.  Per (s, K) the JSON holds both
medians (of the five round medians), each side's max - min over its round medians, the algorithmic
bytes of both ((K·w + 4)·N against 4·N + K·(w + 8)·N + 8·N) and the new call's bytes per second as a
share of the 8 TB/s HBM peak.  ``bar``: the new call's slowest round is faster than the loop's fastest.

    python scripts/decode_sum_ab.py [--out profiles/decode_sum_ab.json] [--model llama400m]
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
    ap.add_argument("--out", default="profiles/decode_sum_ab.json")
    ap.add_argument("--model", default="llama400m")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_sum_ab: no GPU visible (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    sizes = [shapes.numel(sh) for _, sh in shapes.model_shapes(args.model)]
    plan = codec.Plan(sizes, device=dev)
    N = plan.arena_end
    st = torch.cuda.current_stream(dev)
    g = torch.Generator(device=dev).manual_seed(1000)
    x = torch.randn(N, device=dev, generator=g) * 1e-3
    total = 36.0
    out = {"model": args.model, "elements": sum(sizes), "arena_elements": N, "rounds": ROUNDS, "calls": CALLS,
           "device": torch.cuda.get_device_name(dev),
           "source_digest": source_digest(), "cases": []}
    ya, yb = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(2))
    for s in (4, 8):
        levels = 2 ** s
        width = codec.storage_width(levels)
        w = width // 8
        clients = [plan.qsgd_encode(x, s, alpha=float(k + 1), seed=77, offset=k) for k in range(max(KS))]
        plan.check()
        for K in KS:
            qs, ns = [c[0] for c in clients[:K]], [c[1] for c in clients[:K]]

            def loop():
                ya.zero_()
                for q, nm in zip(qs, ns):
                    plan.qsgd_decode(q, width, levels, nm, y_out=ya, accumulate=True)
                codec.div_(ya, total)

            def one():
                plan.qsgd_decode_sum(qs, width, levels, ns, y_out=yb, divisor=total)

            loop()
            one()
            torch.cuda.synchronize()
            equal = bool(torch.equal(ya.view(torch.int32), yb.view(torch.int32)))
            case = {"s": s, "width": width, "K": K, "bytes_equal": equal,
                    "loop_bytes": 4 * N + K * (w + 8) * N + 8 * N, "sum_bytes": (K * w + 4) * N}
            out["cases"].append(case)
            if not equal:
                raise SystemExit(f"decode_sum_ab: outputs differ at s={s} K={K}; nothing timed\n{json.dumps(out)}")

            def timed(fn):
                evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
                for a, b in evs:
                    a.record(st)
                    fn()
                    b.record(st)
                torch.cuda.synchronize()
                return statistics.median(a.elapsed_time(b) for a, b in evs)  # ms

            for _ in range(WARMUP):
                loop()
                one()
            rl, ro = [], []
            for _ in range(ROUNDS):
                rl.append(timed(loop))
                ro.append(timed(one))
            ml, mo = statistics.median(rl), statistics.median(ro)
            case.update({
                "loop_ms": round(ml, 4), "sum_ms": round(mo, 4),
                "loop_rounds_ms": [round(v, 4) for v in rl], "sum_rounds_ms": [round(v, 4) for v in ro],
                "loop_spread_ms": round(max(rl) - min(rl), 4), "sum_spread_ms": round(max(ro) - min(ro), 4),
                "sum_bytes_per_s": round(case["sum_bytes"] / (mo * 1e-3), 0),
                "sum_share_of_hbm_peak": round(case["sum_bytes"] / (mo * 1e-3) / HBM_PEAK, 4),
                "speedup": round(ml / mo, 3),
                "bar": bool(max(ro) < min(rl)),
            })
            print(json.dumps(case), flush=True)
        del clients
    out["bar_everywhere"] = all(c["bar"] for c in out["cases"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "bar_everywhere": out["bar_everywhere"]}), flush=True)


if __name__ == "__main__":
    main()
