"""The QSGD decode rows on the Llama-400M arena by device events, one JSON line: the plain decode of an int8
(s = 4) and an int32 (s = 8) payload, the accumulating decode of both, and the packed decode at s = 4 (6-bit
codes) and s = 8 (10-bit codes).  scripts/wire_bench.py times the int8 and packed s = 4 rows by the host clock
to 0.01 ms; this is the same calls with the resolution an A/B of two libraries needs.

Five rounds of ten calls per row, every call between its own pair of events; a row is the median of its five
round medians.

    python scripts/decode_rows.py [--model llama400m]
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

ROUNDS, CALLS, WARMUP = 5, 10, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama400m")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_rows: no GPU visible (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    sizes = [shapes.numel(sh) for _, sh in shapes.model_shapes(args.model)]
    plan = codec.Plan(sizes, device=dev)
    st = torch.cuda.current_stream(dev)
    g = torch.Generator(device=dev).manual_seed(1000)
    x = torch.randn(plan.arena_end, device=dev, generator=g) * 1e-3
    y = torch.zeros(plan.arena_end, dtype=torch.float32, device=dev)

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        rounds = []
        for _ in range(ROUNDS):
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
            for a, b in evs:
                a.record(st)
                fn()
                b.record(st)
            torch.cuda.synchronize()
            rounds.append(statistics.median(a.elapsed_time(b) for a, b in evs))
        return round(statistics.median(rounds), 4)

    res = {"model": args.model, "arena_elements": plan.arena_end, "source_digest": source_digest()}
    for s in (4, 8):
        levels = 2 ** s
        width = codec.storage_width(levels)
        q, nm = plan.qsgd_encode(x, s, seed=77)
        plan.check()
        pk = plan.qsgd_pack(q, width, levels)
        res[f"decode_int{width}_ms"] = timed(lambda: plan.qsgd_decode(q, width, levels, nm, y_out=y))
        res[f"decode_int{width}_accumulate_ms"] = timed(lambda: plan.qsgd_decode(q, width, levels, nm, y_out=y, accumulate=True))
        res[f"decode_packed_s{s}_ms"] = timed(lambda: plan.qsgd_decode_packed(pk, levels, nm, y_out=y))
        del q, pk
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
