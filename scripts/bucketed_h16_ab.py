"""Bucketed QSGD from bf16 / fp16 arenas (omf_qsgd_encode_bucketed[_packed]_h16) against the only other route to the
same bytes, A/B in one process on the Llama-400M and ResNet-18 tensor lists at s = 4, on the int8 wire and on the
bit-packed wire, bucket sizes d in {64, 512, 4096}.

  c1_{d}      the 16-bit bucketed encoder, 8-byte loads, 4 rows of 1024 elements per workgroup
  c2_{d}      8-byte loads, 8 rows per workgroup (int8 wire only: the packed back half is 4 rows)
  (c3_{d}     16-byte loads with the lane-pair swap, 4 rows: measured with this script, within the others' spread,
              and deleted from the library afterwards; its rows in the committed JSON are from that build)
  up_{d}      x16 upcast into a ready fp32 arena, then omf_qsgd_encode_bucketed[_packed] on it: timed together
  f32_{d}     that fp32 encode alone, on the ready upcast arena
  h16         omf_qsgd_encode_h16, the per-tensor 16-bit encoder (int8 wire): OTHER SEMANTICS (one norm per
              tensor, values rounded to the 16-bit format), for context only

The sides of a group alternate: five rounds, each ten
calls of every side in turn, every call between its own pair of device events, after a warm-up of every side; a
round's figure is the median of its ten calls.  Before any timing every candidate's norms and payload are compared
bit for bit with the upcast route's on the timed input.  Per case the JSON holds each side's median of round
medians, its rounds and their max - min, the counted bytes per element and c1's achieved bytes per second.

    python scripts/bucketed_h16_ab.py [--out profiles/bucketed_h16_ab.json]
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
S, SIZES = 4, (64, 512, 4096)
CANDIDATES = {"c1": 4, "c2": 8}  # rows of 1024 elements per workgroup


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/bucketed_h16_ab.json")
    ap.add_argument("--models", default="llama400m,resnet18")
    ap.add_argument("--candidates", default="c1,c2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bucketed_h16_ab: no GPU visible (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    L, b = 2 ** S, codec.packed_bits(2 ** S)
    cands = [c for c in args.candidates.split(",") if c]
    out = {"s": S, "rounds": ROUNDS, "calls": CALLS, "device": torch.cuda.get_device_name(dev),
           "source_digest": source_digest(), "candidates": cands, "cases": []}

    def timed(fn):
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
        for a, z in evs:
            a.record(st)
            fn()
            z.record(st)
        torch.cuda.synchronize()
        return statistics.median(a.elapsed_time(z) for a, z in evs)  # ms

    def group(sides):
        for _ in range(WARMUP):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in sides}
        for _ in range(ROUNDS):
            for k, fn in sides.items():
                rounds[k].append(timed(fn))
        return {k: {"ms": round(statistics.median(r), 4), "rounds_ms": [round(v, 4) for v in r],
                    "spread_ms": round(max(r) - min(r), 4)} for k, r in rounds.items()}

    for model in args.models.split(","):
        sizes = [shapes.numel(sh) for _, sh in shapes.model_shapes(model)]
        plan = codec.Plan(sizes, device=dev)
        N = plan.arena_end
        x32 = torch.empty(N, device=dev)
        nq, nw = plan.payload_elems(8), plan.packed_words(L)
        bn = {d: [torch.empty(plan.bucket_layout(d)[1], device=dev) for _ in range(2)] for d in SIZES}
        for dt in (torch.bfloat16, torch.float16):
            x16 = (torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(1000)) * 1e-3).to(dt)
            for packed in (False, True):
                bufs = [torch.zeros(nw if packed else nq, dtype=torch.int32 if packed else torch.int8, device=dev)
                        for _ in range(2)]
                okey = "packed_out" if packed else "q_out"
                mine = [c for c in cands if not (packed and c == "c2")]

                def enc(x, d, rows, which):
                    def run():
                        plan.set_bucket_rows(rows, rows == 4)
                        f = plan.qsgd_encode_bucketed_packed if packed else plan.qsgd_encode_bucketed
                        f(x, S, d, bnorm_out=bn[d][which], seed=9, offset=1, **{okey: bufs[which]})
                    return run

                def upcast(d):
                    f32 = enc(x32, d, 4, 1)

                    def run():
                        x32.copy_(x16)
                        f32()
                    return run

                equal = True
                for d in SIZES:  # every candidate against the upcast route: every bit
                    upcast(d)()
                    assert plan.last_encoder == ("bucketed_packed" if packed else "bucketed")
                    for c in mine:
                        enc(x16, d, CANDIDATES[c], 0)()
                        assert plan.last_encoder == ("bucketed_packed_h16" if packed else "bucketed_h16")
                        equal = equal and torch.equal(bufs[0], bufs[1]) and torch.equal(bn[d][0].view(torch.int32),
                                                                                       bn[d][1].view(torch.int32))
                wire_b = b / 8 if packed else 1.0
                case = {"model": model, "format": str(dt).split(".")[-1], "wire": "packed" if packed else "int8",
                        "elements": sum(sizes), "tensors": plan.nt, "bits_equal": bool(equal),
                        "bytes_per_element": {**{f"c_{d}": 2 + wire_b + 4 / d for d in SIZES},
                                              **{f"up_{d}": 2 + 4 + 4 + wire_b + 4 / d for d in SIZES},
                                              **{f"f32_{d}": 4 + wire_b + 4 / d for d in SIZES}, "h16": 5.0}}
                out["cases"].append(case)
                if not equal:
                    raise SystemExit(f"bucketed_h16_ab: the 16-bit path's bytes differ from the upcast route's; "
                                     f"nothing timed\n{json.dumps(case)}")
                sides = {}
                for d in SIZES:
                    sides.update({f"{c}_{d}": enc(x16, d, CANDIDATES[c], 0) for c in mine})
                    sides[f"up_{d}"] = upcast(d)
                    sides[f"f32_{d}"] = enc(x32, d, 4, 1)
                if not packed:
                    q0, n0 = torch.empty(nq, dtype=torch.int8, device=dev), torch.empty(plan.nt, device=dev)
                    sides["h16"] = lambda: plan.qsgd_encode(x16, S, q_out=q0, norm_out=n0, seed=9, offset=1)
                case["encode"] = group(sides)
                case["c1_gbytes_per_s"] = {d: round(case["bytes_per_element"][f"c_{d}"] * sum(sizes)
                                                    / (case["encode"][f"c1_{d}"]["ms"] * 1e6), 1) for d in SIZES}
                plan.check()
                plan.set_bucket_rows(4, True)
                print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}), flush=True)


if __name__ == "__main__":
    main()
