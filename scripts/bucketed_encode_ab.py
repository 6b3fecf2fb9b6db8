"""QSGD with bucket norms against the per-tensor codec, A/B in one process on the Llama-400M and ResNet-18
tensor lists at s = 4 (int8 wire, on-device draws).

  encode      enc         the plan's default per-tensor encoder (omf_qsgd_encode)
              b{d}_r{v}   omf_qsgd_encode_bucketed at bucket size d in {64, 512, 4096} with v in {4, 8, 16}
                          rows of 1024 elements per workgroup (d a kernel argument)
              b{d}_r4s    the 4-row kernel with d at compile time; the pair b{d}_r4 / b{d}_r4s is timed at
                          every allowed d (the library's per-size choice between the two comes from it)
  decode      dec         omf_qsgd_decode;          db{d}  omf_qsgd_decode_bucketed
  decode-sum  sum         omf_qsgd_decode_sum, K = 4;  sb{d}  omf_qsgd_decode_sum_bucketed, K = 4

The sides of a group alternate: five rounds, each ten calls of every side in turn, every call between its own
pair of device events; a round's figure is the median of its ten calls.  Before any timing the rows settings
of one bucket size are compared bit for bit (norms and payload).  Per case the JSON holds each side's median
of round medians, its rounds and their max - min, and the counted bytes per element (encode: 4 + 1 + 4 / d;
decode: 1 + 4 + 4 / d; sum: 4 (1 + 4 / d) + 4).

    python scripts/bucketed_encode_ab.py [--out profiles/bucketed_encode_ab.json]
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
S, K = 4, 4
SIZES, ROWS = (64, 512, 4096), (4, 8, 16)
ALL_SIZES = codec.BUCKET_SIZES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/bucketed_encode_ab.json")
    ap.add_argument("--models", default="llama400m,resnet18")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bucketed_encode_ab: no GPU visible (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    L, width = 2 ** S, 8
    out = {"s": S, "k": K, "rounds": ROUNDS, "calls": CALLS, "device": torch.cuda.get_device_name(dev),
           "source_digest": source_digest(), "cases": []}

    def timed(fn):
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
        for a, b in evs:
            a.record(st)
            fn()
            b.record(st)
        torch.cuda.synchronize()
        return statistics.median(a.elapsed_time(b) for a, b in evs)  # ms

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
        x = torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(1000)) * 1e-3
        y = torch.empty(N, device=dev)
        q0 = torch.empty(plan.payload_elems(width), dtype=torch.int8, device=dev)
        n0 = torch.empty(plan.nt, device=dev)
        qb = {d: torch.empty_like(q0) for d in ALL_SIZES}
        nb = {d: torch.empty(plan.bucket_layout(d)[1], device=dev) for d in ALL_SIZES}

        def enc_b(d, v, static=False):
            def run():
                plan.set_bucket_rows(v, static)
                plan.qsgd_encode_bucketed(x, S, d, q_out=qb[d], bnorm_out=nb[d], seed=9, offset=1)
            return run

        equal = True
        for d in ALL_SIZES:  # the variants of a bucket size: every bit
            ref = None
            for v, static in [(v, False) for v in (ROWS if d in SIZES else (4,))] + [(4, True)]:
                enc_b(d, v, static)()
                got = (qb[d].clone(), nb[d].clone())
                ref = ref or got
                equal = equal and torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))
        case = {"model": model, "elements": sum(sizes), "tensors": plan.nt, "default_strategy": plan.strategy,
                "bits_equal": bool(equal),
                "bytes_per_element": {"enc": 5.0, **{f"b{d}": 5 + 4 / d for d in SIZES}, "dec": 5.0,
                                      **{f"db{d}": 5 + 4 / d for d in SIZES}, "sum": K + 4.0,
                                      **{f"sb{d}": K * (1 + 4 / d) + 4 for d in SIZES}}}
        out["cases"].append(case)
        if not equal:
            raise SystemExit(f"bucketed_encode_ab: the rows settings differ; nothing timed\n{json.dumps(case)}")
        sides = {"enc": lambda: plan.qsgd_encode(x, S, q_out=q0, norm_out=n0, seed=9, offset=1)}
        sides.update({f"b{d}_r{v}": enc_b(d, v) for d in SIZES for v in ROWS})
        sides.update({f"b{d}_r4": enc_b(d, 4) for d in ALL_SIZES if d not in SIZES})
        sides.update({f"b{d}_r4s": enc_b(d, 4, True) for d in ALL_SIZES})
        case["encode"] = group(sides)
        plan.check()
        sides = {"dec": lambda: plan.qsgd_decode(q0, width, L, n0, y_out=y)}
        sides.update({f"db{d}": (lambda d=d: plan.qsgd_decode_bucketed(qb[d], width, L, d, nb[d], y_out=y)) for d in SIZES})
        case["decode"] = group(sides)
        sides = {"sum": lambda: plan.qsgd_decode_sum([q0] * K, width, L, [n0] * K, y_out=y, divisor=float(K))}
        sides.update({f"sb{d}": (lambda d=d: plan.qsgd_decode_sum_bucketed([qb[d]] * K, width, L, d, [nb[d]] * K, y_out=y,
                                                                          divisor=float(K))) for d in SIZES})
        case["decode_sum"] = group(sides)
        plan.set_bucket_rows(4, True)
        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}), flush=True)


if __name__ == "__main__":
    main()
