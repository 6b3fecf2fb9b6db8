"""The bucketed PS step (omf_ps_sum_encode_bucketed) against the sequence the aggregator ran before it, A/B in one
process on the Llama-400M and ResNet-18 tensor lists: s in {4, 8}, bucket sizes d in {64, 512, 4096}, K in
{0, 1, 4, 8} clients, the int8 / int32 wire and the bit-packed wire (the same wire, s and d on both sides of the PS).

  fused    omf_ps_sum_encode_bucketed, the sum kept in the accumulator (sum_out = acc), as the aggregator calls it
  parent   omf_qsgd_decode_sum_bucketed[_packed](init) into the accumulator, avg.copy_(acc), omf_div_f32, the
           bucketed encode of avg (K = 0: without the sum)
  sum      the decode-sum alone (K > 0);  enc  the bucketed encode alone

The sides of a cell alternate: five rounds, each ten calls of every side in turn, every call between its own pair
of device events; a round's figure is the median of its ten calls.  Before any timing the fused call's average,
payload and norms are compared with the parent sequence's on the tensors' elements.  Per cell the JSON holds each
side's median of round medians, its rounds and their max - min, the counted bytes per element (w = 1 or 4 B of
levels or b / 8 of code: fused K (w + 4 / d) + 12 + w + 4 / d with K > 0, 8 + w + 4 / d with K = 0; parent
K (w + 4 / d) + 8 (K > 0) + 8 + 8 + 4 + w + 4 / d) and `ahead`: fused faster than parent by more than fused's own spread.

    python scripts/bucketed_ps_ab.py [--out profiles/bucketed_ps_ab.json]
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
SIZES, WIDTHS, CLIENTS = (64, 512, 4096), (4, 8), (0, 1, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/bucketed_ps_ab.json")
    ap.add_argument("--models", default="llama400m,resnet18")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bucketed_ps_ab: no GPU visible (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    out = {"rounds": ROUNDS, "calls": CALLS, "device": torch.cuda.get_device_name(dev),
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
        mask = torch.zeros(N, dtype=torch.bool, device=dev)
        for o, n in zip(plan.offsets, plan.sizes):
            mask[o:o + n] = True
        acc, acc2, avg, avg2 = (torch.zeros(N, device=dev) for _ in range(4))
        for s in WIDTHS:
            L, b = 2 ** s, s + 2
            width = codec.storage_width(L)
            for packed in (False, True):
                w = b / 8 if packed else width // 8
                enc = plan.qsgd_encode_bucketed_packed if packed else plan.qsgd_encode_bucketed
                for d in SIZES:
                    q_in, bn_in = enc(x, s, d, seed=9, offset=1)  # every client's payload
                    q1, n1 = enc(x, s, d, seed=9, offset=2)
                    q2, n2 = torch.empty_like(q1), torch.empty_like(n1)
                    for K in CLIENTS:
                        qs, bns = [q_in] * K, [bn_in] * K
                        div = float(max(K, 1) * 3)

                        def sum_into(y):
                            if packed:
                                plan.qsgd_decode_sum_bucketed_packed(qs, L, d, bns, y_out=y, init=True)
                            else:
                                plan.qsgd_decode_sum_bucketed(qs, width, L, d, bns, y_out=y, init=True)

                        def enc_into(a, q, nm):
                            if packed:
                                plan.qsgd_encode_bucketed_packed(a, s, d, packed_out=q, bnorm_out=nm, seed=9, offset=2)
                            else:
                                plan.qsgd_encode_bucketed(a, s, d, q_out=q, bnorm_out=nm, seed=9, offset=2)

                        def fused(a=acc, v=avg, q=q1, nm=n1):
                            plan.ps_sum_encode_bucketed(a, qs, bns, 0 if packed else width, L, d, div, s, d, pack_out=packed,
                                                        sum_out=a if K else None, avg_out=v, seed=9, offset=2, q_out=q,
                                                        bnorm_out=nm)

                        def parent(a=acc2, v=avg2, q=q2, nm=n2):
                            if K:
                                sum_into(a)
                            v.copy_(a)
                            codec.div_(v, div)
                            enc_into(v, q, nm)

                        acc.copy_(x)
                        acc2.copy_(x)
                        fused()
                        assert plan.last_encoder == "bucketed_ps"
                        parent()
                        equal = bool(torch.equal(avg.view(torch.int32)[mask], avg2.view(torch.int32)[mask])
                                     and torch.equal(acc.view(torch.int32)[mask], acc2.view(torch.int32)[mask])
                                     and torch.equal(n1.view(torch.int32), n2.view(torch.int32))
                                     and (packed or torch.equal(q1[:N][mask], q2[:N][mask])))
                        k_in = K * (w + 4 / d)
                        case = {"model": model, "s": s, "d": d, "K": K, "wire": "packed" if packed else f"int{width}",
                                "elements": sum(sizes), "bytes_equal": equal,
                                "bytes_per_element": {"fused": k_in + (12 if K else 8) + w + 4 / d,
                                                      "parent": k_in + (8 if K else 0) + 8 + 8 + 4 + w + 4 / d}}
                        out["cases"].append(case)
                        if not equal:
                            raise SystemExit(f"bucketed_ps_ab: the fused bytes differ from the parent's; nothing timed\n"
                                             f"{json.dumps(case)}")
                        sides = {"fused": fused, "parent": parent, "enc": lambda: enc_into(avg2, q2, n2)}
                        if K:
                            sides["sum"] = lambda: sum_into(acc2)
                        case["ms"] = group(sides)
                        f, p = case["ms"]["fused"], case["ms"]["parent"]
                        case["ahead"] = bool(p["ms"] - f["ms"] > f["spread_ms"])
                        print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"out": args.out, "cells": len(out["cases"]), "ahead": sum(c["ahead"] for c in out["cases"])}),
          flush=True)


if __name__ == "__main__":
    main()
