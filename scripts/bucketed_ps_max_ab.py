"""The max-scaled bucketed PS step (omf_ps_sum_encode_bucketed_max) against the three calls it replaces, A/B in one
process on the Llama-400M tensor list at s = 4, bucket sizes d in {64, 512, 4096}, K in {1, 4, 8} clients, rotation
off and on.

  seq        omf_qsgd_decode_sum_bucketed[_rot] into the sum, omf_div_f32 in place, omf_qsgd_encode_bucketed_max of it
  fused      omf_ps_sum_encode_bucketed_max, requantise_rotated = 0: the same bytes
  fused_req  (rotation on) requantise_rotated = 1: the downlink from the rotated-domain sum, no forward transform

The arms of a cell alternate: five rounds, each ten calls of every arm in turn, every call between its own pair of
device events, after a warm-up of every arm; a round's figure is the median of its ten calls.  Per arm the JSON holds
the median of round medians, the rounds and their max - min.  Before any timing the fused step's average, payload and
scales are compared bit for bit with the sequence's.  "ahead": per rotation setting, whether the fused median is below
the sequence's by more than the larger of the two round spreads in every cell — the rule DeviceAggregator's
fuse_bucketed_max_step default follows.

    python scripts/bucketed_ps_max_ab.py [--out profiles/bucketed_ps_max_ab.json]
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
S, SIZES, CLIENTS, RS, DIV = 4, (64, 512, 4096), (1, 4, 8), 20171, 7.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/bucketed_ps_max_ab.json")
    ap.add_argument("--model", default="llama400m")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bucketed_ps_max_ab: no GPU visible (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    L = 2 ** S

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

    sizes = [shapes.numel(sh) for _, sh in shapes.model_shapes(args.model)]
    plan = codec.Plan(sizes, device=dev)
    N = plan.arena_end
    x = torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(1000)) * 1e-3
    live = torch.zeros(N, dtype=torch.bool)
    for o, n in zip(plan.offsets, plan.sizes):
        live[o:o + n] = True  # padding is not written
    live = live.to(dev)
    y, avg = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    q_out = [torch.zeros(plan.payload_elems(8), dtype=torch.int8, device=dev) for _ in range(2)]
    out = {"s": S, "rounds": ROUNDS, "calls": CALLS, "device": torch.cuda.get_device_name(dev),
           "source_digest": source_digest(), "model": args.model, "elements": sum(sizes), "tensors": plan.nt,
           "cells": {}, "ahead": {}}
    for rot in (False, True):
        ahead = True
        for d in SIZES:
            kw = dict(rotate=rot, rotation_seed=RS)
            m_out = [torch.empty(plan.bucket_layout(d)[1], device=dev) for _ in range(2)]
            pay = [plan.qsgd_encode_bucketed_max(x * (1 + 0.25 * k), S, d, seed=k, **kw) for k in range(2)]
            for K in CLIENTS:  # the same two payloads K times: the traffic of K clients
                qs, ms = [pay[k % 2][0] for k in range(K)], [pay[k % 2][1] for k in range(K)]

                def seq():
                    if rot:
                        plan.qsgd_decode_sum_bucketed_rot(qs, 8, L, d, RS, ms, y_out=y)
                    else:
                        plan.qsgd_decode_sum_bucketed(qs, 8, L, d, ms, y_out=y)
                    codec.div_(y, DIV)
                    plan.qsgd_encode_bucketed_max(y, S, d, q_out=q_out[0], bnorm_out=m_out[0], seed=9, offset=1, **kw)

                def fused(req=False):
                    plan.ps_sum_encode_bucketed_max(None, qs, ms, 8, L, d, DIV, S, requantise_rotated=req, avg_out=avg,
                                                    q_out=q_out[1], bnorm_out=m_out[1], seed=9, offset=1, **kw)

                seq(), fused()
                if not (torch.equal(y.view(torch.int32)[live], avg.view(torch.int32)[live]) and torch.equal(m_out[0], m_out[1])
                        and torch.equal(q_out[0][:N][live], q_out[1][:N][live])):
                    raise SystemExit(f"bucketed_ps_max_ab: rot={rot} d={d} K={K}: the fused bytes differ from the "
                                     "sequence's; nothing timed")
                arms = {"seq": seq, "fused": fused}
                if rot:
                    arms["fused_req"] = lambda: fused(True)
                cell = group(arms)
                margin = max(cell["seq"]["spread_ms"], cell["fused"]["spread_ms"])
                ahead = ahead and cell["fused"]["ms"] < cell["seq"]["ms"] - margin
                out["cells"][f"rot{int(rot)}_d{d}_k{K}"] = cell
                print(json.dumps({f"rot{int(rot)}_d{d}_k{K}": {k: v["ms"] for k, v in cell.items()}}), flush=True)
            del pay
        out["ahead"]["rotate" if rot else "plain"] = bool(ahead)
    out["bits_equal"] = True
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "ahead": out["ahead"]}), flush=True)


if __name__ == "__main__":
    main()
