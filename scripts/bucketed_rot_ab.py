"""Max-scaled bucketed QSGD and its Hadamard rotation (omf_qsgd_encode_bucketed_max, omf_qsgd_decode_sum_bucketed_rot)
against the L2 bucketed kernels they stand beside, A/B in one process on the Llama-400M tensor list at s = 4, bucket
sizes d in {64, 512, 4096}.

  encode      l2_{d}   omf_qsgd_encode_bucketed (unchanged)
              max_{d}  omf_qsgd_encode_bucketed_max, rotate = 0
              rot_{d}  omf_qsgd_encode_bucketed_max, rotate = 1
  decode-sum  l2_{d}_k{K}   omf_qsgd_decode_sum_bucketed over K clients' payloads
              rot_{d}_k{K}  omf_qsgd_decode_sum_bucketed_rot over the same buffers (K = 1, 4, 8)

The sides of a group alternate: five rounds, each ten calls of every side in turn, every call between its own pair of
device events, after a warm-up of every side; a round's figure is the median of its ten calls.  Per side the JSON
holds the median of round medians, the rounds and their max - min.  Before any timing the max encoder's payload is
compared bit for bit with omf_qsgd_encode_bucketed's on the rotated arena with the max encoder's scales.

    python scripts/bucketed_rot_ab.py [--out profiles/bucketed_rot_ab.json]
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
S, SIZES, CLIENTS, RS = 4, (64, 512, 4096), (1, 4, 8), 20171


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/bucketed_rot_ab.json")
    ap.add_argument("--model", default="llama400m")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bucketed_rot_ab: no GPU visible (there is no CPU fallback)")
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
    q = [torch.zeros(plan.payload_elems(8), dtype=torch.int8, device=dev) for _ in range(2)]
    bn = {d: [torch.empty(plan.bucket_layout(d)[1], device=dev) for _ in range(2)] for d in SIZES}
    y = torch.empty(N, device=dev)
    live = torch.zeros(N, dtype=torch.bool)
    for o, n in zip(plan.offsets, plan.sizes):
        live[o:o + n] = True  # the payload's padding is not written
    live = live.to(dev)
    equal = True
    for d in SIZES:  # the fused encoder against the existing one on the rotated arena: every payload byte
        plan.qsgd_encode_bucketed_max(x, S, d, rotate=True, rotation_seed=RS, q_out=q[0], bnorm_out=bn[d][0], seed=9, offset=1)
        z = plan.qsgd_rotate_bucketed(x, d, RS)
        plan.qsgd_encode_bucketed(z, S, d, q_out=q[1], bnorm_out=bn[d][1], seed=9, offset=1, bnorm_in=bn[d][0])
        equal = equal and torch.equal(q[0][:N][live], q[1][:N][live])
        del z
    out = {"s": S, "rounds": ROUNDS, "calls": CALLS, "device": torch.cuda.get_device_name(dev),
           "source_digest": source_digest(), "model": args.model, "elements": sum(sizes), "tensors": plan.nt,
           "bits_equal": bool(equal)}
    if not equal:
        raise SystemExit("bucketed_rot_ab: the fused encoder's payload differs from the two-step route's; nothing timed")
    enc = {}
    for d in SIZES:
        enc[f"l2_{d}"] = lambda d=d: plan.qsgd_encode_bucketed(x, S, d, q_out=q[0], bnorm_out=bn[d][0], seed=9, offset=1)
        enc[f"max_{d}"] = lambda d=d: plan.qsgd_encode_bucketed_max(x, S, d, q_out=q[0], bnorm_out=bn[d][0], seed=9, offset=1)
        enc[f"rot_{d}"] = lambda d=d: plan.qsgd_encode_bucketed_max(x, S, d, rotate=True, rotation_seed=RS, q_out=q[0],
                                                                    bnorm_out=bn[d][0], seed=9, offset=1)
    out["encode"] = group(enc)
    print(json.dumps({"encode": out["encode"]}), flush=True)
    dec = {}
    for d in SIZES:
        for K in CLIENTS:  # the same payload and scales K times: the traffic of K clients
            qs, ms = [q[k % 2] for k in range(K)], [bn[d][k % 2] for k in range(K)]
            dec[f"l2_{d}_k{K}"] = lambda d=d, qs=qs, ms=ms: plan.qsgd_decode_sum_bucketed(qs, 8, L, d, ms, y_out=y)
            dec[f"rot_{d}_k{K}"] = lambda d=d, qs=qs, ms=ms: plan.qsgd_decode_sum_bucketed_rot(qs, 8, L, d, RS, ms, y_out=y)
    out["decode_sum"] = group(dec)
    print(json.dumps({"decode_sum": out["decode_sum"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}), flush=True)


if __name__ == "__main__":
    main()
