"""Bucketed QSGD on the bit-packed wire against the two-call path it replaces, A/B in one process on the
Llama-400M and ResNet-18 tensor lists at s = 4 and s = 8, bucket sizes d in {64, 512, 4096} (on-device draws).

  encode      two{d}      omf_qsgd_encode_bucketed followed by omf_qsgd_pack: the yardstick
              enc{d}      omf_qsgd_encode_bucketed alone (the unpacked wire)
              fa{d}       omf_qsgd_encode_bucketed_packed, output assignment 0 (thread i writes words i, i + 256, ...)
              fb{d}       the same, assignment 1 (two threads per 32-element group)
  decode      db{d}       omf_qsgd_decode_bucketed;             dp{d}  omf_qsgd_decode_bucketed_packed
  decode-sum  sb{d}       omf_qsgd_decode_sum_bucketed, K = 4;  sp{d}  omf_qsgd_decode_sum_bucketed_packed, K = 4

The sides of a group alternate: five rounds, each ten calls of every side in turn, every call between its own
pair of device events; a round's figure is the median of its ten calls.  Before any timing the three encodes'
words are compared on every group that holds a tensor element.  Per case the JSON holds each side's median of
round medians, its rounds and their max - min, and the counted bytes per element (w = 1 or 4 B of levels,
b = s + 2 bits of code: two 4 + 2 w + b / 8 + 4 / d, enc 4 + w + 4 / d, fused 4 + b / 8 + 4 / d; decode
w or b / 8, + 4 + 4 / d; sum K times the payload and norms, + 4), and the wire bytes of the update on both wires.

    python scripts/bucketed_packed_ab.py [--out profiles/bucketed_packed_ab.json]
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
K = 4
SIZES, WIDTHS = (64, 512, 4096), (4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/bucketed_packed_ab.json")
    ap.add_argument("--models", default="llama400m,resnet18")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bucketed_packed_ab: no GPU visible (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    out = {"k": K, "rounds": ROUNDS, "calls": CALLS, "device": torch.cuda.get_device_name(dev),
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
        groups = torch.zeros(-(-N // 32) * 32, dtype=torch.bool, device=dev)
        for o, n in zip(plan.offsets, plan.sizes):
            groups[o:o + n] = True
        groups = groups.view(-1, 32).any(dim=1)
        for s in WIDTHS:
            L, b = 2 ** s, s + 2
            width = codec.storage_width(L)
            w = width // 8
            words = plan.packed_words(L)
            q = torch.empty(plan.payload_elems(width), dtype=torch.int8 if width == 8 else torch.int32, device=dev)
            two = torch.zeros(words, dtype=torch.int32, device=dev)
            fused = {d: torch.zeros(words, dtype=torch.int32, device=dev) for d in SIZES}
            qd = {d: torch.empty_like(q) for d in SIZES}
            nb = {d: torch.empty(plan.bucket_layout(d)[1], device=dev) for d in SIZES}

            def enc(d, dst=None):
                return lambda: plan.qsgd_encode_bucketed(x, s, d, q_out=qd[d] if dst is None else dst, bnorm_out=nb[d],
                                                         seed=9, offset=1)

            def enc_two(d):
                def run():
                    plan.qsgd_encode_bucketed(x, s, d, q_out=q, bnorm_out=nb[d], seed=9, offset=1)
                    plan.qsgd_pack(q, width, L, packed_out=two)
                return run

            def enc_fused(d, mode):
                def run():
                    plan.set_bucket_pack(mode)
                    plan.qsgd_encode_bucketed_packed(x, s, d, packed_out=fused[d], bnorm_out=nb[d], seed=9, offset=1)
                return run

            wr = groups.repeat_interleave(b)
            equal = True
            for d in SIZES:
                enc_two(d)()
                for mode in (1, 0):  # the default last: fused[d] and nb[d] then hold what the decodes read
                    enc_fused(d, mode)()
                    equal = equal and torch.equal(fused[d][wr], two[wr])
                enc(d)()
            per = {d: 4 / d for d in SIZES}
            case = {"model": model, "s": s, "code_bits": b, "elements": sum(sizes), "tensors": plan.nt,
                    "words_equal": bool(equal),
                    "bytes_per_element": {**{f"two{d}": 4 + 2 * w + b / 8 + per[d] for d in SIZES},
                                          **{f"enc{d}": 4 + w + per[d] for d in SIZES},
                                          **{f"fa{d}": 4 + b / 8 + per[d] for d in SIZES},
                                          **{f"db{d}": w + 4 + per[d] for d in SIZES},
                                          **{f"dp{d}": b / 8 + 4 + per[d] for d in SIZES},
                                          **{f"sb{d}": K * (w + per[d]) + 4 for d in SIZES},
                                          **{f"sp{d}": K * (b / 8 + per[d]) + 4 for d in SIZES}},
                    "wire_bytes": {**{f"bucketed{d}": sum(n * w + 4 * -(-n // d) for n in sizes) for d in SIZES},
                                   **{f"packed{d}": sum(-(-n * b // 8) + 4 * -(-n // d) for n in sizes) for d in SIZES}}}
            out["cases"].append(case)
            if not equal:
                raise SystemExit(f"bucketed_packed_ab: the fused words differ from the two calls'; nothing timed\n"
                                 f"{json.dumps(case)}")
            sides = {}
            for d in SIZES:
                sides.update({f"two{d}": enc_two(d), f"enc{d}": enc(d), f"fa{d}": enc_fused(d, 0), f"fb{d}": enc_fused(d, 1)})
            case["encode"] = group(sides)
            plan.set_bucket_pack(0)
            sides = {}
            for d in SIZES:
                sides[f"db{d}"] = lambda d=d: plan.qsgd_decode_bucketed(qd[d], width, L, d, nb[d], y_out=y)
                sides[f"dp{d}"] = lambda d=d: plan.qsgd_decode_bucketed_packed(fused[d], L, d, nb[d], y_out=y)
            case["decode"] = group(sides)
            sides = {}
            for d in SIZES:
                sides[f"sb{d}"] = lambda d=d: plan.qsgd_decode_sum_bucketed([qd[d]] * K, width, L, d, [nb[d]] * K, y_out=y,
                                                                           divisor=float(K))
                sides[f"sp{d}"] = lambda d=d: plan.qsgd_decode_sum_bucketed_packed([fused[d]] * K, L, d, [nb[d]] * K,
                                                                                  y_out=y, divisor=float(K))
            case["decode_sum"] = group(sides)
            print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}), flush=True)


if __name__ == "__main__":
    main()
