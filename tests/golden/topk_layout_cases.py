"""Cases shared by the Top-K layout fixture (tests/golden/make_topk_layout_parent.py) and its readers
(tests/test_gpu_topk_layout.py, tests/test_topk_layout_host.py).  Plain Python: no torch, no GPU.
"""

import topk_matrix_inputs as M

CASES = [(name, ratio) for name, spec in M.PLANS.items() for ratio in spec.ratios]
EXACT_PLANS = ("many",)  # more than 256 tensors: the exact path, whose sort temporary rocPRIM sizes


def case_key(name, ratio):
    return f"{name}@{ratio!r}"


def count_vectors(spec, ratio):
    """Two per-tensor count vectors of a received message: the ratio's own, and one with zeros (tensor 0,
    every third one after it, so the start, the middle and often the end) and a k == n entry (tensor 1)."""
    own = spec.ks(ratio)
    mixed = [0 if t % 3 == 0 else k for t, k in enumerate(own)]
    mixed[1] = spec.sizes[1]
    return own, mixed


def a256(b):
    return (b + 255) & ~255


def dead_bytes(nt):
    """The eight workspace regions the encoder stopped allocating, as the recorded build laid them out: koff,
    kk, kb2, tfirst, tlast, bbase and sbase (their contents are in the plan-owned table), and fse (16384 fine
    bins of 4 bytes per tensor, a table topk_plan stored and nothing read)."""
    tables = a256(8 * (nt + 1)) + 2 * a256(8 * nt) + 2 * a256(4 * nt) + 2 * a256(4 * (nt + 1))
    return tables + a256(4 * nt * 16384)


# Two plans of equal nt and arena_end and different sizes (explicit offsets): 152 against 40 bucket slots,
# so the bucket-table regions (4, 16 and 4 bytes per slot, rounded to 256) differ in size.
PAIR_OFFSETS = [16448 * t for t in range(8)]
PAIR_SIZES = ([16385] * 8, [513] * 7 + [16385])
PAIR_RATIO = 0.05
