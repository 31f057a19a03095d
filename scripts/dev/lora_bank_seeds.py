"""CPU: pick the seeds of tests/test_gpu_lora_bank.py.

For every case of that file, print the first seed for which the adapter term of EVERY adapted row is
at least 0.35 of its base term on the unquantised fp16 weight (the file's precondition: the tests
then assert 1/4 on the quantised reference).  Paste the seeds into the case tables; a case whose
shapes, ranks or slots change needs its seed picked again.

    python scripts/dev/lora_bank_seeds.py
"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import test_gpu_lora_bank as tb  # noqa: E402

BAR = 0.35


def first_seed(ratio_of, limit=2000):
    for seed in range(limit):
        r = ratio_of(seed)
        if r >= BAR:
            return seed, r
    raise SystemExit("no seed found")


def group_ratio(seed):
    rows, K, T, _, slots, _ = tb.GROUP_CASE
    x, drawn = tb._group_draw(seed)
    worst = 1e9
    for M, ents in zip(rows, drawn):
        if ents is None:
            continue
        base, ad, adapted = tb._row_terms(tb._w16(M, K).double(), x, ents, slots, 1)
        worst = min([worst] + [(ad[c].norm() / base[c].norm()).item() for c in range(T) if adapted[c]])
    return worst


def main():
    for i, (M, K, T, ranks, dtype, qt, dq, bias, slots, seed) in enumerate(tb.CASES):
        s, r = first_seed(lambda sd: tb.min_ratio_unquantised(M, K, T, ranks, dtype, sd, slots))
        print(f"CASES[{i}] {M}x{K} T={T} r={ranks}: seed {s} (min ratio {r:.3f}; the table has {seed})")
    M, K, streams, S, ranks, dtype, slots, seed = tb.STREAM_CASE
    s, r = first_seed(lambda sd: tb.min_ratio_unquantised(M, K, streams * S, ranks, dtype, sd, slots, S))
    print(f"STREAM_CASE: seed {s} (min ratio {r:.3f}; the table has {seed})")
    M, K, T, ranks, dtype, seed = tb.NOSLOT_CASE
    s, r = first_seed(lambda sd: tb.min_ratio_unquantised(M, K, T, ranks, dtype, sd, None))
    print(f"NOSLOT_CASE: seed {s} (min ratio {r:.3f}; the table has {seed})")
    for name, M, K, T, ranks, dtype, slots, seed in tb.COMPOSED_CASES:
        adt = torch.float16 if dtype == torch.float32 else dtype
        s, r = first_seed(lambda sd: tb.min_ratio_unquantised(M, K, T, ranks, adt, sd, slots))
        print(f"COMPOSED_CASES[{name!r}]: seed {s} (min ratio {r:.3f}; the table has {seed})")
    s, r = first_seed(group_ratio)
    print(f"GROUP_CASE: seed {s} (min ratio {r:.3f}; the table has {tb.GROUP_CASE[5]})")


if __name__ == "__main__":
    main()
