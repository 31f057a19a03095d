#!/usr/bin/env python
"""The wide multi-token 4-bit launches (17..64 rows) beside what the same rows cost today.

  python scripts/mt_wide_times.py                        # launches -> profiles/mt_wide_times.txt
  python scripts/mt_wide_times.py --sessions             # appends the Llama-3-8B session steps
  python scripts/mt_wide_times.py --bench --parent DIR   # appends bench.py's line, parent and this tree in turn

Launches: NF4 + double quant, fp16, T = 17, 32, 48, 64, on 4096 x 4096, 14336 x 4096, 4096 x 14336 and
the grouped q/k/v (4096 + 1024 + 1024 rows) and gate/up (2 x 14336 rows) sets of Llama-3-8B.  us per
call: one call per weight copy captured back to back into one graph and replayed between two events
(scripts/sample_times.py's graph_time_us); the copies rotate so that a pass reads at least 512 MiB of
weights, past the last-level cache.  Medians of three interleaved repeats with their min and max.
  wide      gemm_4bit_wide / gemm_4bit_grouped_wide: the T rows in one launch
  tile      what the rows run on without decode_rows: gemm_4bit(route="fused"), per member for a set
  mt16_x    the existing 16-row launch repeated ceil(T / 16) times (on the first 16 rows)
  mt16      the 16-row launch once

Sessions: bench.py's Llama-3-8B (random init, NF4 + double quant, fp16) laid out by
prepare_for_decode; ms per replayed step of a SpeculativeSession with 4 streams x 8 rows and of a
StreamSession with batch 32, with decode_rows=64 and, where the session opens at all, without.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from sample_times import graph_time_us  # noqa: E402  (scripts/ is sys.path[0])
from streams_times import bench_cases  # noqa: E402

SHAPES = {"4096x4096": ([4096], 4096), "14336x4096": ([14336], 4096), "4096x14336": ([4096], 14336),
          "qkv": ([4096, 1024, 1024], 4096), "gate_up": ([14336, 14336], 4096)}
TS = (17, 32, 48, 64)


def _stats(xs):
    s = sorted(xs)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


@torch.inference_mode()
def launch_cases(emit, repeat):
    from quantizations_amd.core import (gemm_4bit, gemm_4bit_grouped, gemm_4bit_grouped_wide, gemm_4bit_wide,
                                        quantize_4bit)

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, (rows, K) in SHAPES.items():
        copies = max(2, -(-(512 << 20) // (sum(rows) * K // 2)))
        sets = []
        for _ in range(copies):
            sets.append([quantize_4bit((torch.randn(M, K, device=dev, generator=g) * 0.02).half(), quant_type="nf4")
                         + (None,) for M in rows])
        for T in TS:
            xs = [torch.randn(T, K, device=dev, generator=g).half() for _ in range(copies)]
            nb = -(-T // 16)
            if len(rows) == 1:
                wide = [lambda x=x, it=it: gemm_4bit_wide(x, it[0][0], it[0][1]) for x, it in zip(xs, sets)]
            else:
                wide = [lambda x=x, it=it: gemm_4bit_grouped_wide(x, it) for x, it in zip(xs, sets)]
            calls = {
                "wide": wide,
                "tile": [lambda x=x, it=it: [gemm_4bit(x, p, st, route="fused") for p, st, _ in it]
                         for x, it in zip(xs, sets)],
                "mt16_x": [lambda x=x, it=it: [gemm_4bit_grouped(x[:16], it) for _ in range(nb)]
                           for x, it in zip(xs, sets)],
                "mt16": [lambda x=x, it=it: gemm_4bit_grouped(x[:16], it) for x, it in zip(xs, sets)],
            }
            us = {k: [] for k in calls}
            for _ in range(repeat):
                for k, fs in calls.items():
                    us[k].append(graph_time_us(fs, reps=10))
            row = {"case": "launch", "shape": name, "rows": rows, "K": K, "T": T, "format": "nf4+dq", "dtype": "fp16",
                   "copies": copies}
            for k, v in us.items():
                row[k + "_us"] = _stats(v)
            med = {k: row[k + "_us"]["median"] for k in us}
            row["wide_over_tile"] = round(med["wide"] / med["tile"], 3)
            row["wide_over_mt16_x"] = round(med["wide"] / med["mt16_x"], 3)
            row["wide_over_mt16"] = round(med["wide"] / med["mt16"], 3)
            emit(row)
        del sets
        torch.cuda.empty_cache()


def _step_ms(sess, steps, warmup):
    for _ in range(warmup):
        sess.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sess.step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def session_cases(emit, args):
    import bench
    from quantizations_amd.generation import SpeculativeSession, StreamSession, prepare_for_decode
    from quantizations_amd.integration import set_decode_rows

    model, cfg = bench.build_model(args.layers, seed=0)
    prepare_for_decode(model)
    prompt, L = 32, 32 + 8 * (args.warmup + args.steps) + 16

    def open_session(kind, decode_rows):
        batch = 4 if kind == "speculative" else 32
        ids = torch.randint(0, cfg.vocab_size, (batch, prompt), generator=torch.Generator().manual_seed(1234)).cuda()
        if kind == "speculative":
            sess = SpeculativeSession(model, batch, L, draft_tokens=7, decode_rows=decode_rows)
        else:
            sess = StreamSession(model, batch, L, decode_rows=decode_rows)
        sess.prefill(ids, [prompt] * batch)
        return sess

    for kind in ("speculative", "stream"):
        row = {"case": "session", "kind": kind, "model": "llama3-8b", "layers": cfg.num_hidden_layers,
               "rows_per_step": 32, "steps": args.steps, "step_ms": {"decode_rows=64": [], "decode_rows=None": []}}
        for _ in range(args.repeat):
            for dr in (64, None):
                set_decode_rows(model, 16)
                try:
                    sess = open_session(kind, dr)
                except ValueError as e:
                    row["decode_rows=None refused"] = str(e)[:80]
                    continue
                row["step_ms"][f"decode_rows={dr}"].append(round(_step_ms(sess, args.steps, args.warmup), 3))
                del sess
        set_decode_rows(model, 16)
        emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", action="store_true", help="only the Llama-3-8B session steps (appended)")
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mt_wide_times.txt"))
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if (args.bench or args.sessions) else "w") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if args.bench:
            bench_cases(emit, args)
        elif args.sessions:
            session_cases(emit, args)
        else:
            launch_cases(emit, args.repeat)


if __name__ == "__main__":
    main()
