#!/usr/bin/env python
"""The routed mixture-of-experts launches above 16 rows at Mixtral-8x7B geometry: what each costs,
beside the composed route and beside the dense fused tile kernel doing the same flops.

  python scripts/moe_prefill_times.py                       # -> profiles/moe_prefill_times.txt
  python scripts/moe_prefill_times.py --bench --parent DIR  # bench.py's line, parent and this tree in turn

H 4096, I 14336, E 8, top-k 2, NF4 + double quant, fp16; T = 32 .. 8192 rows of randn, routed by the
router itself (`entries_per_expert` is what it chose).  us per call: COPIES calls over rotating weight
and activation buffers captured back to back into one graph and replayed between two events
(scripts/sample_times.py's graph_time_us); medians of three interleaved repeats with their min and max.
  route / plan / pair / down   qz_moe_route_rows, qz_moe_plan, qz_moe_gemm_pair_silu_4bit, qz_moe_gemm_down_4bit
  combine                      qz_moe_gemm_down_4bit over a plan that puts every entry in the last segment:
                               its tile launch leaves at once, what remains is the combine launch (plus
                               one launch of empty workgroups); down_gemm = down - combine
  composed                     SparseMoe4bit._composed on the same rows (it synchronises: host clock)
  dense_pair / dense_down      the yardstick: gemm_4bit(route="fused") on T * top_k / E rows over ONE dense
                               [2I, H] (resp. [H, I]) weight -- the existing tile kernel, no gather and no
                               routing -- and silu_mul on its output; E of them do the grouped launch's flops
  pair_over_dense              pair / (E * (dense_pair + silu_mul)); down_over_dense = down_gemm / (E * dense_down)
  *_tflops                     2 * n * rows * K flops of the grouped launch over its time
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

H, I, E, TOPK = 4096, 14336, 8, 2
COPIES = 3


def _stats(xs):
    s = sorted(xs)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


@torch.inference_mode()
def moe_cases(emit, repeat, rows):
    import quantizations_amd as qa
    from quantizations_amd.core import (gemm_4bit, moe_gemm_down, moe_gemm_pair_silu, moe_plan, moe_route_rows)
    from quantizations_amd.layer_ops import silu_mul
    from quantizations_amd.moe import SparseMoe4bit

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    moe = SparseMoe4bit((torch.randn(E, H, device=dev, generator=g) / 64).half(),
                        (torch.randn(E, 2 * I, H, device=dev, generator=g) * 0.02).half(),
                        (torch.randn(E, H, I, device=dev, generator=g) * 0.02).half(), TOPK)
    gu_state, dn_state = moe.gate_up_proj.quant_state, moe.down_proj.quant_state
    gus = [moe.gate_up_proj.data.clone() for _ in range(COPIES)]
    dns = [moe.down_proj.data.clone() for _ in range(COPIES)]
    dense_gu = [qa.quantize_4bit((torch.randn(2 * I, H, device=dev, generator=g) * 0.02).half(), quant_type="nf4")
                for _ in range(COPIES)]
    dense_dn = [qa.quantize_4bit((torch.randn(H, I, device=dev, generator=g) * 0.02).half(), quant_type="nf4")
                for _ in range(COPIES)]
    for T in rows:
        n, per = T * TOPK, T * TOPK // E
        xs = [torch.randn(T, H, device=dev, generator=g).half() for _ in range(COPIES)]
        routed = [moe_route_rows(x, moe.gate.weight, TOPK) for x in xs]
        plans = [moe_plan(idx, E) for idx, _ in routed]
        hs = [moe_gemm_pair_silu(xs[i], gus[i], gu_state, routed[i][0], plans[i], E) for i in range(COPIES)]
        nowhere = (plans[0][0], torch.tensor([0] * (E + 1) + [n], dtype=torch.int32, device=dev))
        halves = [tuple(u.contiguous() for u in gemm_4bit(xs[i][:per], *dense_gu[i], route="fused").chunk(2, dim=-1))
                  for i in range(COPIES)]
        calls = {
            "route": [lambda i=i: moe_route_rows(xs[i], moe.gate.weight, TOPK) for i in range(COPIES)],
            "plan": [lambda i=i: moe_plan(routed[i][0], E) for i in range(COPIES)],
            "pair": [lambda i=i: moe_gemm_pair_silu(xs[i], gus[i], gu_state, routed[i][0], plans[i], E)
                     for i in range(COPIES)],
            "down": [lambda i=i: moe_gemm_down(hs[i], dns[i], dn_state, *routed[i], plans[i], E) for i in range(COPIES)],
            "combine": [lambda i=i: moe_gemm_down(hs[i], dns[i], dn_state, *routed[i], nowhere, E) for i in range(COPIES)],
            "dense_pair": [lambda i=i: gemm_4bit(xs[i][:per], *dense_gu[i], route="fused") for i in range(COPIES)],
            "silu_mul": [lambda i=i: silu_mul(*halves[i]) for i in range(COPIES)],
            "dense_down": [lambda i=i: gemm_4bit(hs[i].view(n, I)[:per], *dense_dn[i], route="fused")
                           for i in range(COPIES)],
        }
        assert all(f() is not None for fs in calls.values() for f in fs)
        us = {k: [] for k in calls}
        composed = []
        for _ in range(repeat):
            for k, fs in calls.items():
                us[k].append(graph_time_us(fs, reps=5))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = moe._composed(xs[0])
            torch.cuda.synchronize()
            composed.append(1e6 * (time.perf_counter() - t0))
        fast = moe._grouped(xs[0])
        row = {"case": "moe_prefill", "H": H, "I": I, "E": E, "top_k": TOPK, "T": T, "format": "nf4+dq", "dtype": "fp16",
               "copies": COPIES, "token_tile": 128 if n > 64 * E else 64, "dense_rows": per,
               "entries_per_expert": torch.bincount(routed[0][0].flatten().long(), minlength=E).tolist(),
               "max_abs_grouped_minus_composed": round((fast.float() - ref.float()).abs().max().item(), 5)}
        for k, v in us.items():
            row[k + "_us"] = _stats(v)
        row["composed_us_host_clock"] = _stats(composed)
        med = {k: row[k + "_us"]["median"] for k in us}
        down_gemm = med["down"] - med["combine"]
        row["down_gemm_us"] = round(down_gemm, 2)
        row["four_entry_points_us"] = round(med["route"] + med["plan"] + med["pair"] + med["down"], 2)
        row["composed_over_grouped"] = round(row["composed_us_host_clock"]["median"] / row["four_entry_points_us"], 2)
        row["pair_over_dense"] = round(med["pair"] / (E * (med["dense_pair"] + med["silu_mul"])), 2)
        row["down_over_dense"] = round(down_gemm / (E * med["dense_down"]), 2)
        row["pair_tflops"] = round(2.0 * n * 2 * I * H / (med["pair"] * 1e-6) / 1e12, 1)
        row["down_gemm_tflops"] = round(2.0 * n * H * I / (down_gemm * 1e-6) / 1e12, 1)
        row["dense_pair_tflops"] = round(2.0 * per * 2 * I * H / (med["dense_pair"] * 1e-6) / 1e12, 1)
        row["dense_down_tflops"] = round(2.0 * per * H * I / (med["dense_down"] * 1e-6) / 1e12, 1)
        emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "moe_prefill_times.txt"))
    ap.add_argument("--rows", type=int, nargs="+", default=[32, 128, 512, 2048, 8192])
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.bench else "w") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if args.bench:
            bench_cases(emit, args)
        else:
            moe_cases(emit, args.repeat, args.rows)


if __name__ == "__main__":
    main()
