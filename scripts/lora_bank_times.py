#!/usr/bin/env python
"""Adapter banks on the batched bench.py decode step: tok/s of the fused route (shrink_mt + the
multi-token launch carrying the expand) against the composed bank route, and the per-launch times of
the new launches beside their plain twins.

  python scripts/lora_bank_times.py                    # tok/s at batch 4 and 8: no bank; q,v; all seven -- fused and composed
  python scripts/lora_bank_times.py --launches         # per-launch us of the Llama-3-8B layer shapes at batch 4 and 8
  python scripts/lora_bank_times.py --batch 8 --adapters all --fused

The model is bench.py's Llama-3-8B (random init, NF4 + double quant, fp16) with its decode layout and
HIP-graph step (build_model, prepare_decode_model and decode_bench_graph are bench.py's own), `batch`
streams.  Every bank holds three rank-r adapters; the streams cycle through slots 0, 1, 2, -1, so one
stream in four runs on no adapter.  One model is built and re-captured for every case.  Prints one
JSON line per case.
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import bench  # noqa: E402

ALL7 = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
SETS = {"none": (), "all": ALL7, "qv": ("q_proj", "v_proj")}
N_ADAPTERS = 3


def stream_slots(batch, dev):
    from quantizations_amd.core import MT_MAX_TOKENS

    s = torch.full((MT_MAX_TOKENS,), -1, dtype=torch.int32)
    s[:batch] = torch.tensor([(0, 1, 2, -1)[b % 4] for b in range(batch)], dtype=torch.int32)
    return s.to(dev)


def set_banks(model, names, rank, slots, seed=0):
    import quantizations_amd as qa

    g = torch.Generator(device="cuda").manual_seed(seed)
    n = 0
    for name, m in model.named_modules():
        if not isinstance(m, qa.Linear4bit):
            continue
        m.clear_adapter_bank()
        if name.split(".")[-1] in names:
            ents = [((torch.randn(rank, m.in_features, device="cuda", generator=g) * 0.02).half(),
                     (torch.randn(m.out_features, rank, device="cuda", generator=g) / math.sqrt(rank) * 0.1).half(), 1.0)
                    for _ in range(N_ADAPTERS)]
            m.set_adapter_bank(ents, slots)
            n += 1
    return n


def tok_s_cases(args):
    from quantizations_amd import lora

    model, cfg = bench.build_model(args.layers, seed=0)
    bench.prepare_decode_model(model, 0, 1, False)
    for batch in args.batch:
        slots = stream_slots(batch, torch.device("cuda"))
        cases = [(a, c) for a in args.adapters for c in ((False, True) if a != "none" else (False,))
                 if not (args.composed and not c and a != "none") and not (args.fused and c)]
        for adapters, composed in cases:
            n = set_banks(model, SETS[adapters], args.rank, slots)
            lora.FORCE_COMPOSED = composed
            runs = []
            for _ in range(args.repeat):
                dt, _ = bench.decode_bench_graph(model, cfg, args.steps, args.warmup, args.prompt, 1, batch)
                runs.append(args.steps * batch / dt)
            lora.FORCE_COMPOSED = False
            print(json.dumps({"case": "decode", "model": "llama3-8b", "layers": cfg.num_hidden_layers, "batch": batch,
                              "adapters": adapters, "bank": N_ADAPTERS if n else 0, "rank": args.rank if n else 0,
                              "layers_with_bank": n, "path": "none" if not n else "composed" if composed else "fused",
                              "tok_s": [round(v, 2) for v in runs], "steps": args.steps}), flush=True)
        set_banks(model, (), args.rank, slots)


def graph_time_us(fns, reps=20):
    """us per call of the launches fns (one per weight copy, so the weights come from HBM), captured
    back to back into one graph and replayed `reps` times."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for f in fns:
            f()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in fns:
            f()
    for _ in range(3):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / (reps * len(fns))


@torch.inference_mode()
def launch_cases(args):
    """The four projection launches of a Llama-3-8B layer over `batch` streams with a bank of three
    rank-r adapters on every member, beside the plain launch each replaces, and their shrink_mt launch."""
    from quantizations_amd import lora
    from quantizations_amd.core import gemm_4bit_grouped, quantize_4bit

    r = args.rank
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)

    def copies_for(rows, K):   # enough copies that a pass reads >= 512 MiB of weights (past the 256 MiB MALL)
        return max(2, -(-(512 << 20) // (sum(rows) * K // 2)))

    for batch in args.batch:
        slots = stream_slots(batch, dev)
        for name, rows, K in (("q/k/v", (4096, 1024, 1024), 4096), ("gate/up", (14336, 14336), 4096),
                              ("o_proj", (4096,), 4096), ("down_proj", (4096,), 14336)):
            ws = []
            for _ in range(copies_for(rows, K)):
                items, banks = [], []
                for M in rows:
                    W = (torch.randn(M, K, device=dev, generator=g) * 0.02).half()
                    pk, st = quantize_4bit(W, quant_type="nf4", compress_statistics=True)
                    ents = [((torch.randn(r, K, device=dev, generator=g) * 0.02).half(),
                             (torch.randn(M, r, device=dev, generator=g) / math.sqrt(r)).half(), 1.0)
                            for _ in range(N_ADAPTERS)]
                    items.append((pk, st, None))
                    banks.append(lora.AdapterBank(ents, slots, M, K, dev))
                ws.append((items, banks))
            x = torch.randn(batch, 1, K, device=dev, generator=g).half()
            ts = [lora.shrink_mt(x, banks) for _, banks in ws]
            plain = [lambda it=items: gemm_4bit_grouped(x, it) for items, _ in ws]
            fused = [lambda it=items, b=banks, t=t: gemm_4bit_grouped(
                x, it, lora=(t[0], [(bk.B, o) for bk, o in zip(b, t[1])], slots, 1)) for (items, banks), t in zip(ws, ts)]
            shrink = [lambda b=banks: lora.shrink_mt(x, b) for _, banks in ws]
            print(json.dumps({"case": "launch", "name": name, "batch": batch, "rank": r, "bank": N_ADAPTERS,
                              "grouped_us": round(graph_time_us(plain), 2),
                              "grouped_lora_us": round(graph_time_us(fused), 2),
                              "shrink_mt_us": round(graph_time_us(shrink), 2)}), flush=True)
            del ws, plain, fused, shrink, ts
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--adapters", nargs="+", choices=sorted(SETS), default=["none", "all", "qv"])
    ap.add_argument("--batch", nargs="+", type=int, default=[4, 8])
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--composed", action="store_true", help="only the composed bank route (forces the fallback)")
    ap.add_argument("--fused", action="store_true", help="only the fused route")
    ap.add_argument("--launches", action="store_true", help="per-launch times instead of tok/s")
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=2)
    args = ap.parse_args()
    if args.launches:
        launch_cases(args)
    else:
        with torch.inference_mode():
            tok_s_cases(args)


if __name__ == "__main__":
    main()
