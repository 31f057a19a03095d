#!/usr/bin/env python
"""LoRA adapters on the bench.py decode step: tok/s fused (shrink + the adapter-carrying launches)
against the composed torch path, and the per-launch times of the new launches beside their plain twins.

  python scripts/lora_times.py                       # tok/s: no adapter, r=16 on all seven / on q,v; fused and composed
  python scripts/lora_times.py --launches            # per-launch us of the Llama-3-8B layer shapes
  python scripts/lora_times.py --adapters qv --composed --steps 128

The model is bench.py's Llama-3-8B (random init, NF4 + double quant, fp16, batch 1) with its decode
layout (groups, layer ops, fused norms) and its HIP-graph step: build_model, prepare_decode_model and
decode_bench_graph are bench.py's own.  One model is built and re-captured for every case.  Prints one
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


def set_adapters(model, names, rank, seed=0):
    import quantizations_amd as qa

    g = torch.Generator(device="cuda").manual_seed(seed)
    n = 0
    for name, m in model.named_modules():
        if not isinstance(m, qa.Linear4bit):
            continue
        m.clear_adapter()
        if name.split(".")[-1] in names:
            A = (torch.randn(rank, m.in_features, device="cuda", generator=g) * 0.02).half()
            B = (torch.randn(m.out_features, rank, device="cuda", generator=g) / math.sqrt(rank) * 0.1).half()
            m.set_adapter(A, B, 1.0)
            n += 1
    return n


def tok_s_cases(args):
    from quantizations_amd import lora

    model, cfg = bench.build_model(args.layers, seed=0)
    bench.prepare_decode_model(model, 0, 1, False)
    cases = [(a, c) for a in args.adapters for c in ((False, True) if a != "none" else (False,))
             if not (args.composed and not c and a != "none") and not (args.fused and c)]
    for adapters, composed in cases:
        n = set_adapters(model, SETS[adapters], args.rank)
        lora.FORCE_COMPOSED = composed
        runs = []
        for _ in range(args.repeat):
            dt, _ = bench.decode_bench_graph(model, cfg, args.steps, args.warmup, args.prompt, 1, 1)
            runs.append(args.steps / dt)
        lora.FORCE_COMPOSED = False
        print(json.dumps({"case": "decode", "model": "llama3-8b", "layers": cfg.num_hidden_layers, "adapters": adapters,
                          "rank": args.rank if n else 0, "layers_with_adapter": n,
                          "path": "none" if not n else "composed" if composed else "fused",
                          "tok_s": [round(v, 2) for v in runs], "steps": args.steps}), flush=True)


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
    """The four projection launches of a Llama-3-8B layer with rank-r adapters on every member,
    beside the plain launch each replaces, and their shrink launches."""
    from quantizations_amd import layer_ops, lora
    from quantizations_amd.core import gemv_4bit, gemv_4bit_grouped, gemv_4bit_pair_silu, quantize_4bit

    r = args.rank
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)

    def weights(rows, K, copies):
        out = []
        for _ in range(copies):
            items = []
            for M in rows:
                W = (torch.randn(M, K, device=dev, generator=g) * 0.02).half()
                pk, st = quantize_4bit(W, quant_type="nf4", compress_statistics=True)
                A = (torch.randn(r, K, device=dev, generator=g) * 0.02).half()
                B = (torch.randn(M, r, device=dev, generator=g) / math.sqrt(r)).half()
                items.append((pk, st, lora.LoraAdapter(A, B, 1.0, dev)))
            out.append(items)
        return out

    def copies_for(rows, K):   # enough copies that a pass reads >= 512 MiB of weights (past the 256 MiB MALL)
        return max(2, -(-(512 << 20) // (sum(rows) * K // 2)))

    def report(name, **us):
        print(json.dumps({"case": "launch", "name": name, "rank": r, **{k: round(v, 2) for k, v in us.items()}}),
              flush=True)

    eps = 1e-5
    # q/k/v and gate/up: grouped launch with the fused norm
    for name, rows in (("q/k/v + norm", (4096, 1024, 1024)), ("gate/up + norm", (14336, 14336))):
        K = 4096
        ws = weights(rows, K, copies_for(rows, K))
        x = torch.randn(1, 1, K, device=dev, generator=g).half()
        nw = torch.ones(K, device=dev).half()
        ads = [[it[2] for it in items] for items in ws]
        ts = [lora.shrink(x, a, norm=(nw, eps)) for a in ads]
        plain = [lambda it=items: gemv_4bit_grouped(x, [(p, s, None) for p, s, _ in it], exact_codes=True,
                                                    norm=(nw, eps)) for items in ws]
        fused = [lambda it=items, t=t, a=a: gemv_4bit_grouped(
            x, [(p, s, None) for p, s, _ in it], exact_codes=True, norm=(nw, eps),
            lora=(t[0], [(ad.B, o) for ad, o in zip(a, t[1])])) for items, t, a in zip(ws, ts, ads)]
        shrink = [lambda a=a: lora.shrink(x, a, norm=(nw, eps)) for a in ads]
        us = {"grouped_us": graph_time_us(plain), "grouped_lora_us": graph_time_us(fused),
              "shrink_us": graph_time_us(shrink)}
        if len(rows) == 2:   # the plain gate/up is the pair launch; with adapters: grouped + silu_mul
            pair = [lambda it=items: gemv_4bit_pair_silu(x, [(p, s, None) for p, s, _ in it], exact_codes=True,
                                                         norm=(nw, eps)) for items in ws]
            gu = torch.randn(2, 1, 1, rows[0], device=dev, generator=g).half()
            us["pair_silu_us"] = graph_time_us(pair)
            us["silu_mul_us"] = graph_time_us([lambda: layer_ops.silu_mul(gu[0], gu[1])] * 8)
        report(name, **us)
        del ws, plain, fused, shrink, ads, ts
        torch.cuda.empty_cache()
    # o_proj and down_proj: single launch with the residual epilogue
    for name, M, K in (("o_proj + residual", 4096, 4096), ("down_proj + residual", 4096, 14336)):
        ws = weights((M,), K, copies_for((M,), K))
        x = torch.randn(1, 1, K, device=dev, generator=g).half()
        res = torch.randn(1, 1, M, device=dev, generator=g).half()
        ts = [lora.shrink(x, [items[0][2]])[0] for items in ws]
        plain = [lambda it=items[0]: gemv_4bit(x, it[0], state=it[1], exact_codes=True, residual=res) for items in ws]
        fused = [lambda it=items[0], t=t: gemv_4bit(x, it[0], state=it[1], exact_codes=True, residual=res,
                                                    lora=(it[2].B, t)) for items, t in zip(ws, ts)]
        shrink = [lambda it=items[0]: lora.shrink(x, [it[2]]) for items in ws]
        report(name, gemv_us=graph_time_us(plain), gemv_lora_us=graph_time_us(fused), shrink_us=graph_time_us(shrink))
        del ws, plain, fused, shrink, ts
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--adapters", nargs="+", choices=sorted(SETS), default=["none", "all", "qv"])
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--composed", action="store_true", help="only the composed torch path (forces the fallback)")
    ap.add_argument("--fused", action="store_true", help="only the fused path")
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
