#!/usr/bin/env python
"""The sampled token pick: per-call times of layer_ops.sample_step beside the composed torch route
and greedy_step, and tok/s of generation.DecodeSession beside bench.py's own decode loop.

  python scripts/sample_times.py                   # both parts, written to profiles/sample_times.txt
  python scripts/sample_times.py --launches        # only the per-call times
  python scripts/sample_times.py --generate --repeat 3

Per-call times: V = 128256 fp16 logits (randn * 4), B = 1, 4, 8.  COPIES calls over rotating logits
buffers (64: 16-128 MiB, past the 4 MiB L2) are captured back to back into one graph, which is
replayed `reps` times between two events; the figure is the mean per call.  Routes: (a) sample_step
with top_k 50, top_p 0.9, temperature 0.8; (b) the same with top-k off; (c) the composed torch
route on the inputs of (a) and of (b); greedy_step for scale.

tok/s: bench.py's Llama-3-8B (random init, NF4 + double quant, fp16, batch 1), one model, laid out by
generation.prepare_for_decode.  Per repeat, interleaved: bench.decode_bench_graph (its own captured
loop, the README's figure), a DecodeSession with greedy streams (the same launches), and one
sampling with top_k 50, top_p 0.9, temperature 0.8.  Each prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

V = 128256
COPIES = 64


def graph_time_us(fns, reps=20):
    """us per call of fns captured back to back into one graph and replayed `reps` times."""
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
def launch_cases(emit):
    from quantizations_amd.layer_ops import greedy_step, sample_step

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in (1, 4, 8):
        logits = [(torch.randn(B, V, device=dev, generator=g) * 4).half() for _ in range(COPIES)]
        H = 4 * COPIES
        hist = torch.zeros((B, H), dtype=torch.int64, device=dev)
        pos = torch.zeros(1, dtype=torch.int64, device=dev)
        tok = torch.zeros(B, dtype=torch.int64, device=dev)
        U = torch.rand((B, H), device=dev, generator=g)
        T = torch.full((B,), 0.8, device=dev)
        P = torch.full((B,), 0.9, device=dev)
        K50 = torch.full((B,), 50, dtype=torch.int32, device=dev)
        K0 = torch.zeros(B, dtype=torch.int32, device=dev)

        def timed(fn):
            pos.zero_()
            return graph_time_us([lambda lo=lo: fn(lo) for lo in logits])

        row = {"case": "pick", "V": V, "B": B, "dtype": "fp16", "copies": COPIES}
        row["sample_k50_p0.9_us"] = timed(lambda lo: sample_step(lo, hist, pos, tok, T, K50, P, U))
        row["sample_p0.9_us"] = timed(lambda lo: sample_step(lo, hist, pos, tok, T, K0, P, U))
        row["composed_k50_p0.9_us"] = timed(lambda lo: sample_step(lo, hist, pos, tok, T, K50, P, U, composed=True))
        row["composed_p0.9_us"] = timed(lambda lo: sample_step(lo, hist, pos, tok, T, K0, P, U, composed=True))
        row["greedy_us"] = timed(lambda lo: greedy_step(lo, hist, pos, tok))
        row["fused_ahead_of_composed"] = bool(row["sample_k50_p0.9_us"] < row["composed_k50_p0.9_us"]
                                              and row["sample_p0.9_us"] < row["composed_p0.9_us"])
        emit({k: round(v, 2) if isinstance(v, float) else v for k, v in row.items()})
        del logits
        torch.cuda.empty_cache()


def session_tok_s(model, cfg, steps, warmup, prompt, sampled):
    from quantizations_amd.generation import DecodeSession

    ids = torch.randint(0, cfg.vocab_size, (1, prompt), generator=torch.Generator().manual_seed(1234)).cuda()
    sess = DecodeSession(model, 1, prompt + warmup + steps + 8)
    if sampled:
        sess.set_sampling(temperature=0.8, top_k=50, top_p=0.9)
        sess.seed(0)
    sess.prefill(ids)
    for _ in range(warmup):
        sess.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sess.step()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def generate_cases(emit, args):
    import bench
    from quantizations_amd.generation import prepare_for_decode

    model, cfg = bench.build_model(args.layers, seed=0)
    counts = prepare_for_decode(model)
    runs = {"bench_decode_bench_graph": [], "session_greedy": [], "session_sampled_k50_p0.9_t0.8": []}
    for _ in range(args.repeat):
        dt, _ = bench.decode_bench_graph(model, cfg, args.steps, args.warmup, args.prompt, 1, 1)
        runs["bench_decode_bench_graph"].append(args.steps / dt)
        runs["session_greedy"].append(session_tok_s(model, cfg, args.steps, args.warmup, args.prompt, False))
        runs["session_sampled_k50_p0.9_t0.8"].append(session_tok_s(model, cfg, args.steps, args.warmup, args.prompt, True))
    b = runs["bench_decode_bench_graph"]
    gmean = sum(runs["session_greedy"]) / args.repeat
    emit({"case": "decode", "model": "llama3-8b", "layers": cfg.num_hidden_layers, "batch": 1, "steps": args.steps,
          "prepare_for_decode": counts, "tok_s": {k: [round(v, 2) for v in vs] for k, vs in runs.items()},
          "greedy_session_mean_inside_bench_spread": bool(min(b) <= gmean <= max(b))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true", help="only the per-call times")
    ap.add_argument("--generate", action="store_true", help="only the Llama-3-8B tok/s")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sample_times.txt"))
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    both = not (args.launches or args.generate)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if not both else "w") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if both or args.launches:
            launch_cases(emit)
        if both or args.generate:
            with torch.inference_mode():
                generate_cases(emit, args)


if __name__ == "__main__":
    main()
