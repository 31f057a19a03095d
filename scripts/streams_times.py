#!/usr/bin/env python
"""Per-stream positions: what they cost beside the shared-position launches.

  python scripts/streams_times.py                      # launches + sessions, written to profiles/streams_times.txt
  python scripts/streams_times.py --launches           # only the per-call times
  python scripts/streams_times.py --sessions --repeat 3
  python scripts/streams_times.py --bench --parent DIR # bench.py's line, this tree and a built parent tree in turn

Per-call times (us): COPIES calls over rotating buffers are captured back to back into one graph,
which is replayed `reps` times between two events, as scripts/sample_times.py does; three repeats.
* attention, Llama-3-8B heads (Hq 32, Hkv 8, D 128, fp16), B = 4 and 8: decode_attention and
  decode_attention_streams with every stream at L - 64 for L = 512 and L = 4096 ("equal"), and at
  L = 4096 with stream 0 at L - 64 and the others at 40 ("ragged": the shared launch has one position
  for the batch, so it runs -- as a padded batch would -- at the long stream's).  The caches rotate
  (16 copies: 0.5-2 GiB at L = 4096); each copy of the shared launch has its own position word,
  which the launch advances by one per replay (fewer than 64 replays in all).
* picks, V = 128256 fp16 logits, B = 4 and 8, 64 rotating logits buffers: greedy_step /
  greedy_step_streams, sample_step / sample_step_streams (top_k 50, top_p 0.9, temperature 0.8) and
  the composed torch route of both streams picks.

Sessions (tok/s): bench.py's Llama-3-8B (random init, NF4 + double quant, fp16), batch 4, equal
prompt lengths, one model laid out by generation.prepare_for_decode; per repeat, interleaved, a
greedy DecodeSession and a greedy StreamSession.

--bench: `bench.py --gpus 1 --steps K --warmup W` as a process of its own per run, the parent tree
(P) and this tree (N) in the order P N P N P N.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from sample_times import graph_time_us  # noqa: E402  (scripts/ is sys.path[0])

V = 128256
PICK_COPIES = 64
ATTN_COPIES = 16
HQ, HKV, D = 32, 8, 128


@torch.inference_mode()
def attention_cases(emit, repeat):
    from quantizations_amd.layer_ops import decode_attention, decode_attention_streams

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    scale = 1.0 / math.sqrt(D)
    for B in (4, 8):
        for L, shape in ((512, "equal"), (4096, "equal"), (4096, "ragged")):
            q = (torch.randn(B, 1, HQ * D, device=dev, generator=g)).half()
            k = (torch.randn(B, 1, HKV * D, device=dev, generator=g)).half()
            v = (torch.randn(B, 1, HKV * D, device=dev, generator=g)).half()
            ang = torch.rand(B, 1, D // 2, device=dev, generator=g) * 6.0
            cos = torch.cat((ang.cos(), ang.cos()), -1).half()
            sin = torch.cat((ang.sin(), ang.sin()), -1).half()
            caches = [(torch.randn(B, HKV, L, D, device=dev, generator=g).half(),
                       torch.randn(B, HKV, L, D, device=dev, generator=g).half()) for _ in range(ATTN_COPIES)]
            long_p = L - 64
            ps = [long_p] * B if shape == "equal" else [long_p] + [40] * (B - 1)
            pos_streams = torch.tensor(ps, dtype=torch.int64, device=dev)
            mask = torch.ones((B, 1, 1, L), dtype=torch.bool, device=dev)   # keys up to the advancing position and past it
            arrive = torch.zeros(1, dtype=torch.int32, device=dev)
            shared_pos = [torch.tensor(long_p, dtype=torch.int64, device=dev) for _ in range(ATTN_COPIES)]
            row = {"case": "attention", "B": B, "L": L, "positions": shape, "p": ps[:2], "copies": ATTN_COPIES,
                   "shared_us": [], "streams_us": []}
            for _ in range(repeat):
                for p in shared_pos:
                    p.fill_(long_p)
                row["shared_us"].append(graph_time_us(
                    [lambda kc=kc, vc=vc, p=p: decode_attention(q, k, v, cos, sin, kc, vc, mask, p, arrive, HQ, scale)
                     for (kc, vc), p in zip(caches, shared_pos)]))
                row["streams_us"].append(graph_time_us(
                    [lambda kc=kc, vc=vc: decode_attention_streams(q, k, v, cos, sin, kc, vc, pos_streams, HQ, scale)
                     for kc, vc in caches]))
            torch.cuda.synchronize()
            assert all(int(p) < L for p in shared_pos)
            emit({k_: [round(x, 2) for x in v_] if k_.endswith("_us") else v_ for k_, v_ in row.items()})
            del caches
            torch.cuda.empty_cache()


@torch.inference_mode()
def pick_cases(emit, repeat):
    from quantizations_amd.layer_ops import greedy_step, greedy_step_streams, sample_step, sample_step_streams

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in (4, 8):
        logits = [(torch.randn(B, V, device=dev, generator=g) * 4).half() for _ in range(PICK_COPIES)]
        H = 4 * PICK_COPIES
        hist = torch.zeros((B, H), dtype=torch.int64, device=dev)
        pos1 = torch.zeros(1, dtype=torch.int64, device=dev)
        posB = torch.zeros(B, dtype=torch.int64, device=dev)
        live = torch.ones(B, dtype=torch.int32, device=dev)
        stop = torch.full((B,), -1, dtype=torch.int64, device=dev)
        limit = torch.full((B,), 1 << 40, dtype=torch.int64, device=dev)
        tok = torch.zeros(B, dtype=torch.int64, device=dev)
        U = torch.rand((B, H), device=dev, generator=g)
        T = torch.full((B,), 0.8, device=dev)
        P = torch.full((B,), 0.9, device=dev)
        K = torch.full((B,), 50, dtype=torch.int32, device=dev)
        routes = {
            "greedy_us": lambda lo: greedy_step(lo, hist, pos1, tok),
            "greedy_streams_us": lambda lo: greedy_step_streams(lo, hist, posB, live, stop, limit, tok),
            "greedy_streams_composed_us": lambda lo: greedy_step_streams(lo, hist, posB, live, stop, limit, tok,
                                                                         composed=True),
            "sample_us": lambda lo: sample_step(lo, hist, pos1, tok, T, K, P, U),
            "sample_streams_us": lambda lo: sample_step_streams(lo, hist, posB, live, stop, limit, tok, T, K, P, U),
            "sample_streams_composed_us": lambda lo: sample_step_streams(lo, hist, posB, live, stop, limit, tok, T, K,
                                                                         P, U, composed=True),
        }
        row = {"case": "pick", "V": V, "B": B, "dtype": "fp16", "copies": PICK_COPIES}
        row.update({name: [] for name in routes})
        for _ in range(repeat):
            for name, fn in routes.items():
                pos1.zero_(), posB.zero_()
                row[name].append(graph_time_us([lambda lo=lo, fn=fn: fn(lo) for lo in logits]))
        torch.cuda.synchronize()
        assert int(live.sum()) == B
        emit({k_: [round(x, 2) for x in v_] if k_.endswith("_us") else v_ for k_, v_ in row.items()})
        del logits
        torch.cuda.empty_cache()


def session_tok_s(cls, model, cfg, batch, steps, warmup, prompt):
    ids = torch.randint(0, cfg.vocab_size, (batch, prompt), generator=torch.Generator().manual_seed(1234)).cuda()
    sess = cls(model, batch, prompt + warmup + steps + 8)
    if cls.__name__ == "StreamSession":
        sess.prefill(ids, [prompt] * batch)
    else:
        sess.prefill(ids)
    for _ in range(warmup):
        sess.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sess.step()
    torch.cuda.synchronize()
    return batch * steps / (time.perf_counter() - t0)


def session_cases(emit, args):
    import bench
    from quantizations_amd.generation import DecodeSession, StreamSession, prepare_for_decode

    model, cfg = bench.build_model(args.layers, seed=0)
    counts = prepare_for_decode(model)
    runs = {"DecodeSession": [], "StreamSession": []}
    for _ in range(args.repeat):
        for cls in (DecodeSession, StreamSession):
            runs[cls.__name__].append(session_tok_s(cls, model, cfg, args.batch, args.steps, args.warmup, args.prompt))
    d, s = runs["DecodeSession"], runs["StreamSession"]
    spread = max(d) - min(d)
    smed = sorted(s)[len(s) // 2]
    emit({"case": "sessions", "model": "llama3-8b", "layers": cfg.num_hidden_layers, "batch": args.batch,
          "steps": args.steps, "prompt": args.prompt, "prepare_for_decode": counts,
          "tok_s": {k: [round(v, 2) for v in vs] for k, vs in runs.items()},
          "decode_session_spread_tok_s": round(spread, 2), "stream_session_median_tok_s": round(smed, 2),
          "stream_not_behind_by_more_than_the_spread": bool(smed >= min(d) - spread)})


def bench_cases(emit, args):
    """bench.py's line, one process per run: parent (P) and this tree (N) alternating."""
    trees = ([("P", os.path.abspath(args.parent))] if args.parent else []) + [("N", REPO)]
    runs = {name: [] for name, _ in trees}
    for _ in range(args.repeat):
        for name, root in trees:
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup",
                                  str(args.warmup)], cwd=root, capture_output=True, text=True, timeout=600, check=True)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
            runs[name].append(json.loads(line))
    key = next(k for k in ("tokens_per_s", "tok_s", "value", "score") if k in runs["N"][0])
    vals = {name: [round(float(r[key]), 3) for r in rs] for name, rs in runs.items()}
    row = {"case": "bench", "cmd": f"bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup}", "metric": key, **vals}
    if "P" in vals:
        n_med = sorted(vals["N"])[len(vals["N"]) // 2]
        row["N_median"] = n_med
        row["N_median_inside_P_min_max"] = bool(min(vals["P"]) <= n_med <= max(vals["P"]))
        row["N_median_not_below_P_min"] = bool(n_med >= min(vals["P"]))
    emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true", help="only the per-call times")
    ap.add_argument("--sessions", action="store_true", help="only the Llama-3-8B batch-4 sessions")
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "streams_times.txt"))
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    both = not (args.launches or args.sessions or args.bench)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if not both else "w") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if both or args.launches:
            attention_cases(emit, args.repeat)
            pick_cases(emit, args.repeat)
        if both or args.sessions:
            with torch.inference_mode():
                session_cases(emit, args)
        if args.bench:
            bench_cases(emit, args)


if __name__ == "__main__":
    main()
