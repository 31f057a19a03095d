#!/usr/bin/env python
"""Sampled speculative decoding: what the pick that accepts drafts costs, and what a sampled window
costs beside one-token sampled steps.

  python scripts/verify_sample_times.py                      # launches + sessions -> profiles/verify_sample_times.txt
  python scripts/verify_sample_times.py --launches
  python scripts/verify_sample_times.py --sessions --repeat 3
  python scripts/verify_sample_times.py --picks --parent DIR # sample_times.py's per-call times, parent and this tree in turn
  python scripts/verify_sample_times.py --bench --parent DIR # bench.py's line, parent and this tree in turn

Launches (us per call, scripts/sample_times.py's graph_time_us: COPIES calls over rotating logits
buffers captured back to back into one graph, replayed between two events; three repeats,
interleaved): V = 128256 fp16, top-k 50, top-p 0.9, temperature 0.8, (B, T) = (1, 4), (1, 8), (2, 8),
(4, 4): one verify_sample_step_streams call (six launches) beside T successive sample_step_streams
calls at B rows (5 T launches, the same work per row) and one verify_step_streams call (the greedy
pick of the same window).

Sessions: bench.py's Llama-3-8B (random init, NF4 + double quant, fp16), B = 1, a 1472-slot cache.
Per repeat, interleaved: the replayed step of a sampled StreamSession, and for T = 2, 4, 8 of a greedy
SpeculativeSession and of SpeculativeSession(sample=True) (ms per step; the ratio to the sampled
StreamSession step minus one is the number of extra tokens a step must emit to break even).  A
random-init model has no acceptance rate of its own, so none is reported.

--picks: `scripts/sample_times.py --launches` as a process of its own per run, the parent tree (P)
and this tree (N) in the order P N P N P N: the existing picks gained a run-time operand.
--bench: scripts/streams_times.py's bench_cases.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from sample_times import graph_time_us  # noqa: E402  (scripts/ is sys.path[0])
from streams_times import bench_cases  # noqa: E402

COPIES = 16          # 1-4 MiB of logits per call: 16-64 MiB in rotation, past the 4 MiB L2
V = 128256
SETTINGS = dict(temperature=0.8, top_k=50, top_p=0.9)


@torch.inference_mode()
def launch_cases(emit, repeat):
    from quantizations_amd.layer_ops import sample_step_streams, verify_sample_step_streams, verify_step_streams

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    H = 1 << 15                                           # every call advances pos by at least one
    for B, T in ((1, 4), (1, 8), (2, 8), (4, 4)):
        logits = [(torch.randn(B * T, V, device=dev, generator=g) * 4).half() for _ in range(COPIES)]
        temp = torch.full((B,), SETTINGS["temperature"], device=dev)
        topk = torch.full((B,), SETTINGS["top_k"], dtype=torch.int32, device=dev)
        topp = torch.full((B,), SETTINGS["top_p"], device=dev)
        U = torch.rand((B, H), device=dev, generator=g)

        def state():
            return dict(hist=torch.zeros((B, H), dtype=torch.int64, device=dev),
                        pos=torch.zeros(B, dtype=torch.int64, device=dev), live=torch.ones(B, dtype=torch.int32, device=dev),
                        stop=torch.full((B,), -1, dtype=torch.int64, device=dev),
                        limit=torch.full((B,), 1 << 40, dtype=torch.int64, device=dev))

        a, b, c = state(), state(), state()
        tok = torch.zeros((B, T), dtype=torch.int64, device=dev)
        tok1 = torch.zeros(B, dtype=torch.int64, device=dev)
        acc = torch.zeros(B, dtype=torch.int32, device=dev)

        def sampled(lo):
            verify_sample_step_streams(lo, a["hist"], a["pos"], a["live"], a["stop"], a["limit"], tok, acc, temp, topk,
                                       topp, U)

        def sequential(lo):
            rows = lo.view(B, T, V)
            for i in range(T):
                sample_step_streams(rows[:, i], b["hist"], b["pos"], b["live"], b["stop"], b["limit"], tok1, temp, topk,
                                    topp, U)

        def greedy(lo):
            verify_step_streams(lo, c["hist"], c["pos"], c["live"], c["stop"], c["limit"], tok, acc)

        row = {"case": "pick", "V": V, "B": B, "T": T, "dtype": "fp16", "copies": COPIES, **SETTINGS,
               "verify_sample_us": [], "sequential_sample_us": [], "verify_greedy_us": []}
        for _ in range(repeat):
            for name, fn in (("verify_sample_us", sampled), ("sequential_sample_us", sequential), ("verify_greedy_us", greedy)):
                for s in (a, b, c):
                    s["pos"].zero_()
                row[name].append(graph_time_us([lambda lo=lo, fn=fn: fn(lo) for lo in logits]))
        torch.cuda.synchronize()
        med = {n: sorted(row[n])[len(row[n]) // 2] for n in ("verify_sample_us", "sequential_sample_us", "verify_greedy_us")}
        row["verify_sample_over_sequential"] = round(med["verify_sample_us"] / med["sequential_sample_us"], 3)
        row["verify_sample_minus_greedy_us"] = round(med["verify_sample_us"] - med["verify_greedy_us"], 2)
        emit({k: [round(x, 2) for x in v] if k.endswith("_us") and isinstance(v, list) else v for k, v in row.items()})
        del logits
        torch.cuda.empty_cache()


def _timed_steps(sess, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sess.step()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def session_cases(emit, args):
    import bench
    from quantizations_amd.generation import SpeculativeSession, StreamSession, prepare_for_decode

    model, cfg = bench.build_model(args.layers, seed=0)
    counts = prepare_for_decode(model)
    ids = torch.randint(0, cfg.vocab_size, (1, args.prompt), generator=torch.Generator().manual_seed(1234)).cuda()
    n = args.steps
    room = 8 * (args.prompt + args.warmup + n + 16)       # one cache length for every session: 8 tokens a step fit

    def open_session(cls, sampled, **kw):
        sess = cls(model, 1, room, **kw)
        if sampled:
            sess.set_sampling(**SETTINGS)
            sess.seed(0)
        sess.prefill(ids, [args.prompt])
        return sess

    names = ["StreamSession_sampled"] + [f"T={T}_{k}" for T in (2, 4, 8) for k in ("greedy", "sampled")]
    ms = {k: [] for k in names}
    for _ in range(args.repeat):
        sess = open_session(StreamSession, True)
        _timed_steps(sess, args.warmup)
        ms["StreamSession_sampled"].append(1e3 * _timed_steps(sess, n) / n)
        for T in (2, 4, 8):
            for kind in ("greedy", "sampled"):
                sess = open_session(SpeculativeSession, kind == "sampled", draft_tokens=T - 1, sample=kind == "sampled")
                _timed_steps(sess, args.warmup)
                ms[f"T={T}_{kind}"].append(1e3 * _timed_steps(sess, n // T) / (n // T))
    med = {k: sorted(v)[args.repeat // 2] for k, v in ms.items()}
    base = med["StreamSession_sampled"]
    out = {"case": "sessions", "model": "llama3-8b", "layers": cfg.num_hidden_layers, "batch": 1, "tokens": n,
           "prompt": args.prompt, "cache_slots": room, **SETTINGS, "prepare_for_decode": counts,
           "StreamSession_sampled_ms_per_step": [round(x, 4) for x in ms["StreamSession_sampled"]]}
    for T in (2, 4, 8):
        s, g = med[f"T={T}_sampled"], med[f"T={T}_greedy"]
        out[f"T={T}"] = {"sampled_ms_per_step": [round(x, 4) for x in ms[f"T={T}_sampled"]],
                         "greedy_ms_per_step": [round(x, 4) for x in ms[f"T={T}_greedy"]],
                         "sampled_minus_greedy_ms": round(s - g, 4), "step_ratio": round(s / base, 3),
                         "extra_tokens_to_break_even": round(s / base - 1, 3)}
    emit(out)


def pick_cases(emit, args):
    """scripts/sample_times.py --launches, one process per run: parent (P) and this tree (N) alternating."""
    trees = ([("P", os.path.abspath(args.parent))] if args.parent else []) + [("N", REPO)]
    runs = {name: [] for name, _ in trees}
    for _ in range(args.repeat):
        for name, root in trees:
            with tempfile.NamedTemporaryFile(suffix=".txt") as tmp:
                subprocess.run([sys.executable, os.path.join("scripts", "sample_times.py"), "--launches", "--out", tmp.name],
                               cwd=root, capture_output=True, text=True, timeout=600, check=True)
                runs[name].append([json.loads(ln) for ln in open(tmp.name) if ln.startswith("{")])
    for i, first in enumerate(runs["N"][0]):
        row = {k: v for k, v in first.items() if not k.endswith("_us")}
        for key in (k for k in first if k.endswith("_us")):
            for name in runs:
                row[f"{name}_{key}"] = [r[i][key] for r in runs[name]]
            if "P" in runs:
                n_med = sorted(row[f"N_{key}"])[args.repeat // 2]
                row[f"{key}_N_median_inside_P_min_max"] = bool(min(row[f"P_{key}"]) <= n_med <= max(row[f"P_{key}"]))
        emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true", help="only the per-call times of the picks")
    ap.add_argument("--sessions", action="store_true", help="only the Llama-3-8B batch-1 sessions")
    ap.add_argument("--picks", action="store_true", help="only sample_times.py's per-call times (with --parent: both trees)")
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "verify_sample_times.txt"))
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    both = not (args.launches or args.sessions or args.picks or args.bench)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if not both else "w") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if both or args.launches:
            launch_cases(emit, args.repeat)
        if both or args.sessions:
            with torch.inference_mode():
                session_cases(emit, args)
        if args.picks:
            pick_cases(emit, args)
        if args.bench:
            bench_cases(emit, args)


if __name__ == "__main__":
    main()
