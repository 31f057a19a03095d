#!/usr/bin/env python
"""The logits processors: what the processing launch costs beside the pick it precedes, and what it
adds to a step.

  python scripts/logits_process_times.py                      # launches + sessions -> profiles/logits_process_times.txt
  python scripts/logits_process_times.py --launches
  python scripts/logits_process_times.py --sessions --repeat 3
  python scripts/logits_process_times.py --picks --parent DIR # sample_times.py's per-call times, parent and this tree in turn
  python scripts/logits_process_times.py --bench --parent DIR # bench.py's line, parent and this tree in turn

Launches (us per call, scripts/sample_times.py's graph_time_us: COPIES calls over rotating logits
buffers captured back to back into one graph, replayed between two events; medians of three,
interleaved): V = 128256 fp16, (B, T) = (1, 1), (4, 1), (8, 1), (1, 4), (2, 8), histories of n = 64, 1024
and 4096 random tokens in a hist of n + 16 columns, all five processors on (repetition 1.2, presence
0.3, frequency 0.2, no-repeat trigrams, a minimum length that holds the EOS back; the prompt is the
first half).  Beside it: the pick the launch precedes on the same logits (sample_step_streams with
top-k 50, top-p 0.9, temperature 0.8; for T > 1 verify_sample_step_streams) and the composed torch
route on the same inputs, which reads the history on the host and therefore runs eagerly between two
events.  `home` says where the hash table lives (LDS up to 16384 slots, i.e. hist_len + T <= 8192).  One
more case has a 20000-column history with n = 17000: the table in the workspace.

Sessions: bench.py's Llama-3-8B (random init, NF4 + double quant, fp16), B = 1.  Per repeat,
interleaved: the replayed step of a sampled StreamSession without and with all five processors, and
of SpeculativeSession(sample=True) at T = 4 without and with them (ms per step).

--picks / --bench: scripts/verify_sample_times.py's pick_cases and scripts/streams_times.py's
bench_cases: the parent tree (P) and this tree (N) in the order P N P N P N.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from sample_times import graph_time_us  # noqa: E402  (scripts/ is sys.path[0])
from streams_times import bench_cases  # noqa: E402
from verify_sample_times import _timed_steps, pick_cases  # noqa: E402

COPIES = 16          # 0.25-4 MiB of logits per call, 4-64 MiB in rotation
V = 128256
SETTINGS = dict(temperature=0.8, top_k=50, top_p=0.9)
PENALTIES = dict(repetition_penalty=1.2, presence_penalty=0.3, frequency_penalty=0.2, no_repeat_ngram_size=3,
                 min_new_tokens=1 << 20)


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _eager_time_us(fns, reps=3):
    for f in fns[:2]:
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        for f in fns:
            f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / (reps * len(fns))


@torch.inference_mode()
def launch_cases(emit, repeat):
    from quantizations_amd import _lib
    from quantizations_amd.layer_ops import process_logits, sample_step_streams, verify_sample_step_streams

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    shapes = [(B, T, n, n + 16) for B, T in ((1, 1), (4, 1), (8, 1), (1, 4), (2, 8)) for n in (64, 1024, 4096)]
    shapes.append((1, 1, 17000, 20000))
    for B, T, n, H in shapes:
        logits = [(torch.randn(B * T, V, device=dev, generator=g) * 4).half() for _ in range(COPIES)]
        hist = torch.randint(0, V, (B, H), device=dev, generator=g)
        pos = torch.full((B,), n - 1, dtype=torch.int64, device=dev)
        tok = torch.randint(0, V, (B, T), device=dev, generator=g)
        tok[:, 0] = hist[:, n - 1]
        par = dict(repetition_penalty=torch.full((B,), 1.2, device=dev), presence_penalty=torch.full((B,), 0.3, device=dev),
                   frequency_penalty=torch.full((B,), 0.2, device=dev),
                   no_repeat_ngram=torch.full((B,), 3, dtype=torch.int32, device=dev),
                   min_new_tokens=torch.full((B,), 1 << 20, dtype=torch.int64, device=dev),
                   prompt_len=torch.full((B,), n // 2, dtype=torch.int64, device=dev),
                   eos=torch.full((B,), 2, dtype=torch.int64, device=dev))
        temp = torch.full((B,), SETTINGS["temperature"], device=dev)
        topk = torch.full((B,), SETTINGS["top_k"], dtype=torch.int32, device=dev)
        topp = torch.full((B,), SETTINGS["top_p"], device=dev)
        PH = 1 << 15                                          # the pick's own state: every call advances pos
        U = torch.rand((B, PH), device=dev, generator=g)
        st = dict(hist=torch.zeros((B, PH), dtype=torch.int64, device=dev), pos=torch.zeros(B, dtype=torch.int64, device=dev),
                  live=torch.ones(B, dtype=torch.int32, device=dev), stop=torch.full((B,), -1, dtype=torch.int64, device=dev),
                  limit=torch.full((B,), 1 << 40, dtype=torch.int64, device=dev))
        ptok = torch.zeros((B, T), dtype=torch.int64, device=dev)
        acc = torch.zeros(B, dtype=torch.int32, device=dev)

        def process(lo, composed=False):
            process_logits(lo, hist, pos, tok if T > 1 else None, composed=composed, **par)

        def pick(lo):
            if T == 1:
                sample_step_streams(lo, st["hist"], st["pos"], st["live"], st["stop"], st["limit"], ptok, temp, topk, topp, U)
            else:
                verify_sample_step_streams(lo, st["hist"], st["pos"], st["live"], st["stop"], st["limit"], ptok, acc, temp,
                                           topk, topp, U)

        row = {"case": "launch", "V": V, "B": B, "T": T, "n": n, "hist_len": H, "dtype": "fp16", "copies": COPIES,
               "home": "lds" if _lib.lib.qz_logits_process_work_bytes(B, T, H) == 0 else "work",
               "process_us": [], "pick_us": [], "composed_eager_us": []}
        for _ in range(repeat):
            row["process_us"].append(graph_time_us([lambda lo=lo: process(lo) for lo in logits]))
            st["pos"].zero_()
            row["pick_us"].append(graph_time_us([lambda lo=lo: pick(lo) for lo in logits]))
            row["composed_eager_us"].append(_eager_time_us([lambda lo=lo: process(lo, True) for lo in logits[:4]], reps=1))
        row["process_over_pick"] = round(_median(row["process_us"]) / _median(row["pick_us"]), 3)
        emit({k: [round(x, 2) for x in v] if k.endswith("_us") else v for k, v in row.items()})
        del logits
        torch.cuda.empty_cache()


def session_cases(emit, args):
    import bench
    from quantizations_amd.generation import SpeculativeSession, StreamSession, prepare_for_decode

    model, cfg = bench.build_model(args.layers, seed=0)
    counts = prepare_for_decode(model)
    ids = torch.randint(0, cfg.vocab_size, (1, args.prompt), generator=torch.Generator().manual_seed(1234)).cuda()
    n = args.steps
    room = 4 * (args.prompt + args.warmup + n + 16)

    def open_session(cls, penalties, **kw):
        sess = cls(model, 1, room, **kw)
        sess.set_sampling(**SETTINGS)
        sess.seed(0)
        if penalties:
            sess.set_penalties(**PENALTIES)
        sess.prefill(ids, [args.prompt], stop=2)
        return sess

    kinds = [("StreamSession", StreamSession, {}, 1), ("SpeculativeSession_T=4", SpeculativeSession,
                                                       dict(draft_tokens=3, sample=True), 4)]
    ms = {f"{name}_{p}": [] for name, _, _, _ in kinds for p in ("plain", "processors")}
    for _ in range(args.repeat):
        for name, cls, kw, T in kinds:
            for p in ("plain", "processors"):
                sess = open_session(cls, p == "processors", **kw)
                _timed_steps(sess, args.warmup)
                ms[f"{name}_{p}"].append(1e3 * _timed_steps(sess, n // T) / (n // T))
    out = {"case": "sessions", "model": "llama3-8b", "layers": cfg.num_hidden_layers, "batch": 1, "tokens": n,
           "prompt": args.prompt, "cache_slots": room, **SETTINGS, **PENALTIES, "prepare_for_decode": counts}
    for name, _, _, _ in kinds:
        a, b = ms[f"{name}_plain"], ms[f"{name}_processors"]
        out[name] = {"plain_ms_per_step": [round(x, 4) for x in a], "processors_ms_per_step": [round(x, 4) for x in b],
                     "added_us": round(1e3 * (_median(b) - _median(a)), 2),
                     "processors_median_inside_plain_min_max": bool(min(a) <= _median(b) <= max(a))}
    emit(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true", help="only the per-call times")
    ap.add_argument("--sessions", action="store_true", help="only the Llama-3-8B batch-1 sessions")
    ap.add_argument("--picks", action="store_true", help="only sample_times.py's per-call times (with --parent: both trees)")
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "logits_process_times.txt"))
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
