#!/usr/bin/env python
"""Log-probabilities: what the logprobs launches cost beside the pick they follow.

  python scripts/logprobs_times.py                      # launches -> profiles/logprobs_times.txt
  python scripts/logprobs_times.py --picks --parent DIR # sample_times.py's per-call times, parent and this tree in turn
  python scripts/logprobs_times.py --bench --parent DIR # bench.py's line, parent and this tree in turn

Launches (us per call, scripts/sample_times.py's graph_time_us: COPIES calls over rotating logits
buffers captured back to back into one graph, replayed between two events; medians of three,
interleaved): V = 128256 fp16, (B, T) = (1, 1), (4, 1), (8, 1), (1, 4), (2, 8), n = 0, 5 and 20 top
entries; every row live (pos1 = pos0 + T).  Beside it: the pick the call follows on the same logits
(sample_step_streams with top-k 50, top-p 0.9, temperature 0.8; for T > 1
verify_sample_step_streams), the greedy pick (greedy_step_streams / verify_step_streams), and the
composed torch route (fp32 log_softmax + a stable sort; it scatters through a boolean mask, so it
runs eagerly between two events).  One more column times
the session form with no live row (pos1 = pos0): the workgroups leave before loading anything.

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
from verify_sample_times import pick_cases  # noqa: E402

COPIES = 16          # 0.25-4 MiB of logits per call, 4-64 MiB in rotation
V = 128256
SETTINGS = dict(temperature=0.8, top_k=50, top_p=0.9)


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
    from quantizations_amd.layer_ops import (greedy_step_streams, logprobs_streams, sample_step_streams,
                                             verify_sample_step_streams, verify_step_streams)

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    for B, T in ((1, 1), (4, 1), (8, 1), (1, 4), (2, 8)):
        logits = [(torch.randn(B * T, V, device=dev, generator=g) * 4).half() for _ in range(COPIES)]
        Ls = 64
        seq = torch.randint(0, V, (B, Ls), device=dev, generator=g)
        pos0 = torch.full((B,), 7, dtype=torch.int64, device=dev)
        pos1 = pos0 + T
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

        def pick(lo, greedy=False):
            a = (lo, st["hist"], st["pos"], st["live"], st["stop"], st["limit"], ptok)
            if T == 1:
                greedy_step_streams(*a) if greedy else sample_step_streams(*a, temp, topk, topp, U)
            else:
                verify_step_streams(*a, acc) if greedy else verify_sample_step_streams(*a, acc, temp, topk, topp, U)

        def reset():
            st["pos"].zero_()
            st["live"].fill_(1)

        picks = {"sampled_pick_us": [], "greedy_pick_us": []}
        rows = []
        for n in (0, 5, 20):
            lp = torch.full((B, Ls), float("nan"), device=dev)
            ti = torch.full((B, Ls, n), -1, dtype=torch.int32, device=dev) if n else None
            tl = torch.full((B, Ls, n), float("nan"), device=dev) if n else None
            rows.append((n, lp, ti, tl, {"logprobs_us": [], "composed_eager_us": [], "not_live_us": []}))
        for _ in range(repeat):
            reset()
            picks["sampled_pick_us"].append(graph_time_us([lambda lo=lo: pick(lo) for lo in logits]))
            reset()
            picks["greedy_pick_us"].append(graph_time_us([lambda lo=lo: pick(lo, True) for lo in logits]))
            for n, lp, ti, tl, out in rows:
                def call(lo, p1=pos1, composed=False):
                    logprobs_streams(lo, seq, pos0, p1, lp, ti, tl, T=T, composed=composed)
                out["logprobs_us"].append(graph_time_us([lambda lo=lo: call(lo) for lo in logits]))
                out["not_live_us"].append(graph_time_us([lambda lo=lo: call(lo, pos0) for lo in logits]))
                out["composed_eager_us"].append(_eager_time_us([lambda lo=lo: call(lo, composed=True) for lo in logits[:4]]))
        for n, lp, ti, tl, out in rows:
            row = {"case": "launch", "V": V, "B": B, "T": T, "ntop": n, "dtype": "fp16", "copies": COPIES, **out, **picks}
            m = _median(out["logprobs_us"])
            row["logprobs_over_sampled_pick"] = round(m / _median(picks["sampled_pick_us"]), 3)
            row["logprobs_over_greedy_pick"] = round(m / _median(picks["greedy_pick_us"]), 3)
            row["composed_over_logprobs"] = round(_median(out["composed_eager_us"]) / m, 2)
            emit({k: [round(x, 2) for x in v] if k.endswith("_us") else v for k, v in row.items()})
        del logits
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true", help="only the per-call times")
    ap.add_argument("--picks", action="store_true", help="only sample_times.py's per-call times (with --parent: both trees)")
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "logprobs_times.txt"))
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    default = not (args.launches or args.picks or args.bench)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w" if default else "a") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if default or args.launches:
            launch_cases(emit, args.repeat)
        if args.picks:
            pick_cases(emit, args)
        if args.bench:
            bench_cases(emit, args)


if __name__ == "__main__":
    main()
