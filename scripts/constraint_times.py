#!/usr/bin/env python
"""Constrained decoding: what the constrain launch and the advance cost beside the pick they surround,
and what they add to a step.

  python scripts/constraint_times.py                      # launches + sessions -> profiles/constraint_times.txt
  python scripts/constraint_times.py --launches
  python scripts/constraint_times.py --sessions --repeat 3
  python scripts/constraint_times.py --picks --parent DIR # sample_times.py's per-call times, parent and this tree in turn
  python scripts/constraint_times.py --bench --parent DIR # bench.py's line, parent and this tree in turn

Launches (us per call, scripts/sample_times.py's graph_time_us: COPIES calls over rotating logits
buffers captured back to back into one graph, replayed between two events; medians of three,
interleaved): V = 128256 fp16, (B, T) = (1, 1), (4, 1), (8, 1), (1, 4), (2, 8).  The automaton has 64
states over 256 token classes; every stream stands in a state that refuses about 99 % of the
vocabulary ("tight": nearly every vector is stored) or in one that refuses nothing ("open": nothing is
stored).  Variants: the automaton alone, the automaton with 300 bias entries per stream, the host mask
alone (T = 1; half the bits set), and the advance alone (one emitted column per stream).  Beside them:
every constrain time is that of a graph of "restore the rows, then constrain" less the restore alone
(`restore_us`, one copy of the B T rows): the launch writes in place and a masked row stores nothing
the second time, so a replay without the restore would not pay for the stores.  Beside them: the pick
the launch precedes on the same logits (sample_step_streams with top-k 50, top-p 0.9,
temperature 0.8; for T > 1 verify_sample_step_streams) and the greedy pick; profiles/
logits_process_times.txt has process_logits at n = 1024 on the same shapes.

Sessions: bench.py's Llama-3-8B (random init, NF4 + double quant, fp16), B = 1.  Per repeat,
interleaved: the replayed step of a sampled StreamSession without and with a constraint (an automaton
whose every state allows a random half of the vocabulary, so the stream never retires), and of
SpeculativeSession(sample=True) at T = 4 without and with it (ms per step).

--picks / --bench: scripts/verify_sample_times.py's pick_cases and scripts/streams_times.py's
bench_cases: the parent tree (P) and this tree (N) in the order P N P N P N.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sample_times import graph_time_us  # noqa: E402  (scripts/ is sys.path[0])
from streams_times import bench_cases  # noqa: E402
from verify_sample_times import _timed_steps, pick_cases  # noqa: E402

COPIES = 16
V = 128256
STATES, CLASSES, NBIAS = 64, 256, 300
SETTINGS = dict(temperature=0.8, top_k=50, top_p=0.9)


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _tables(rng):
    """Tables straight from arrays (no reachability check: state 0 is tight, state 1 open, the rest random)."""
    from quantizations_amd.constraints import TokenAutomaton

    class_of = rng.integers(0, CLASSES, V)
    nxt = rng.integers(0, STATES, (STATES, CLASSES))
    nxt[2:][rng.random((STATES - 2, CLASSES)) < 0.5] = -1
    nxt[0] = -1
    nxt[0, :3] = 0            # 3 of 256 classes: about 1 % of the vocabulary stays
    nxt[1] = 1
    return TokenAutomaton(class_of, nxt, starts=())


@torch.inference_mode()
def launch_cases(emit, repeat):
    from quantizations_amd.layer_ops import (constrain_logits, constraint_advance, greedy_step_streams,
                                              sample_step_streams, verify_sample_step_streams, verify_step_streams)

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    auto = _tables(rng)
    tables = auto.to(dev)
    keep = np.flatnonzero(auto.next[0, auto.class_of] >= 0)
    for B, T in ((1, 1), (4, 1), (8, 1), (1, 4), (2, 8)):
        logits = [(torch.randn(B * T, V, device=dev, generator=g) * 4).half() for _ in range(COPIES)]
        state = {"tight": torch.zeros(B, dtype=torch.int32, device=dev), "open": torch.ones(B, dtype=torch.int32, device=dev)}
        # drafts the tight state allows (it loops), so every row of the window is masked
        tok = torch.from_numpy(rng.choice(keep, (B, T))).to(dev)
        bias_ids = torch.from_numpy(np.stack([rng.permutation(V)[:NBIAS] for _ in range(B)]).astype(np.int32)).to(dev)
        bias_vals = torch.randn((B, NBIAS), device=dev, generator=g)
        bias_n = torch.full((B,), NBIAS, dtype=torch.int32, device=dev)
        mask = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (B, (V + 31) // 32)).astype(np.int32)).to(dev)
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
        seq = torch.from_numpy(rng.choice(keep, (B, 64))).to(dev)
        p0, p1 = torch.full((B,), 10, dtype=torch.int64, device=dev), torch.full((B,), 11, dtype=torch.int64, device=dev)
        adv_state = torch.zeros(B, dtype=torch.int32, device=dev)

        def auto_only(lo, which):
            constrain_logits(lo, state=state[which], tok=tok if T > 1 else None, automaton=tables, T=T)

        def auto_bias(lo, which):
            constrain_logits(lo, state=state[which], tok=tok if T > 1 else None, automaton=tables, bias_ids=bias_ids,
                             bias_vals=bias_vals, bias_n=bias_n, T=T)

        def sampled(lo):
            if T == 1:
                sample_step_streams(lo, st["hist"], st["pos"], st["live"], st["stop"], st["limit"], ptok, temp, topk, topp, U)
            else:
                verify_sample_step_streams(lo, st["hist"], st["pos"], st["live"], st["stop"], st["limit"], ptok, acc, temp,
                                           topk, topp, U)

        def greedy(lo):
            if T == 1:
                greedy_step_streams(lo, st["hist"], st["pos"], st["live"], st["stop"], st["limit"], ptok)
            else:
                verify_step_streams(lo, st["hist"], st["pos"], st["live"], st["stop"], st["limit"], ptok, acc)

        fresh = [lo.clone() for lo in logits]
        cases = {"automaton_tight_us": lambda lo: auto_only(lo, "tight"), "automaton_open_us": lambda lo: auto_only(lo, "open"),
                 "automaton_tight_bias300_us": lambda lo: auto_bias(lo, "tight"),
                 "automaton_open_bias300_us": lambda lo: auto_bias(lo, "open")}
        if T == 1:
            cases["host_mask_us"] = lambda lo: constrain_logits(lo, mask=mask)
        row = {"case": "launch", "V": V, "B": B, "T": T, "dtype": "fp16", "copies": COPIES, "states": STATES,
               "classes": CLASSES, "refused_by_tight": round(1 - keep.size / V, 4)}
        row.update({k: [] for k in cases})
        row.update({"advance_us": [], "sampled_pick_us": [], "greedy_pick_us": []})
        row["restore_us"] = []

        def restored(f):      # the launches write in place: every call starts from the model's rows
            def run(lo, src):
                lo.copy_(src)
                f(lo)
            return [lambda lo=lo, src=src: run(lo, src) for lo, src in zip(logits, fresh)]

        for _ in range(repeat):
            base = graph_time_us(restored(lambda lo: None))
            row["restore_us"].append(base)
            for k, f in cases.items():
                row[k].append(graph_time_us(restored(f)) - base)
            for lo, src in zip(logits, fresh):
                lo.copy_(src)
            row["advance_us"].append(graph_time_us([lambda: constraint_advance(adv_state, seq, p0, p1, tables)] * COPIES))
            st["pos"].zero_()
            row["sampled_pick_us"].append(graph_time_us([lambda lo=lo: sampled(lo) for lo in logits]))
            st["pos"].zero_()
            row["greedy_pick_us"].append(graph_time_us([lambda lo=lo: greedy(lo) for lo in logits]))
        row["tight_over_sampled_pick"] = round(_median(row["automaton_tight_us"]) / _median(row["sampled_pick_us"]), 3)
        row["tight_over_greedy_pick"] = round(_median(row["automaton_tight_us"]) / _median(row["greedy_pick_us"]), 3)
        emit({k: [round(x, 2) for x in v] if k.endswith("_us") else v for k, v in row.items()})
        del logits, fresh
        torch.cuda.empty_cache()


def session_cases(emit, args):
    import bench
    from quantizations_amd.constraints import TokenAutomaton
    from quantizations_amd.generation import SpeculativeSession, StreamSession, prepare_for_decode

    model, cfg = bench.build_model(args.layers, seed=0)
    counts = prepare_for_decode(model)
    ids = torch.randint(0, cfg.vocab_size, (1, args.prompt), generator=torch.Generator().manual_seed(1234)).cuda()
    n = args.steps
    room = 4 * (args.prompt + args.warmup + n + 16)
    rng = np.random.default_rng(1)
    nxt = rng.integers(0, STATES, (STATES, CLASSES))
    nxt[rng.random((STATES, CLASSES)) < 0.5] = -1
    auto = TokenAutomaton(rng.integers(0, CLASSES, cfg.vocab_size), nxt, starts=(0,))

    def open_session(cls, constrained, **kw):
        sess = cls(model, 1, room, constraint=auto if constrained else None, **kw)
        sess.set_sampling(**SETTINGS)
        sess.seed(0)
        sess.prefill(ids, [args.prompt], **(dict(constraint_start=0) if constrained else {}))
        return sess

    kinds = [("StreamSession", StreamSession, {}, 1), ("SpeculativeSession_T=4", SpeculativeSession,
                                                       dict(draft_tokens=3, sample=True), 4)]
    ms = {f"{name}_{p}": [] for name, _, _, _ in kinds for p in ("plain", "constrained")}
    for _ in range(args.repeat):
        for name, cls, kw, T in kinds:
            for p in ("plain", "constrained"):
                sess = open_session(cls, p == "constrained", **kw)
                _timed_steps(sess, args.warmup)
                ms[f"{name}_{p}"].append(1e3 * _timed_steps(sess, n // T) / (n // T))
                if p == "constrained":
                    assert int(sess.constraint_state[0]) >= 0
    out = {"case": "sessions", "model": "llama3-8b", "layers": cfg.num_hidden_layers, "batch": 1, "tokens": n,
           "prompt": args.prompt, "cache_slots": room, **SETTINGS, "states": STATES, "classes": CLASSES,
           "prepare_for_decode": counts}
    for name, _, _, _ in kinds:
        a, b = ms[f"{name}_plain"], ms[f"{name}_constrained"]
        out[name] = {"plain_ms_per_step": [round(x, 4) for x in a], "constrained_ms_per_step": [round(x, 4) for x in b],
                     "added_us": round(1e3 * (_median(b) - _median(a)), 2),
                     "constrained_median_inside_plain_min_max": bool(min(a) <= _median(b) <= max(a))}
    emit(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true", help="only the per-call times")
    ap.add_argument("--sessions", action="store_true", help="only the Llama-3-8B batch-1 sessions")
    ap.add_argument("--picks", action="store_true", help="only sample_times.py's per-call times (with --parent: both trees)")
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "constraint_times.txt"))
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
