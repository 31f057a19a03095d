#!/usr/bin/env python
"""Speculative greedy decoding: what a verify window costs beside one-token steps.

  python scripts/verify_times.py                      # launches + sessions, written to profiles/verify_times.txt
  python scripts/verify_times.py --launches           # only the attention launches
  python scripts/verify_times.py --sessions --repeat 3
  python scripts/verify_times.py --bench --parent DIR # bench.py's line, this tree and a built parent tree in turn

Per-call times (us), as scripts/streams_times.py takes them: COPIES calls over rotating caches are
captured back to back into one graph, which is replayed between two events; three repeats,
interleaved.  Llama-3-8B heads (Hq 32, Hkv 8, D 128, fp16), B = 1, the window starting at L - 64 for
L = 512 and 4096, T = 2, 4, 8: one decode_attention_verify call beside T successive
decode_attention_streams calls at positions p, p + 1, ... (the kernel this tree shares with its
parent, instruction for instruction).

Sessions: bench.py's Llama-3-8B (random init, NF4 + double quant, fp16), B = 1, one model laid out
by generation.prepare_for_decode.  Per repeat, interleaved: the replayed step of a StreamSession and
of a SpeculativeSession with T = 2, 4, 8 (ms per step; ratio - 1 is the number of extra tokens a step
must emit to break even), then tokens per second of that SpeculativeSession under a replay drafter
(every draft right: the ceiling) and a null drafter (no draft right: the floor).  A random-init model
has no acceptance rate of its own, so none is reported.

--bench: `bench.py --gpus 1 --steps K --warmup W` as a process of its own per run, the parent tree
(P) and this tree (N) in the order P N P N P N (scripts/streams_times.py's bench_cases).
"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from sample_times import graph_time_us  # noqa: E402  (scripts/ is sys.path[0])
from streams_times import bench_cases  # noqa: E402

ATTN_COPIES = 16
HQ, HKV, D = 32, 8, 128


@torch.inference_mode()
def attention_cases(emit, repeat):
    from quantizations_amd.layer_ops import decode_attention_streams, decode_attention_verify

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    scale = 1.0 / math.sqrt(D)
    for L in (512, 4096):
        caches = [(torch.randn(1, HKV, L, D, device=dev, generator=g).half(),
                   torch.randn(1, HKV, L, D, device=dev, generator=g).half()) for _ in range(ATTN_COPIES)]
        for T in (2, 4, 8):
            q = torch.randn(1, T, HQ * D, device=dev, generator=g).half()
            k = torch.randn(1, T, HKV * D, device=dev, generator=g).half()
            v = torch.randn(1, T, HKV * D, device=dev, generator=g).half()
            ang = torch.rand(1, T, D // 2, device=dev, generator=g) * 6.0
            cos = torch.cat((ang.cos(), ang.cos()), -1).half()
            sin = torch.cat((ang.sin(), ang.sin()), -1).half()
            p0 = L - 64
            pos = torch.tensor([p0], dtype=torch.int64, device=dev)
            each = [torch.tensor([p0 + i], dtype=torch.int64, device=dev) for i in range(T)]

            def sequential(kc, vc):
                for i in range(T):
                    decode_attention_streams(q[:, i:i + 1], k[:, i:i + 1], v[:, i:i + 1], cos[:, i:i + 1],
                                             sin[:, i:i + 1], kc, vc, each[i], HQ, scale)

            row = {"case": "attention", "B": 1, "T": T, "L": L, "p": p0, "copies": ATTN_COPIES,
                   "verify_us": [], "sequential_streams_us": []}
            for _ in range(repeat):
                row["verify_us"].append(graph_time_us(
                    [lambda kc=kc, vc=vc: decode_attention_verify(q, k, v, cos, sin, kc, vc, pos, HQ, scale)
                     for kc, vc in caches]))
                row["sequential_streams_us"].append(graph_time_us(
                    [lambda kc=kc, vc=vc: sequential(kc, vc) for kc, vc in caches]))
            torch.cuda.synchronize()
            med = {n: sorted(row[n])[len(row[n]) // 2] for n in ("verify_us", "sequential_streams_us")}
            row["verify_over_sequential"] = round(med["verify_us"] / med["sequential_streams_us"], 3)
            emit({k_: [round(x, 2) for x in v_] if k_.endswith("_us") else v_ for k_, v_ in row.items()})
        del caches
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

    class Null(SpeculativeSession):
        def _draft(self):
            super()._draft()
            self.tok[:, 1:] = (self.tok[:, :1] + 1) % self.model.config.vocab_size

    class Replay(SpeculativeSession):
        known = None

        def _draft(self):
            self.pos_ids.copy_(self.pos[:, None] + torch.arange(self.T, device=self.device)[None, :])
            self.tok[:, 1:] = self.known.gather(1, self.pos_ids[:, 1:].clamp(max=self.known.shape[1] - 1)).clamp(min=0)

    model, cfg = bench.build_model(args.layers, seed=0)
    counts = prepare_for_decode(model)
    ids = torch.randint(0, cfg.vocab_size, (1, args.prompt), generator=torch.Generator().manual_seed(1234)).cuda()
    n = args.steps                       # tokens the timed steps emit
    room = 8 * (args.prompt + args.warmup + n + 16)   # one cache length for every session: 8 tokens a step fit

    def open_session(cls, T=None, known=None, tokens=None):
        kw = {} if T is None else {"draft_tokens": T - 1}
        sess = cls(model, 1, room, **kw)
        if known is not None:
            sess.known = known
        sess.prefill(ids, [args.prompt], max_new_tokens=tokens)
        return sess

    rows = {"StreamSession": {"ms_per_step": []}}
    for T in (2, 4, 8):
        rows[f"T={T}"] = {"ms_per_step": [], "replay_tok_s": [], "null_tok_s": [], "replay_steps": [], "null_steps": []}
    for _ in range(args.repeat):
        sess = open_session(StreamSession)
        _timed_steps(sess, args.warmup)
        rows["StreamSession"]["ms_per_step"].append(1e3 * _timed_steps(sess, n) / n)
        for T in (2, 4, 8):
            r = rows[f"T={T}"]
            sess = open_session(SpeculativeSession, T)         # the n-gram drafter: up to T tokens a step
            _timed_steps(sess, args.warmup)
            r["ms_per_step"].append(1e3 * _timed_steps(sess, n // T) / (n // T))
            total = args.warmup + n + 1                         # prefill's token, warm-up steps, n timed tokens
            null = open_session(Null, T, tokens=total)
            _timed_steps(null, args.warmup)
            dt = _timed_steps(null, n)
            assert not bool(null.alive().any())
            st = null.stats()
            r["null_tok_s"].append(n / dt), r["null_steps"].append(int(st["steps"][0]))
            rep = open_session(Replay, T, known=null._hist_full.clone(), tokens=total)
            w = math.ceil(args.warmup / T)
            _timed_steps(rep, w)
            left = total - 1 - int(rep.stats()["tokens"][0])
            k = math.ceil(left / T)
            dt = _timed_steps(rep, k)
            assert not bool(rep.alive().any()) and torch.equal(rep.hist[:, :args.prompt + total], null.hist[:, :args.prompt + total])
            r["replay_tok_s"].append(left / dt), r["replay_steps"].append(k)
    base = sorted(rows["StreamSession"]["ms_per_step"])[args.repeat // 2]
    out = {"case": "sessions", "model": "llama3-8b", "layers": cfg.num_hidden_layers, "batch": 1, "tokens": n,
           "prompt": args.prompt, "prepare_for_decode": counts,
           "StreamSession_ms_per_step": [round(x, 4) for x in rows["StreamSession"]["ms_per_step"]],
           "StreamSession_tok_s": round(1e3 / base, 2)}
    for T in (2, 4, 8):
        r = rows[f"T={T}"]
        med = sorted(r["ms_per_step"])[args.repeat // 2]
        out[f"T={T}"] = {"ms_per_step": [round(x, 4) for x in r["ms_per_step"]],
                         "step_ratio": round(med / base, 3), "extra_tokens_to_break_even": round(med / base - 1, 3),
                         "replay_tok_s": [round(x, 2) for x in r["replay_tok_s"]], "replay_steps": r["replay_steps"],
                         "null_tok_s": [round(x, 2) for x in r["null_tok_s"]], "null_steps": r["null_steps"]}
    emit(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true", help="only the attention launches")
    ap.add_argument("--sessions", action="store_true", help="only the Llama-3-8B batch-1 sessions")
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "verify_times.txt"))
    ap.add_argument("--layers", type=int, default=0)
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
        if both or args.sessions:
            with torch.inference_mode():
                session_cases(emit, args)
        if args.bench:
            bench_cases(emit, args)


if __name__ == "__main__":
    main()
