#!/usr/bin/env python
"""The paged KV cache: what each paged attention launch costs beside its contiguous twin, and what
kv_pages / prefix_cache / fork do to a session.

  python scripts/paged_attention_times.py                      # kernel + sessions -> profiles/paged_attention_times.txt
  python scripts/paged_attention_times.py --kernel
  python scripts/paged_attention_times.py --sessions --repeat 3
  python scripts/paged_attention_times.py --bench --parent DIR # bench.py's line, parent and this tree in turn

Kernel (us per call; COPIES calls over rotating q / k / v buffers captured back to back into one graph
and replayed between two events, scripts/sample_times.py's graph_time_us; medians of three interleaved
repeats with their min and max): Llama-3-8B heads (Hq 32, Hkv 8, D 128, fp16).  The yardstick of every
paged launch is the contiguous launch in the same run on a cache of L = 128 NP; the pages are scrambled
over a pool of twice the needed size.
  decode   B = 4 / 8, L = 512 / 4096, every stream at L - 2 ("long") and one there, the rest at 40 ("mixed")
  verify   the same with T = 4
  prefill  B = 1, L = 8192: windows of 512 and 2048 rows from 0 and of 512 rows from 7680
"slower_than_spread": the paged median exceeds the twin's by more than the twin's own max - min.

Sessions: bench.py's Llama-3-8B (random init, NF4 + double quant, fp16), max_len 8192, prefill_chunk 512:
a StreamSession step at B = 4 with and without kv_pages (ms per replayed step); admit() of a 2048-token
prompt whose first 1920 tokens are resident against the same admit with prefix_cache=False (ms to the
first token, peak MiB above the session); fork (ms); and the bytes the pool holds against the
StaticCache of the same batch x max_len for a stated mix of lengths.
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

HQ, HKV, D = 32, 8, 128
COPIES = 4
PAGE = 128


def _stats(xs):
    s = sorted(xs)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


def _pair(row, twin, paged):
    a, b = _stats(twin), _stats(paged)
    row["contiguous_us"], row["paged_us"] = a, b
    row["paged_minus_contiguous_us"] = round(b["median"] - a["median"], 2)
    row["slower_than_spread"] = bool(b["median"] - a["median"] > a["max"] - a["min"])
    return row


def _pools(B, NP, dev, g):
    """Pools of twice the needed pages and a table of scrambled, distinct pages."""
    P = 2 * B * NP
    kp = torch.randn(P, HKV, PAGE, D, device=dev, generator=g).half()
    vp = torch.randn(P, HKV, PAGE, D, device=dev, generator=g).half()
    table = torch.randperm(P, device=dev, generator=g)[:B * NP].to(torch.int32).view(B, NP).contiguous()
    return kp, vp, table


@torch.inference_mode()
def kernel_cases(emit, repeat):
    from quantizations_amd import layer_ops as lo

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    scale = D ** -0.5
    for T in (1, 4):
        for B in (4, 8):
            for L in (512, 4096):
                NP = L // PAGE
                kc = torch.randn(B, HKV, L, D, device=dev, generator=g).half()
                vc = torch.randn(B, HKV, L, D, device=dev, generator=g).half()
                kp, vp, table = _pools(B, NP, dev, g)
                qs = [torch.randn(B, T, HQ * D, device=dev, generator=g).half() for _ in range(COPIES)]
                ks = [torch.randn(B, T, HKV * D, device=dev, generator=g).half() for _ in range(COPIES)]
                vs = [torch.randn(B, T, HKV * D, device=dev, generator=g).half() for _ in range(COPIES)]
                ang = torch.rand(B, T, D // 2, device=dev, generator=g) * 6.0
                cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
                for mix in ("long", "mixed"):
                    pos = torch.full((B,), 40, dtype=torch.int64, device=dev)
                    pos[0 if mix == "mixed" else slice(None)] = L - 2 - T
                    if T == 1:
                        twin = [lambda i=i: lo.decode_attention_streams(qs[i], ks[i], vs[i], cos, sin, kc, vc, pos, HQ, scale)
                                for i in range(COPIES)]
                        paged = [lambda i=i: lo.decode_attention_paged(qs[i], ks[i], vs[i], cos, sin, kp, vp, table, pos, HQ,
                                                                       scale) for i in range(COPIES)]
                    else:
                        twin = [lambda i=i: lo.decode_attention_verify(qs[i], ks[i], vs[i], cos, sin, kc, vc, pos, HQ, scale)
                                for i in range(COPIES)]
                        paged = [lambda i=i: lo.decode_attention_verify_paged(qs[i], ks[i], vs[i], cos, sin, kp, vp, table,
                                                                              pos, HQ, scale) for i in range(COPIES)]
                    a, b = [], []
                    for _ in range(repeat):
                        a.append(graph_time_us(twin, reps=20))
                        b.append(graph_time_us(paged, reps=20))
                    emit(_pair({"case": "decode" if T == 1 else "verify", "B": B, "T": T, "L": L, "positions": mix,
                                "Hq": HQ, "Hkv": HKV, "D": D, "dtype": "fp16", "pool_pages": kp.shape[0]}, a, b))
                del kc, vc, kp, vp
                torch.cuda.empty_cache()
    L = 8192
    NP = L // PAGE
    kc = torch.randn(1, HKV, L, D, device=dev, generator=g).half()
    vc = torch.randn(1, HKV, L, D, device=dev, generator=g).half()
    kp, vp, table = _pools(1, NP, dev, g)
    for T, start in ((512, 0), (2048, 0), (512, 7680)):
        qs = [torch.randn(1, T, HQ * D, device=dev, generator=g).half() for _ in range(COPIES)]
        ks = [torch.randn(1, T, HKV * D, device=dev, generator=g).half() for _ in range(COPIES)]
        vs = [torch.randn(1, T, HKV * D, device=dev, generator=g).half() for _ in range(COPIES)]
        ang = torch.rand(1, T, D // 2, device=dev, generator=g) * 6.0
        cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
        pos = torch.tensor([start], dtype=torch.int64, device=dev)
        ln = torch.tensor([T], dtype=torch.int64, device=dev)
        twin = [lambda i=i: lo.prefill_attention(qs[i], ks[i], vs[i], cos, sin, kc, vc, pos, ln, HQ, scale)
                for i in range(COPIES)]
        paged = [lambda i=i: lo.prefill_attention_paged(qs[i], ks[i], vs[i], cos, sin, kp, vp, table, pos, ln, HQ, scale)
                 for i in range(COPIES)]
        a, b = [], []
        for _ in range(repeat):
            a.append(graph_time_us(twin, reps=5))
            b.append(graph_time_us(paged, reps=5))
        emit(_pair({"case": "prefill", "B": 1, "T": T, "start": start, "L": L, "Hq": HQ, "Hkv": HKV, "D": D,
                    "dtype": "fp16", "pool_pages": kp.shape[0]}, a, b))


def _timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def session_cases(emit, args):
    import bench
    from quantizations_amd.generation import StreamSession, prepare_for_decode

    model, cfg = bench.build_model(args.layers, seed=0)
    prepare_for_decode(model)
    gen = torch.Generator().manual_seed(1234)
    B, L, chunk = 4, 8192, 512
    NPS = L // PAGE
    ids = torch.randint(0, cfg.vocab_size, (B, 64), generator=gen).cuda()
    long_prompt = torch.randint(0, cfg.vocab_size, (2048,), generator=gen)

    def session(**kw):
        sess = StreamSession(model, B, L, prefill_chunk=chunk, **kw)
        sess.prefill(ids, [64] * B, max_new_tokens=[512, 2, 2, 512])
        for _ in range(4):
            sess.step()
        return sess

    # a replayed step, B = 4, with and without kv_pages
    ms = {"contiguous": [], "paged": []}
    for rep in range(args.repeat + 1):
        for name, kw in (("contiguous", {}), ("paged", {"kv_pages": 2 * B * NPS})):
            sess = session(**kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(64):
                sess.step()
            torch.cuda.synchronize()
            if rep:
                ms[name].append(1e3 * (time.perf_counter() - t0) / 64)
            del sess
            torch.cuda.empty_cache()
    emit({"case": "step", "model": "llama3-8b", "layers": cfg.num_hidden_layers, "batch": B, "max_len": L,
          "ms_per_step": {n: _stats(v) for n, v in ms.items()}})
    # admit() of a 2048-token prompt: 1920 tokens (15 pages) resident, against prefix_cache=False; then fork
    ms = {"shared_1920": [], "prefix_cache_off": [], "fork": []}
    mib = {"shared_1920": [], "prefix_cache_off": []}
    first = {}
    stats = None
    for rep in range(args.repeat + 1):
        for name, share in (("shared_1920", True), ("prefix_cache_off", False)):
            sess = session(kv_pages=B * NPS, prefix_cache=share)
            sess.admit(1, long_prompt, max_new_tokens=8)           # the donor: publishes 16 pages
            t, m = _timed(lambda: sess.admit(2, long_prompt, max_new_tokens=8))
            first[name] = int(sess.tok[2, 0])
            if rep:
                ms[name].append(t)
                mib[name].append(m)
            if share:
                t, _ = _timed(lambda: sess.fork(1, 2))
                if rep:
                    ms["fork"].append(t)
                stats = sess.page_stats()
            del sess
            torch.cuda.empty_cache()
    emit({"case": "admit", "model": "llama3-8b", "layers": cfg.num_hidden_layers, "batch": B, "prompt": 2048,
          "resident_tokens": 1920, "max_len": L, "prefill_chunk": chunk, "ms_to_first_token": {n: _stats(ms[n]) for n in mib},
          "peak_MiB_above_session": {n: _stats(v) for n, v in mib.items()}, "first_token": first,
          "fork_ms": _stats(ms["fork"])})
    # bytes: streams of 64 + 512, 2048 + 8 (forked: 16 shared pages), 2048 + 8 and 64 + 512 tokens at most
    static = 2 * cfg.num_hidden_layers * cfg.num_key_value_heads * (cfg.hidden_size // cfg.num_attention_heads) * L * 2 * B
    emit({"case": "bytes", "mix": "limits of 576, 2056, 2056 (a fork of the second: 16 pages shared) and 576 tokens",
          "page_stats": stats, "pool_held_MiB": round(stats["held"] * stats["bytes_per_page"] / 2 ** 20, 1),
          "static_cache_MiB": round(static / 2 ** 20, 1), "batch": B, "max_len": L})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true", help="only the per-call times")
    ap.add_argument("--sessions", action="store_true", help="only the Llama-3-8B sessions")
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "paged_attention_times.txt"))
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    both = not (args.kernel or args.sessions or args.bench)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if not both else "w") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if both or args.kernel:
            kernel_cases(emit, args.repeat)
        if both or args.sessions:
            with torch.inference_mode():
                session_cases(emit, args)
        if args.bench:
            bench_cases(emit, args)


if __name__ == "__main__":
    main()
