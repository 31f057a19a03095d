#!/usr/bin/env python
"""The prefill attention: what the launch costs beside the library's two routes, and what
prefill_chunk does to a session's time to the first token and to its peak memory.

  python scripts/prefill_attention_times.py                      # kernel + sessions -> profiles/prefill_attention_times.txt
  python scripts/prefill_attention_times.py --kernel
  python scripts/prefill_attention_times.py --sessions --repeat 3
  python scripts/prefill_attention_times.py --bench --parent DIR # bench.py's line, parent and this tree in turn

Kernel (us per call; COPIES calls over rotating q / k / v / out buffers captured back to back into one
graph and replayed between two events, scripts/sample_times.py's graph_time_us; medians of three
interleaved repeats with their min and max): Llama-3-8B heads (Hq 32, Hkv 8, D 128, fp16), B = 1,
L = 8192, a window of 512 / 2048 / 8192 rows from position 0 and 512 rows from position 7680.
TFLOP/s are causal: 4 Hq D (sum of visible keys).  Beside it
  (a) F.scaled_dot_product_attention(is_causal=True, enable_gqa=True) on contiguous q / k / v of the
      same S: the library's flash kernel, start-0 windows only (no rotary, no cache write: it does less);
  (b) what the unchanged route does for those queries: sdpa against the full L-slot cache under the
      bool mask [1, 1, T, L] (again without the rotary and the cache update the route also runs).

Sessions: bench.py's Llama-3-8B (random init, NF4 + double quant, fp16), B = 1, max_len 8192, prompts of
512 / 2048 / 7680 tokens: time from prefill() to the first token (host clock around a synchronised
call) and torch.cuda.max_memory_allocated above the session's own buffers, for the default route,
prefill_chunk = S and prefill_chunk = 512; and admit() of a 2048-token prompt into a running batch of 4.
To separate the gains: the lm_head alone on all S rows (the default route) and on one row (ms, peak MiB), and the
size of the scratch StaticCache the default admit() allocates; what is left is the attention and its glue.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from sample_times import graph_time_us  # noqa: E402  (scripts/ is sys.path[0])
from streams_times import bench_cases  # noqa: E402

HQ, HKV, D, L = 32, 8, 128, 8192
COPIES = 4


def _stats(xs):
    s = sorted(xs)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


@torch.inference_mode()
def kernel_cases(emit, repeat):
    from quantizations_amd.layer_ops import prefill_attention

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    scale = D ** -0.5
    kc = torch.randn(1, HKV, L, D, device=dev, generator=g).half()
    vc = torch.randn(1, HKV, L, D, device=dev, generator=g).half()
    for T, start in ((512, 0), (2048, 0), (8192, 0), (512, 7680)):
        qs = [torch.randn(1, T, HQ * D, device=dev, generator=g).half() for _ in range(COPIES)]
        ks = [torch.randn(1, T, HKV * D, device=dev, generator=g).half() for _ in range(COPIES)]
        vs = [torch.randn(1, T, HKV * D, device=dev, generator=g).half() for _ in range(COPIES)]
        ang = torch.rand(1, T, D // 2, device=dev, generator=g) * 6.0
        cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
        pos = torch.tensor([start], dtype=torch.int64, device=dev)
        ln = torch.tensor([T], dtype=torch.int64, device=dev)
        mask = (torch.arange(L, device=dev)[None, :] <= (start + torch.arange(T, device=dev))[:, None]).view(1, 1, T, L)
        q4 = [q.view(1, T, HQ, D).transpose(1, 2).contiguous() for q in qs]
        k4 = [k.view(1, T, HKV, D).transpose(1, 2).contiguous() for k in ks]
        v4 = [v.view(1, T, HKV, D).transpose(1, 2).contiguous() for v in vs]
        ours = [lambda i=i: prefill_attention(qs[i], ks[i], vs[i], cos, sin, kc, vc, pos, ln, HQ, scale) for i in range(COPIES)]
        flash = [lambda i=i: F.scaled_dot_product_attention(q4[i], k4[i], v4[i], is_causal=True, enable_gqa=True)
                 for i in range(COPIES)]
        masked = [lambda i=i: F.scaled_dot_product_attention(q4[i], kc, vc, attn_mask=mask, enable_gqa=True)
                  for i in range(COPIES)]
        visible = sum(start + i + 1 for i in range(T))
        flops = 4.0 * HQ * D * visible
        us = {"prefill_attention": [], "sdpa_causal_flash": [], "sdpa_masked_full_cache": []}
        for _ in range(repeat):
            us["prefill_attention"].append(graph_time_us(ours, reps=5))
            if start == 0:
                us["sdpa_causal_flash"].append(graph_time_us(flash, reps=5))
            us["sdpa_masked_full_cache"].append(graph_time_us(masked, reps=5))
        # the same bits from the graph as from an eager call, and the library's routes agree with ours
        ref = F.scaled_dot_product_attention(q4[0], kc, vc, attn_mask=mask, enable_gqa=True)
        row = {"case": "kernel", "Hq": HQ, "Hkv": HKV, "D": D, "L": L, "T": T, "start": start, "dtype": "fp16",
               "copies": COPIES, "causal_gflop": round(flops / 1e9, 2), "masked_sdpa_finite": bool(torch.isfinite(ref).all())}
        for name, xs in us.items():
            if xs:
                st = _stats(xs)
                row[name + "_us"] = st
                row[name + "_tflops"] = round(flops / st["median"] / 1e6, 1)
        ours_med = row["prefill_attention_us"]["median"]
        row["masked_over_ours"] = round(row["sdpa_masked_full_cache_us"]["median"] / ours_med, 2)
        if start == 0:
            row["ours_over_flash"] = round(ours_med / row["sdpa_causal_flash_us"]["median"], 2)
        emit(row)
        del qs, ks, vs, q4, k4, v4, mask
        torch.cuda.empty_cache()


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
    counts = prepare_for_decode(model)
    gen = torch.Generator().manual_seed(1234)
    for S in (512, 2048, 7680):
        ids = torch.randint(0, cfg.vocab_size, (1, S), generator=gen).cuda()
        routes = [("default", None), ("chunk_S", S), ("chunk_512", 512)]
        ms = {n: [] for n, _ in routes}
        mib = {n: [] for n, _ in routes}
        first = {}
        for rep in range(args.repeat + 1):             # the first round warms every route up and is dropped
            for name, chunk in routes:
                sess = StreamSession(model, 1, L, prefill_chunk=chunk)
                t, m = _timed(lambda: sess.prefill(ids, [S], max_new_tokens=4))
                first[name] = int(sess.tok[0, 0])
                if rep:
                    ms[name].append(t)
                    mib[name].append(m)
                del sess
                torch.cuda.empty_cache()
        emit({"case": "prefill", "model": "llama3-8b", "layers": cfg.num_hidden_layers, "batch": 1, "prompt": S,
              "max_len": L, "ms_to_first_token": {n: _stats(v) for n, v in ms.items()},
              "peak_MiB_above_session": {n: _stats(v) for n, v in mib.items()}, "first_token": first,
              "prepare_for_decode": counts})
    # what the B-row lm_head saves: the head on S rows (the default route) and on one row, alone
    head = model.get_output_embeddings()
    for S in (512, 2048, 7680):
        hid = torch.randn(1, S, cfg.hidden_size, device="cuda", dtype=torch.float16)
        ms = {"all_rows": [], "one_row": []}
        mib = {"all_rows": [], "one_row": []}
        for rep in range(args.repeat + 1):
            for name, x in (("all_rows", hid), ("one_row", hid[:, -1:])):
                t, m = _timed(lambda: head(x))
                if rep:
                    ms[name].append(t)
                    mib[name].append(m)
        emit({"case": "lm_head", "rows": S, "vocab": cfg.vocab_size, "ms": {n: _stats(v) for n, v in ms.items()},
              "peak_MiB": {n: _stats(v) for n, v in mib.items()}})
        del hid
        torch.cuda.empty_cache()
    kv = cfg.num_key_value_heads * (cfg.hidden_size // cfg.num_attention_heads)
    emit({"case": "scratch_cache", "what": "the second StaticCache of the default admit(): 2 * layers * Hkv * D * max_len * 2 B",
          "MiB": round(2 * cfg.num_hidden_layers * kv * L * 2 / 2 ** 20, 1)})
    B, S = 4, 2048
    ids = torch.randint(0, cfg.vocab_size, (B, 64), generator=gen).cuda()
    newcomer = torch.randint(0, cfg.vocab_size, (S,), generator=gen)
    routes = [("default", None), ("chunk_S", S), ("chunk_512", 512)]
    ms = {n: [] for n, _ in routes}
    mib = {n: [] for n, _ in routes}
    for rep in range(args.repeat + 1):
        for name, chunk in routes:
            sess = StreamSession(model, B, L, prefill_chunk=chunk)
            sess.prefill(ids, [64] * B, max_new_tokens=[64, 2, 64, 64])
            for _ in range(4):
                sess.step()
            t, m = _timed(lambda: sess.admit(1, newcomer, max_new_tokens=8))
            if rep:
                ms[name].append(t)
                mib[name].append(m)
            del sess
            torch.cuda.empty_cache()
    emit({"case": "admit", "model": "llama3-8b", "layers": cfg.num_hidden_layers, "batch": B, "prompt": S, "max_len": L,
          "ms": {n: _stats(v) for n, v in ms.items()}, "peak_MiB_above_session": {n: _stats(v) for n, v in mib.items()},
          "note": "the default route's peak includes its scratch StaticCache on the first admit of a session"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true", help="only the per-call times")
    ap.add_argument("--sessions", action="store_true", help="only the Llama-3-8B sessions")
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "prefill_attention_times.txt"))
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
