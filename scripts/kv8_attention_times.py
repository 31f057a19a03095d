#!/usr/bin/env python
"""The FP8 paged KV cache: what each kv8 attention launch costs beside its 16-bit paged twin, what
kv_dtype="fp8" does to a session, and what the format does to the attention output.

  python scripts/kv8_attention_times.py                      # everything -> profiles/kv8_attention_times.txt
  python scripts/kv8_attention_times.py --kernel | --sessions | --accuracy
  python scripts/kv8_attention_times.py --bench --parent DIR # bench.py's line, parent and this tree in turn

Kernel (us per call; scripts/paged_attention_times.py's shapes and manner: COPIES calls over rotating
q / k / v buffers captured back to back into one graph, medians of three interleaved repeats with their
min and max): Llama-3-8B heads (Hq 32, Hkv 8, D 128, fp16), pages scrambled over a pool of twice the
needed size.  The yardstick of every kv8 launch is the 16-bit paged launch in the same run.
"slower_than_spread": the kv8 median exceeds the twin's by more than the twin's own max - min.

Sessions: bench.py's Llama-3-8B (random init, NF4 + double quant, fp16), B = 4, max_len 8192,
prefill_chunk 512: a replayed step with kv_pages, 16-bit against fp8; bytes_per_page of both; and the
number of 2056-token streams (limit: 64 prompt tokens + 1992 new ones, 17 pages) a session of 32 rows (each
holds one page from the start) over a pool of 4096 MiB -- the StaticCache of 4 x 8192 -- admits before
KVPagesExhausted.

Accuracy (a property of the format, not of the kernel): max and rms error of the decode attention output
against fp64 attention over the unquantised cache, on randn operands, beside the 16-bit launch's own.
"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))

import torch  # noqa: E402

from sample_times import graph_time_us  # noqa: E402  (scripts/ is sys.path[0])
from streams_times import bench_cases  # noqa: E402

HQ, HKV, D = 32, 8, 128
COPIES = 4
PAGE = 128


def _stats(xs):
    s = sorted(xs)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


def _pair(row, twin, kv8):
    a, b = _stats(twin), _stats(kv8)
    row["paged_us"], row["kv8_us"] = a, b
    row["kv8_minus_paged_us"] = round(b["median"] - a["median"], 2)
    row["slower_than_spread"] = bool(b["median"] - a["median"] > a["max"] - a["min"])
    row["faster_than_spread"] = bool(a["median"] - b["median"] > a["max"] - a["min"])
    return row


def _pools(B, NP, dev, g):
    """16-bit pools of twice the needed pages, byte pools of the same page count holding plausible rows
    (random finite codes, scale bytes near 120) and a table of scrambled, distinct pages."""
    P = 2 * B * NP
    kp = torch.randn(P, HKV, PAGE, D, device=dev, generator=g).half()
    vp = torch.randn(P, HKV, PAGE, D, device=dev, generator=g).half()
    pools8 = []
    for _ in range(2):
        codes = torch.randint(0, 256, (P, HKV, PAGE * D), device=dev, generator=g, dtype=torch.uint8)
        codes[(codes & 0x7F) == 0x7F] = 0x38
        scales = torch.randint(118, 122, (P, HKV, PAGE), device=dev, generator=g, dtype=torch.uint8)
        pools8.append(torch.cat((codes, scales), -1).contiguous())
    table = torch.randperm(P, device=dev, generator=g)[:B * NP].to(torch.int32).view(B, NP).contiguous()
    return kp, vp, pools8[0], pools8[1], table


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
                kp, vp, kp8, vp8, table = _pools(B, NP, dev, g)
                qs = [torch.randn(B, T, HQ * D, device=dev, generator=g).half() for _ in range(COPIES)]
                ks = [torch.randn(B, T, HKV * D, device=dev, generator=g).half() for _ in range(COPIES)]
                vs = [torch.randn(B, T, HKV * D, device=dev, generator=g).half() for _ in range(COPIES)]
                ang = torch.rand(B, T, D // 2, device=dev, generator=g) * 6.0
                cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
                for mix in ("long", "mixed"):
                    pos = torch.full((B,), 40, dtype=torch.int64, device=dev)
                    pos[0 if mix == "mixed" else slice(None)] = L - 2 - T
                    f16, f8 = ((lo.decode_attention_paged, lo.decode_attention_paged_kv8) if T == 1 else
                               (lo.decode_attention_verify_paged, lo.decode_attention_verify_paged_kv8))
                    twin = [lambda i=i: f16(qs[i], ks[i], vs[i], cos, sin, kp, vp, table, pos, HQ, scale) for i in range(COPIES)]
                    kv8 = [lambda i=i: f8(qs[i], ks[i], vs[i], cos, sin, kp8, vp8, table, pos, HQ, scale) for i in range(COPIES)]
                    a, b = [], []
                    for _ in range(repeat):
                        a.append(graph_time_us(twin, reps=20))
                        b.append(graph_time_us(kv8, reps=20))
                    emit(_pair({"case": "decode" if T == 1 else "verify", "B": B, "T": T, "L": L, "positions": mix,
                                "Hq": HQ, "Hkv": HKV, "D": D, "dtype": "fp16", "pool_pages": kp.shape[0]}, a, b))
                del kp, vp, kp8, vp8
                torch.cuda.empty_cache()
    L = 8192
    NP = L // PAGE
    kp, vp, kp8, vp8, table = _pools(1, NP, dev, g)
    for T, start in ((512, 0), (2048, 0), (512, 7680)):
        qs = [torch.randn(1, T, HQ * D, device=dev, generator=g).half() for _ in range(COPIES)]
        ks = [torch.randn(1, T, HKV * D, device=dev, generator=g).half() for _ in range(COPIES)]
        vs = [torch.randn(1, T, HKV * D, device=dev, generator=g).half() for _ in range(COPIES)]
        ang = torch.rand(1, T, D // 2, device=dev, generator=g) * 6.0
        cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
        pos = torch.tensor([start], dtype=torch.int64, device=dev)
        ln = torch.tensor([T], dtype=torch.int64, device=dev)
        twin = [lambda i=i: lo.prefill_attention_paged(qs[i], ks[i], vs[i], cos, sin, kp, vp, table, pos, ln, HQ, scale)
                for i in range(COPIES)]
        kv8 = [lambda i=i: lo.prefill_attention_paged_kv8(qs[i], ks[i], vs[i], cos, sin, kp8, vp8, table, pos, ln, HQ,
                                                          scale) for i in range(COPIES)]
        a, b = [], []
        for _ in range(repeat):
            a.append(graph_time_us(twin, reps=5))
            b.append(graph_time_us(kv8, reps=5))
        emit(_pair({"case": "prefill", "B": 1, "T": T, "start": start, "L": L, "Hq": HQ, "Hkv": HKV, "D": D,
                    "dtype": "fp16", "pool_pages": kp.shape[0]}, a, b))


def session_cases(emit, args):
    import bench
    from quantizations_amd.generation import StreamSession, prepare_for_decode
    from quantizations_amd.kv_pages import KVPagesExhausted

    model, cfg = bench.build_model(args.layers, seed=0)
    prepare_for_decode(model)
    gen = torch.Generator().manual_seed(1234)
    B, L, chunk = 4, 8192, 512
    NPS = L // PAGE
    ids = torch.randint(0, cfg.vocab_size, (B, 64), generator=gen).cuda()
    kinds = (("paged_16bit", {}), ("paged_fp8", {"kv_dtype": "fp8"}))
    ms, per_page = {n: [] for n, _ in kinds}, {}
    for rep in range(args.repeat + 1):
        for name, kw in kinds:
            sess = StreamSession(model, B, L, prefill_chunk=chunk, kv_pages=2 * B * NPS, **kw)
            sess.prefill(ids, [64] * B, max_new_tokens=[512, 2, 2, 512])
            for _ in range(4):
                sess.step()
            per_page[name] = sess.page_stats()["bytes_per_page"]
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
          "ms_per_step": {n: _stats(v) for n, v in ms.items()}, "bytes_per_page": per_page})
    # streams of 2056 tokens (17 pages each) in a pool of the StaticCache's bytes
    head_dim = cfg.hidden_size // cfg.num_attention_heads
    budget = 2 * cfg.num_hidden_layers * cfg.num_key_value_heads * head_dim * L * 2 * B
    rows, admitted = 32, {}
    prompt = torch.randint(0, cfg.vocab_size, (64,), generator=gen)
    for name, kw in kinds:
        pages = budget // per_page[name]
        sess = StreamSession(model, rows, 2056, graph=False, prefill_chunk=chunk, kv_pages=int(pages), **kw)
        first = torch.randint(0, cfg.vocab_size, (rows, 1), generator=gen).cuda()
        sess.prefill(first, [1] * rows, max_new_tokens=1)      # lays the cache out: every row holds one page
        n = 0
        try:
            for r in range(rows):
                sess.admit(r, prompt, max_new_tokens=2056 - 64)
                n += 1
        except KVPagesExhausted:
            pass
        admitted[name] = {"pool_pages": int(pages), "streams": n, "page_stats": sess.page_stats()}
        del sess
        torch.cuda.empty_cache()
    emit({"case": "capacity", "pool_MiB": round(budget / 2 ** 20, 1), "stream_tokens": 2056, "rows": rows,
          "admitted": admitted})


@torch.inference_mode()
def accuracy_cases(emit):
    """Decode attention at L = 512 / 4096 on randn operands: fp64 attention over the unquantised cache
    (the rotated new row included) against the 16-bit paged launch and the kv8 launch on the quantised cache."""
    import kv8_reference as k8
    from quantizations_amd import layer_ops as lo

    dev = torch.device("cuda")
    hq, hkv = 8, 2
    for dt, name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        for L in (512, 4096):
            g = torch.Generator().manual_seed(L)
            NP, B = L // PAGE, 2
            kp = torch.randn(B * NP, hkv, PAGE, D, generator=g).to(dt)
            vp = torch.randn(B * NP, hkv, PAGE, D, generator=g).to(dt)
            table = torch.arange(B * NP, dtype=torch.int32).view(B, NP).to(dev)
            q = torch.randn(B, 1, hq * D, generator=g).to(dt).to(dev)
            k = torch.randn(B, 1, hkv * D, generator=g).to(dt).to(dev)
            v = torch.randn(B, 1, hkv * D, generator=g).to(dt).to(dev)
            cos, sin = torch.ones(B, 1, D, dtype=dt, device=dev), torch.zeros(B, 1, D, dtype=dt, device=dev)
            pos = torch.full((B,), L - 1, dtype=torch.int64, device=dev)
            scale = 1.0 / math.sqrt(D)
            k16, v16 = kp.to(dev), vp.to(dev)
            out16 = lo.decode_attention_paged(q, k, v, cos, sin, k16, v16, table, pos, hq, scale).double().cpu()
            k8p, v8p = k8.quantize_pool(kp).to(dev), k8.quantize_pool(vp).to(dev)
            out8 = lo.decode_attention_paged_kv8(q, k, v, cos, sin, k8p, v8p, table, pos, hq, scale).double().cpu()
            kc = k16.cpu().double().view(B, NP, hkv, PAGE, D).permute(0, 2, 1, 3, 4).reshape(B, hkv, L, D)
            vc = v16.cpu().double().view(B, NP, hkv, PAGE, D).permute(0, 2, 1, 3, 4).reshape(B, hkv, L, D)
            kc[:, :, L - 1] = k.cpu().double().view(B, hkv, D)       # the new token's row (identity rotary)
            vc[:, :, L - 1] = v.cpu().double().view(B, hkv, D)
            qh = q.cpu().double().view(B, hq, D)
            kh = kc.repeat_interleave(hq // hkv, 1)
            vh = vc.repeat_interleave(hq // hkv, 1)
            w = torch.softmax(torch.einsum("bhd,bhld->bhl", qh, kh) * scale, -1)
            ref = torch.einsum("bhl,bhld->bhd", w, vh).reshape(B, 1, hq * D)
            row = {"case": "accuracy", "dtype": name, "L": L, "Hq": hq, "Hkv": hkv, "D": D,
                   "ref_rms": float(ref.pow(2).mean().sqrt())}
            for tag, o in (("paged_16bit", out16), ("kv8", out8)):
                row[tag] = {"max_abs_err": float((o - ref).abs().max()), "rms_err": float((o - ref).pow(2).mean().sqrt())}
            emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true", help="only the per-call times")
    ap.add_argument("--sessions", action="store_true", help="only the Llama-3-8B sessions")
    ap.add_argument("--accuracy", action="store_true", help="only the format's accuracy")
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kv8_attention_times.txt"))
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    both = not (args.kernel or args.sessions or args.accuracy or args.bench)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if not both else "w") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if both or args.kernel:
            kernel_cases(emit, args.repeat)
        if both or args.accuracy:
            accuracy_cases(emit)
        if both or args.sessions:
            with torch.inference_mode():
                session_cases(emit, args)
        if args.bench:
            bench_cases(emit, args)


if __name__ == "__main__":
    main()
