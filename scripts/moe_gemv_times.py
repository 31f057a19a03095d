#!/usr/bin/env python
"""The one-token routed expert launches on the byte-table GEMV (csrc/moe_gemv.hip) at Mixtral-8x7B geometry,
beside the launches they stand in for and beside the dense GEMVs they are built from.

  python scripts/moe_gemv_times.py                       # -> profiles/moe_gemv_times.txt
  python scripts/moe_gemv_times.py --bench --parent DIR  # bench.py's line, parent and this tree in turn

H 4096, I 14336, E 8, top-k 2 (two distinct experts), NF4 + double quant, fp16, T = 1.  us per call as in
scripts/moe_times.py: COPIES calls over rotating weight / activation buffers captured back to back into one graph
and replayed between two events; medians of three interleaved repeats with their min and max.
  mma_pair / mma_down    qz_moe_pair_silu_4bit, qz_moe_down_4bit (decode_route "mma")
  gemv_pair / gemv_down  qz_moe_gemv_pair_silu_4bit, qz_moe_gemv_down_4bit (decode_route "gemv")
  dense_pair             qz_gemv_4bit_pair_silu on ONE dense 14336 x 4096 gate/up pair
  dense_down             qz_gemv_4bit on ONE dense 4096 x 14336
  *_frac_hbm             bytes of the codes and scales read over the time, over HBM_PEAK_GBS
The expectation under test: gemv_pair ~ top_k x dense_pair, gemv_down ~ top_k x dense_down.
`session`: a LAYERS-layer Mixtral of that geometry in a StreamSession at B = 1, one captured step per replay, under
each decode_route: us per step between two events over STEPS replays, the routes alternating.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from moe_times import COPIES, HBM_PEAK_GBS, E, H, I, TOPK, _stats  # noqa: E402  (scripts/ is sys.path[0])
from sample_times import graph_time_us  # noqa: E402
from streams_times import bench_cases  # noqa: E402

LAYERS, STEPS = 4, 64


@torch.inference_mode()
def launch_cases(emit, repeat):
    import quantizations_amd as qa
    from quantizations_amd.core import (gemv_4bit, gemv_4bit_pair_silu, moe_down, moe_gemv_down, moe_gemv_pair_silu,
                                        moe_pair_silu)

    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: (torch.randn(*s, device=dev, generator=g) * 0.02).half()
    gu, gu_state = qa.quantize_4bit(rnd(E * 2 * I, H), quant_type="nf4")
    dn, dn_state = qa.quantize_4bit(rnd(E * H, I), quant_type="nf4")
    gus, dns = [gu.clone() for _ in range(COPIES)], [dn.clone() for _ in range(COPIES)]
    dense_gu = [qa.quantize_4bit(rnd(I, H), quant_type="nf4") for _ in range(2 * COPIES)]
    dense_dn = [qa.quantize_4bit(rnd(H, I), quant_type="nf4") for _ in range(COPIES)]
    idx = torch.tensor([[5, 2]], dtype=torch.int32, device=dev)
    w = torch.tensor([[0.6, 0.4]], device=dev)
    xs = [torch.randn(1, H, device=dev, generator=g).half() for _ in range(COPIES)]
    hs = [moe_pair_silu(xs[i], gus[i], gu_state, idx, E) for i in range(COPIES)]
    calls = {
        "mma_pair": [lambda i=i: moe_pair_silu(xs[i], gus[i], gu_state, idx, E) for i in range(COPIES)],
        "mma_down": [lambda i=i: moe_down(hs[i], dns[i], dn_state, idx, w, E) for i in range(COPIES)],
        "gemv_pair": [lambda i=i: moe_gemv_pair_silu(xs[i], gus[i], gu_state, idx, E) for i in range(COPIES)],
        "gemv_down": [lambda i=i: moe_gemv_down(hs[i], dns[i], dn_state, idx, w, E) for i in range(COPIES)],
        "dense_pair": [lambda i=i: gemv_4bit_pair_silu(xs[i], [(dense_gu[2 * i][0], dense_gu[2 * i][1], None),
                                                               (dense_gu[2 * i + 1][0], dense_gu[2 * i + 1][1], None)])
                       for i in range(COPIES)],
        "dense_down": [lambda i=i: gemv_4bit(hs[i][:, 0], dense_dn[i][0].t(), state=dense_dn[i][1]) for i in range(COPIES)],
    }
    assert all(f() is not None for fs in calls.values() for f in fs)
    us = {k: [] for k in calls}
    for _ in range(repeat):
        for k, fs in calls.items():
            us[k].append(graph_time_us(fs, reps=10))
    row = {"case": "moe_gemv", "H": H, "I": I, "E": E, "top_k": TOPK, "T": 1, "hit": 2, "format": "nf4+dq",
           "dtype": "fp16", "copies": COPIES}
    for k, v in us.items():
        row[k + "_us"] = _stats(v)
    med = {k: row[k + "_us"]["median"] for k in us}
    per_weight = 0.5 + 1.0 / 64 + 4.0 / (64 * 256)   # code nibble, one u8 per 64, one fp32 per 64 * 256
    for k, n in (("mma_pair", 2 * TOPK), ("gemv_pair", 2 * TOPK), ("dense_pair", 2), ("mma_down", TOPK),
                 ("gemv_down", TOPK), ("dense_down", 1)):
        row[k + "_frac_hbm"] = round(n * I * H * per_weight / (med[k] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
    row["gemv_pair_over_topk_dense_pair"] = round(med["gemv_pair"] / (TOPK * med["dense_pair"]), 2)
    row["gemv_down_over_topk_dense_down"] = round(med["gemv_down"] / (TOPK * med["dense_down"]), 2)
    row["mma_over_gemv_pair"] = round(med["mma_pair"] / med["gemv_pair"], 2)
    row["mma_over_gemv_down"] = round(med["mma_down"] / med["gemv_down"], 2)
    h2, y1 = calls["gemv_pair"][0](), calls["mma_down"][0]()
    row["max_abs_pair_gemv_minus_mma"] = round((h2.float() - hs[0].float()).abs().max().item(), 6)
    row["max_abs_down_gemv_minus_mma"] = round((calls["gemv_down"][0]().float() - y1.float()).abs().max().item(), 6)
    emit(row)


@torch.inference_mode()
def session_case(emit, repeat):
    import quantizations_amd as qa
    from quantizations_amd.generation import StreamSession, prepare_for_decode
    from quantizations_amd.integration import replace_with_bnb_linear
    from quantizations_amd.moe import SparseMoe4bit
    from transformers import MixtralConfig, MixtralForCausalLM

    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=TOPK,
                        num_attention_heads=32, num_key_value_heads=8, head_dim=128, num_hidden_layers=LAYERS,
                        vocab_size=32000, max_position_embeddings=2048, sliding_window=None, eos_token_id=None,
                        bos_token_id=None, pad_token_id=None)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = MixtralForCausalLM(cfg)
    model = model.half().eval()
    qa.replace_moe_blocks(replace_with_bnb_linear(model, modules_to_not_convert=["lm_head"]))
    prepare_for_decode(model)
    blocks = [m for m in model.modules() if isinstance(m, SparseMoe4bit)]
    prompt = torch.randint(0, 32000, (1, 32), generator=torch.Generator().manual_seed(3)).cuda()
    sessions = {}
    for route in ("mma", "gemv"):   # each session's graph is captured under its route and keeps it
        for b in blocks:
            b.decode_route = route
        sessions[route] = s = StreamSession(model, 1, 32 + (repeat + 1) * STEPS + 8)
        s.prefill(prompt, [32], max_new_tokens=(repeat + 1) * STEPS + 4)
        for _ in range(8):
            s.step()
    ms = {route: [] for route in sessions}
    for _ in range(repeat):
        for route, s in sessions.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(STEPS):
                s.step()
            e1.record()
            torch.cuda.synchronize()
            ms[route].append(e0.elapsed_time(e1) / STEPS)
    row = {"case": "session", "model": f"Mixtral geometry, {LAYERS} layers, vocab 32000", "B": 1, "steps": STEPS}
    for route, v in ms.items():
        row[f"step_us_{route}"] = _stats([1000 * t for t in v])
    row["mma_over_gemv"] = round(row["step_us_mma"]["median"] / row["step_us_gemv"]["median"], 3)
    emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", action="store_true", help="only bench.py's line (with --parent: against that tree)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "moe_gemv_times.txt"))
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.bench else "w") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if args.bench:
            bench_cases(emit, args)
        else:
            launch_cases(emit, args.repeat)
            session_case(emit, args.repeat)


if __name__ == "__main__":
    main()
