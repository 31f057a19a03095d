"""Low-T backward route crossover (GPU): gemm_4bit_dgrad(route="fused") -- the fused 4-bit dgrad
kernel (+ its split-M reduce) -- against route="dequant" (dequantize_4bit + the library GEMM, the
bitsandbytes MatMul4Bit.backward route), whole-route times including the dequant pass, for the four
Llama-3-8B shapes.  Sets core.dgrad_fused_max_tokens' table.

Both routes run in the same process, interleaved (fused, dequant, fused, ... over ROUNDS rounds; the
median of the rounds is reported with the spread), after one warm-up call per route and shape.  Every
call takes the next of several copies of the packed weight, together larger than the 256 MB
Infinity Cache, so no route finds its weight in a cache.  The timed window is queued behind a
device-side sleep, so it holds kernel time and not the Python launch overhead.
   python scripts/dgrad_lowT_sweep.py [--out FILE]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantizations_amd.core import gemm_4bit_dgrad, quantize_4bit  # noqa: E402

ROUNDS, ITERS = 5, 20
CACHE_BYTES = 256 << 20
HBM_BYTES_PER_US = 8.0e6      # 8 TB/s peak: the read floor of the packed bytes


def timed(fn, iters=ITERS):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(50_000_000)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    dev = torch.device("cuda")
    out = {}
    lines = []
    for (M, K) in [(4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336)]:
        torch.manual_seed(M + K)
        packed, st = quantize_4bit((torch.randn(M, K, device=dev) * 0.02).half(), quant_type="nf4")
        ncopy = max(2, -(-CACHE_BYTES // packed.numel()) + 1)
        copies = [packed.clone() for _ in range(ncopy)]
        floor = packed.numel() / HBM_BYTES_PER_US
        for T in (1, 16, 64, 128, 256, 512, 1024, 2048):
            g = torch.randn(T, M, device=dev, dtype=torch.float16)
            routes = {"fused": lambda i: gemm_4bit_dgrad(g, copies[i % ncopy], st, route="fused"),
                      "dequant": lambda i: gemm_4bit_dgrad(g, copies[i % ncopy], st, route="dequant")}
            for fn in routes.values():   # warm-up: code objects, the library's algorithm choice
                fn(0)
                fn(1)
            times = {k: [] for k in routes}
            for _ in range(ROUNDS):
                for k, fn in routes.items():
                    times[k].append(timed(fn))
            f, d = statistics.median(times["fused"]), statistics.median(times["dequant"])
            r = {"fused_us": round(f, 2), "fused_min_max": [round(min(times["fused"]), 2), round(max(times["fused"]), 2)],
                 "dequant_us": round(d, 2),
                 "dequant_min_max": [round(min(times["dequant"]), 2), round(max(times["dequant"]), 2)],
                 "fused_not_slower": f <= d, "packed_read_floor_us": round(floor, 2),
                 "fused_over_floor": round(f / floor, 2)}
            out[f"{M}x{K} T={T}"] = r
            line = f"{M}x{K} T={T} " + json.dumps(r)
            lines.append(line)
            print(line, flush=True)
        del copies
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
