"""Profiler target: the two launches of a Llama-3-8B decode layer that carry a fused RMSNorm, as the
decode runs them -- q/k/v grouped with the input norm (4096 + 1024 + 1024 rows, K = 4096) and the
gate/up pair with the post-attention norm (2 x 14336 rows, persistent workgroups) -- NF4 + double
quant, exact codes, over rotating weight sets, `iters` of each (eager, so rocprofv3 sees every
dispatch).  QZ_ROOT: the tree whose package is measured (default: this one)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.abspath(os.environ.get("QZ_ROOT", HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_prenorm import _items, DEV  # noqa: E402
from quantizations_amd.core import LAST_FORM, gemv_4bit_grouped, gemv_4bit_pair_silu  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
H, KV, FF, NC = 4096, 1024, 14336, 4
qkv = [_items((H, KV, KV), H, torch.float16, seed=1 + c) for c in range(NC)]
mlp = [_items((FF, FF), H, torch.float16, seed=50 + c) for c in range(NC)]
g = torch.Generator(device="cuda").manual_seed(3)
x = torch.randn(1, 1, H, device=DEV, generator=g).half()
w = (1 + 0.1 * torch.randn(H, device=DEV, generator=g)).half()
outs = [torch.empty(m, device=DEV, dtype=torch.float16) for m in (H, KV, KV)]
for i in range(iters):
    c = i % NC
    gemv_4bit_grouped(x, [(*t, 0, y) for t, y in zip(qkv[c], outs)], exact_codes=True, norm=(w, 1e-5))
    gemv_4bit_pair_silu(x, mlp[c], exact_codes=True, norm=(w, 1e-5))
torch.cuda.synchronize()
print("ok", iters, LAST_FORM, "package", os.path.relpath(ROOT, HERE))
