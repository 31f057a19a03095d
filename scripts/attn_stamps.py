"""In-kernel timeline of the decode attention head (k_decode_attn, csrc/attn_core.h).

  python scripts/attn_stamps.py [--lib PATH/libqz_diag.so] [--hq 32] [--hkv 8]

The measurement-only library's qz_diag_decode_attn_stamped runs the fp16, D = 128, one-chunk head with
s_memrealtime stamps (100 MHz) per wave: 0 entry, 1 every load issued, 2 the wave's K half rows in
registers, 3 the first workgroup barrier passed, 4 the V half rows in registers, 5 P V done, 6 the
output store issued.  Printed per cache length L = 32 / 112 / 128: for each point the median over
the workgroups of the workgroup's LAST wave to reach it (the workgroup is done when its slowest wave
is), in us after the workgroup's first wave entered; then the segments between the points.  The
launch is the last of a burst queued behind a parked stream (the kernels run back to back, as in the
decode graph), `samples` times; the figure of a point is the median over the samples.
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

POINTS = ("entry", "loads issued", "K in registers", "first barrier passed", "V in registers", "P V done",
          "output store issued")


@torch.inference_mode()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(REPO, "quantizations_amd", "libqz_diag.so"))
    ap.add_argument("--hq", type=int, default=32)
    ap.add_argument("--hkv", type=int, default=8)
    ap.add_argument("--samples", type=int, default=12)
    ap.add_argument("--burst", type=int, default=30)
    a = ap.parse_args()
    diag = ctypes.CDLL(a.lib)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    diag.qz_diag_decode_attn_stamped.argtypes = [i32, i32, i32] + [vp] * 11 + [ctypes.c_float, vp, vp]
    dev = torch.device("cuda")
    torch.manual_seed(7)
    Hq, Hkv, D, NL = a.hq, a.hkv, 128, 32
    print(f"decode attention head, fp16, Hq {Hq}, Hkv {Hkv}, D {D}, lib {os.path.relpath(a.lib, REPO)}")
    for L in (32, 112, 128):
        kcs = [torch.randn(1, Hkv, L, D, device=dev).half() for _ in range(NL)]
        vcs = [torch.randn(1, Hkv, L, D, device=dev).half() for _ in range(NL)]
        q = torch.randn(1, Hq * D, device=dev).half()
        k = torch.randn(1, Hkv * D, device=dev).half()
        v = torch.randn(1, Hkv * D, device=dev).half()
        cos = torch.rand(1, D, device=dev).half()
        sin = torch.rand(1, D, device=dev).half()
        mask = torch.ones(1, L, dtype=torch.bool, device=dev)
        pos = torch.zeros(max(a.burst, NL), dtype=torch.int64, device=dev)   # a position word per launch of a burst
        arrive = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.empty(1, Hq * D, device=dev, dtype=torch.float16)
        stamps = torch.zeros(Hq * 4 * 8, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def launch(i):
            rc = diag.qz_diag_decode_attn_stamped(Hq, Hkv, L, q.data_ptr(), k.data_ptr(), v.data_ptr(), cos.data_ptr(),
                                                  sin.data_ptr(), kcs[i % NL].data_ptr(), vcs[i % NL].data_ptr(),
                                                  mask.data_ptr(), pos.data_ptr() + 8 * (i % pos.numel()),
                                                  arrive.data_ptr(), out.data_ptr(),
                                                  D ** -0.5, stamps.data_ptr(), stream)
            if rc:
                raise RuntimeError(f"qz_diag_decode_attn_stamped rc={rc}")

        for i in range(NL):
            launch(i)
        torch.cuda.synchronize()
        per_point = [[] for _ in POINTS]
        for smp in range(a.samples):
            pos.fill_(L - 2)                      # every launch writes slot L - 2 and advances its own word
            torch.cuda._sleep(20_000_000)         # park the stream: the burst queues behind it and runs back to back
            for i in range(a.burst):
                launch(i)
            torch.cuda.synchronize()
            st = stamps.view(Hq, 4, 8).cpu()
            t0 = st[:, :, 0].min(dim=1).values     # the workgroup's first wave in
            for kpt in range(len(POINTS)):
                last = st[:, :, kpt].max(dim=1).values
                per_point[kpt].append(float(((last - t0).double() * 0.01).median()))
        med = [statistics.median(x) for x in per_point]
        print(f"L = {L}: us after the workgroup's first wave entered (median over {Hq} workgroups of the slowest wave)")
        for kpt, name in enumerate(POINTS):
            print(f"  {kpt} {name:22s} {med[kpt]:7.3f}")
        print(f"  loads issued -> K {med[2] - med[1]:.3f}   K -> V {med[4] - med[2]:.3f}   "
              f"V in registers -> output store {med[6] - med[4]:.3f}   whole {med[6]:.3f}")


if __name__ == "__main__":
    main()
