"""In-kernel cost of the fused RMSNorm prologue of the normed grouped decode GEMV.

  python scripts/prenorm_stamps.py [--lib PATH/libqz_diag.so] [--m 6144] [--k 4096]

The measurement-only library's qz_diag_grouped_norm_stamped runs the product instantiation (fp16 x,
exact NF4 codes + double quant) with s_memrealtime stamps (100 MHz): stamp 0 at wave start, 1 after
the prologue (byte table, sum of squares, rs, the normalised LDS image, both barriers), 4 after the
wave's stores.  Printed: the per-wave prologue (1 - 0) and whole-wave (4 - 0) times and the launch's
span (last end - first start), over the last of `burst` back-to-back launches, `samples` times.
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


@torch.inference_mode()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(REPO, "quantizations_amd", "libqz_diag.so"))
    ap.add_argument("--m", type=int, default=6144)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=12)
    ap.add_argument("--burst", type=int, default=30)
    ap.add_argument("--copies", type=int, default=48)
    a = ap.parse_args()
    from quantizations_amd.core import quantize_4bit

    diag = ctypes.CDLL(a.lib)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    diag.qz_diag_set_stamp_buffer.argtypes = [vp]
    diag.qz_diag_grouped_norm_stamped.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, ctypes.c_float, vp,
                                                  ctypes.POINTER(i32), vp]
    dev = torch.device("cuda")
    torch.manual_seed(7)
    M, K = a.m, a.k
    W = (torch.randn(M, K, device=dev) * 0.02).half()
    packed, qs = quantize_4bit(W, blocksize=64, quant_type="nf4", compress_statistics=True)
    sets = [(packed.clone(), qs.absmax.clone(), qs.state2.absmax.clone()) for _ in range(a.copies)]
    x = torch.randn(K, device=dev).half()
    w = (1.0 + 0.1 * torch.randn(K, device=dev)).half()
    y = torch.empty(M, device=dev, dtype=torch.float16)
    stamps = torch.zeros((M + 8) * 8, dtype=torch.int64, device=dev)   # at most M / 2 + 4 waves x 8 u64
    if diag.qz_diag_set_stamp_buffer(stamps.data_ptr()):
        raise RuntimeError("qz_diag_set_stamp_buffer failed")
    stream = torch.cuda.current_stream().cuda_stream
    nw = i32(0)

    def launch(i):
        p, qa, a2 = sets[i % a.copies]
        rc = diag.qz_diag_grouped_norm_stamped(M, K, x.data_ptr(), p.data_ptr(), qa.data_ptr(), a2.data_ptr(),
                                               qs.state2.code.data_ptr(), qs.offset.data_ptr(), w.data_ptr(), 1e-5,
                                               y.data_ptr(), ctypes.byref(nw), stream)
        if rc:
            raise RuntimeError(f"qz_diag_grouped_norm_stamped rc={rc}")

    for i in range(2 * a.copies):
        launch(i)
    torch.cuda.synchronize()
    pro_med, pro_mean, pro_max, wave_med, spans = [], [], [], [], []
    for smp in range(a.samples):
        torch.cuda._sleep(20_000_000)
        for i in range(a.burst):
            launch(smp * a.burst + i)
        torch.cuda.synchronize()
        st = stamps.view(-1, 8)[:nw.value].cpu()
        pro = (st[:, 1] - st[:, 0]).double() * 0.01          # 100 MHz ticks -> us
        wav = (st[:, 4] - st[:, 0]).double() * 0.01
        pro_med.append(float(pro.median()))
        pro_mean.append(float(pro.mean()))
        pro_max.append(float(pro.max()))
        wave_med.append(float(wav.median()))
        spans.append((int(st[:, 4].max()) - int(st[:, 0].min())) * 0.01)
    med = statistics.median
    print(f"normed grouped launch {M} x {K} fp16 exact NF4+DQ, {nw.value} waves, lib {os.path.relpath(a.lib, REPO)}")
    print(f"  prologue per wave (stamps 0->1): median {med(pro_med):.3f} us, mean {med(pro_mean):.3f} us, "
          f"slowest wave {med(pro_max):.3f} us")
    print(f"  whole wave (0->4): median {med(wave_med):.3f} us")
    print(f"  launch span (first start -> last end): median {med(spans):.3f} us, min {min(spans):.3f}, "
          f"max {max(spans):.3f}  ({a.samples} samples, last of {a.burst} back-to-back launches)")


if __name__ == "__main__":
    main()
