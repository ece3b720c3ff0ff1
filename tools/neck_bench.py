"""The fused FPN level (neck_stream.hip: out = W2 . bf16(W1 . bf16(x) + b1) + b2) against the two launches it replaces, at the level-0 / level-1 shapes of
a 12-frame group of hiera_b+.  python tools/neck_bench.py [frames]"""
import ctypes as C
import os
import sys

os.environ.setdefault("OVO_KNOBS_DYNAMIC", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ovo_amd import _lib as L

dev = torch.device("cuda", 0)
lib = L.load()
FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 12


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def run(rows, d, k1, n_out, iters=20, hid=256):
    x = torch.randn(rows, d, device=dev)
    w1 = torch.zeros(hid, k1, dtype=torch.bfloat16, device=dev)
    w1[:, :d] = (torch.randn(hid, d, device=dev) * d ** -0.5).to(torch.bfloat16)
    w2 = (torch.randn(n_out, hid, device=dev) * hid ** -0.5).to(torch.bfloat16)
    b1, b2 = torch.randn(hid, device=dev), torch.randn(n_out, device=dev)
    lat, out, ref = torch.empty(rows, hid, device=dev), torch.empty(rows, n_out, device=dev), torch.empty(rows, n_out, device=dev)
    q1, q2 = L.gemm_desc(None, w1, lat, bias=b1, rows=rows), L.gemm_desc(None, w2, ref, bias=b2, rows=rows)

    def two():
        L.check(lib.ovo_gemm_f32a(C.byref(q1), None, x.data_ptr(), d, None, None, 0.0, 2, 0, L.stream()))
        L.check(lib.ovo_gemm_f32a(C.byref(q2), None, lat.data_ptr(), hid, None, None, 0.0, 2, 0, L.stream()))

    def fused():
        L.check(lib.ovo_neck_f32(x.data_ptr(), rows, d, w1.data_ptr(), k1, b1.data_ptr(), hid, w2.data_ptr(), hid, b2.data_ptr(), out.data_ptr(), n_out, L.stream()))
    t2 = timed(two, iters)
    by = 4.0 * rows * (d + n_out)
    print(f"({rows}, {d} -> {hid} -> {n_out}): two launches {t2:7.1f} us")
    t = timed(fused, iters)
    print(f"    fused: {t:7.1f} us = {by / t / 1e3:6.0f} GB/s of x in + out;  bit-identical to the two launches: {torch.equal(out, ref)}")


run(FRAMES * 65536, 112, 128, 32)
run(FRAMES * 16384, 224, 256, 64)
