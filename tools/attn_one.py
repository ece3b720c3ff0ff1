"""One attention shape, a few launches -- for rocprofv3 --pmc runs: python tools/attn_one.py B H Tq Tk hd [iters]"""
import os; os.environ.setdefault("OVO_KNOBS_DYNAMIC", "1")    # this tool flips OVO_* knobs between launches
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ovo_amd import _lib as L
B, H, Tq, Tk, hd = (int(v) for v in sys.argv[1:6])
iters = int(sys.argv[6]) if len(sys.argv) > 6 else 5
dev = torch.device("cuda", 0); lib = L.load()
D = H * hd; T = max(Tq, Tk)
qkv = torch.randn(B, T, 3, H, hd, device=dev).to(torch.bfloat16)
out = torch.zeros(B, Tq, D, dtype=torch.bfloat16, device=dev)
a = L.attention_packed(qkv, out, B, H, Tq, Tk, hd, scale=hd ** -0.5)
for _ in range(iters): L.check(lib.ovo_attention(C.byref(a), L.stream()))
torch.cuda.synchronize()
