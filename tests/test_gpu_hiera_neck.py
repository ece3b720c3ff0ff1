"""-m gpu: the SAM2 neck's levels 0 / 1 in one launch each (neck_stream.hip: lateral 1 x 1 convolution + conv_s0 / conv_s1, the 256-channel lateral never
written) against a float64 reference with the kernel's rounding points, against the two launches it replaces, and inside ovo_hiera_forward."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(112, 128, 256, 32), (224, 256, 256, 64)]            # (d, ldw1, hid, n_out): hiera_b+ level 0 and level 1
ROWS = 16384 + 37                                                # a partial 16-row block and a partly filled last workgroup


def _case(d, k1, hid, n_out, rows=ROWS):
    """x is a view into a buffer whose elements behind rows * d are NaN: a padding lane (columns d .. k1) or a block past the last row that read them
    would poison the output.  Non-zero mean, a few large channels."""
    g = torch.Generator().manual_seed(1000 + d)
    x0 = torch.randn(rows, d, generator=g) * 1.5 + 0.7
    x0[:, [3, d // 2, d - 1]] *= 40.0
    buf = torch.full((rows * d + 8192,), float("nan"))
    buf[:rows * d] = x0.reshape(-1)
    buf = buf.to(DEV)
    x = buf[:rows * d].view(rows, d)
    w1 = torch.zeros(hid, k1, dtype=torch.bfloat16)
    w1[:, :d] = (torch.randn(hid, d, generator=g) * d ** -0.5).to(torch.bfloat16)
    w2 = (torch.randn(n_out, hid, generator=g) * hid ** -0.5).to(torch.bfloat16)
    b1, b2 = torch.randn(hid, generator=g), torch.randn(n_out, generator=g)
    return x, w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV)


def _fused(lib, L, x, w1, b1, w2, b2, out, rows=None):
    return lib.ovo_neck_f32(x.data_ptr(), x.shape[0] if rows is None else rows, x.shape[1], w1.data_ptr(), w1.stride(0), b1.data_ptr(), w1.shape[0],
                            w2.data_ptr(), w2.stride(0), b2.data_ptr(), out.data_ptr(), w2.shape[0], L.stream())


@pytest.mark.parametrize("d,k1,hid,n_out", SHAPES)
def test_neck_kernel_vs_float64_and_two_launches(d, k1, hid, n_out):
    """out = W2 . bf16(W1 . bf16(x) + b1) + b2 against (a) float64 with the same two roundings (x and the lateral to bf16, nothing else) and (b) the two
    ovo_gemm_f32a launches it replaces, which it must equal BIT FOR BIT: the same roundings and the same f32 sums in the same order.
    Bound of (a): what separates an f32-accumulating kernel from the float64 reference is a lateral value whose f32 sum lands on the other side of a bf16
    rounding boundary -- one bf16 step, <= 2^-8 |lateral|, times its |w2| -- and the f32 rounding of the sums (2^-24 relative per term, far below).  A flip
    needs the f32 error (~1e-6 relative) to straddle a boundary 2^-8 apart: ~1e-4 per value, 0.03 per output (256 values), so among 5e5 outputs a few
    carry three.  max |err| <= 4 steps of the largest lateral through the largest weight; rms err <= ONE typical step in every output (30 times the
    expected rate).  A wrong row, channel order or chunk is ~16 rms(lateral) rms(w2): 4000 times the rms bound."""
    from ovo_amd import _lib as L
    lib = L.load()
    x, w1, b1, w2, b2 = _case(d, k1, hid, n_out)
    rows = x.shape[0]
    GUARD = 7.0
    out = torch.full((rows + 64, n_out), GUARD, device=DEV)
    L.check(_fused(lib, L, x, w1, b1, w2, b2, out, rows))
    # (b) the two launches, through a lateral in memory
    lat, two = torch.empty(rows, hid, device=DEV), torch.empty(rows, n_out, device=DEV)
    q1, q2 = L.gemm_desc(None, w1, lat, bias=b1, rows=rows), L.gemm_desc(None, w2, two, bias=b2, rows=rows)
    L.check(lib.ovo_gemm_f32a(C.byref(q1), None, x.data_ptr(), d, None, None, 0.0, 2, 0, L.stream()))
    L.check(lib.ovo_gemm_f32a(C.byref(q2), None, lat.data_ptr(), hid, None, None, 0.0, 2, 0, L.stream()))
    torch.cuda.synchronize()
    got = out[:rows]
    assert torch.equal(out[rows:], torch.full((64, n_out), GUARD, device=DEV)), "rows behind the end were written"
    assert torch.isfinite(got).all(), "a lane read behind the row data"
    # (a) float64 with the rounding points
    lat64 = x.to(torch.bfloat16).double() @ w1[:, :d].double().T + b1.double()
    ref = lat64.to(torch.bfloat16).double() @ w2.double().T + b2.double()
    step = 2.0 ** -8
    b_max = 4 * step * lat64.abs().max().item() * w2.float().abs().max().item()
    b_rms = step * lat64.pow(2).mean().sqrt().item() * w2.float().pow(2).mean().sqrt().item()
    e_f, e_t = (got.double() - ref).abs(), (two.double() - ref).abs()
    print(f"({rows}, {d} -> {hid} -> {n_out}) vs float64: fused max {e_f.max().item():.3e} rms {e_f.pow(2).mean().sqrt().item():.3e}; "
          f"two launches max {e_t.max().item():.3e} rms {e_t.pow(2).mean().sqrt().item():.3e}; bounds {b_max:.3e} / {b_rms:.3e}; "
          f"output rms {ref.pow(2).mean().sqrt().item():.3e}; elements differing from the two launches: {(got != two).sum().item()}")
    assert e_f.max().item() < b_max and e_f.pow(2).mean().sqrt().item() < b_rms
    assert torch.equal(got, two), "the fused level differs from the two launches"


def test_neck_kernel_declines_what_it_does_not_cover():
    """rows < 16384 and widths without an instantiation: OVO_E_UNSUPPORTED and nothing launched (the output keeps its sentinel)."""
    from ovo_amd import _lib as L
    lib = L.load()
    x, w1, b1, w2, b2 = _case(112, 128, 256, 32)
    out = torch.full((ROWS, 32), 7.0, device=DEV)
    assert _fused(lib, L, x, w1, b1, w2, b2, out, rows=16383) == L.E_UNSUPPORTED
    xs, w1s = torch.randn(ROWS, 96, device=DEV), torch.zeros(256, 128, dtype=torch.bfloat16, device=DEV)
    assert _fused(lib, L, xs, w1s, b1, w2, b2, out) == L.E_UNSUPPORTED                       # hiera_t's width
    w2w = torch.zeros(64, 256, dtype=torch.bfloat16, device=DEV)
    assert _fused(lib, L, x, w1, b1, w2w, torch.zeros(64, device=DEV), out) == L.E_UNSUPPORTED   # level 0's input with level 1's output width
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full((ROWS, 32), 7.0, device=DEV))


def test_neck_fused_equals_two_pass_forward(monkeypatch):
    """The whole hiera_b+ forward (batch 2) with the fused levels against OVO_HIERA_NECK_TWO_PASS=1: every output bit-identical (feat2 never went through
    the new kernel; its top-down sum is now written straight into it).  The workspace is exactly ovo_hiera_workspace_bytes with guard bytes behind it,
    and it is smaller than the two-pass one by the two laterals that are no longer reserved."""
    from ovo_amd import _lib as L
    from ovo_amd.encoders.hiera import SPECS, HipHiera, random_state
    lib = L.load()
    spec = SPECS["hiera_b+"]
    enc = HipHiera(spec, random_state(spec, seed=5), device=DEV)
    B = 2
    x = torch.randn(B, 3, spec.image_size, spec.image_size, generator=torch.Generator().manual_seed(2)).to(DEV)

    def run():
        need = lib.ovo_hiera_workspace_bytes(C.byref(enc._cfg), B)
        enc._ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
        feats = [f.clone() for f in enc.forward(x)]
        torch.cuda.synchronize()
        assert bool((enc._ws[need:] == 0xA5).all()), "the forward wrote behind its workspace"
        return need, feats
    need_f, a = run()
    monkeypatch.setenv("OVO_HIERA_NECK_TWO_PASS", "1")
    need_t, b = run()
    assert need_t - need_f == B * (65536 + 16384) * 256 * 4
    for i, (u, v) in enumerate(zip(a, b)):
        print(f"level {i}: elements differing = {(u != v).sum().item()}, max |difference| = {(u - v).abs().max().item():.3e}")
    for u, v in zip(a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v)


@pytest.mark.parametrize("d,k1,hid,n_out", SHAPES)
def test_neck_kernel_repeats_bit_for_bit(d, k1, hid, n_out):
    """Twenty launches on one input, the same bits every time (the kernel family's two-workgroups-per-CU form once was not: mlp_stream.hip)."""
    from ovo_amd import _lib as L
    lib = L.load()
    x, w1, b1, w2, b2 = _case(d, k1, hid, n_out)
    outs = []
    for _ in range(20):
        out = torch.zeros(ROWS, n_out, device=DEV)
        L.check(_fused(lib, L, x, w1, b1, w2, b2, out))
        outs.append(out)
    torch.cuda.synchronize()
    bad = sum(int(not torch.equal(outs[0], o)) for o in outs[1:])
    assert bad == 0, f"{bad} of 19 repeats differ"
