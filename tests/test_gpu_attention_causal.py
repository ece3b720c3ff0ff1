"""-m gpu: `ovo_attention_t.causal` in every kernel form (k_attention_tiny, k_attention32 in each instantiation, k_attention with its trimmed, wide,
2-D-grid and chunked-grid launches) against fp64 softmax on the same bf16 operands.  tests/attention_cases.py has the reference, the inputs and the
table of forms with the dispatcher rule that reaches each; tests/test_attention_cases_host.py proves on the CPU that the probe inputs would show a
mask that is off by one key.  Every comparison prints its figures before it asserts (pytest -s)."""
import pytest
import torch

import attention_cases as AC
from test_gpu_encoder import _attention_call

pytestmark = pytest.mark.gpu

DEV = "cuda"
KNOBS = ("OVO_ATTN32", "OVO_ATTN_NO_TINY", "OVO_ATTN_WIDE", "OVO_ATTN_NARROW", "OVO_ATTN_NO_CHUNK")
FILL = 0x7fc1                               # a bf16 NaN no kernel produces: what the padding of `out` holds before and after

TOL = 2e-2                                  # check 1: atol = rtol = TOL and mean |err| < TOL / 10, the bounds of test_attention_vs_torch for the same roundings


def _knobs(monkeypatch, form):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in form.env.items():
        monkeypatch.setenv(name, value)


def _buffer(shape, lead):
    """bf16 `shape` filled with FILL, `lead` elements into its allocation (lead = 4: 8 bytes, aligned for k_attention's stores but not for
    k_attention32's), and the allocation as int16."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((lead + n,), FILL, dtype=torch.int16, device=DEV)
    assert flat.data_ptr() % 16 == 0
    return flat[lead:].view(torch.bfloat16).view(shape), flat


def _packed_call(form, qkv, Tq, Tk, hd, causal, scale):
    """[b, Tq, h hd] through L.attention_packed; the form's `out` is contiguous and, with offset_out, 8 bytes into its buffer."""
    b, _, _, h, _ = qkv.shape
    out, _ = _buffer((b, Tq, h * hd), 4 if form.offset_out else 0)
    return _attention_call(qkv, b, h, Tq, Tk, hd, causal=causal, scale=scale, out=out)


def _hand_call(q, k, v, o, scale, causal):
    """ovo_attention on a hand-filled descriptor (as tests/test_lib_descriptors.py::_hand_attention): q, k, v, o are [B, H, T, hd] views, any strides."""
    import ctypes as C
    from ovo_amd import _lib as L
    a = L.Attention()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    for name, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        sb, sh, st, sd = t.stride()
        assert sd == 1 and t.dtype == torch.bfloat16
        for field, stride in (("_sb", sb), ("_sh", sh), ("_st", st)):
            setattr(a, name + field, stride)
    a.B, a.H, a.Tq, a.hd = q.shape
    a.Tk, a.scale, a.causal = k.shape[2], scale, causal
    assert o.shape == q.shape and k.shape == v.shape == (a.B, a.H, a.Tk, a.hd)
    L.check(L.load().ovo_attention(C.byref(a), L.stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_ids(AC.CASES))
def test_causal_and_full_attention_vs_fp64(case, monkeypatch):
    """Checks 1-3, on random_case and both probe_cases, causal = 1 and 0, scale = hd ** -0.5 and 0 (prescaled queries):
    1. the whole output against `reference`: atol = rtol = 2e-2 and mean |err| < 2e-3 (P is rounded to bf16 before P V, O is stored in bf16).  The
       probe rows past the first key tile go through the online softmax's rescale branch (their deciding key is ~2^35 above the rest); no case needs
       test_attention_rescale_path's wider 3e-2 / 3e-3 for it: the largest error measured is 0.94 of the bound (230 x 230, hd 56, superdiag, scale in
       the kernel), the largest mean 1.4e-3;
    2. the probe rows alone, max |err| < 0.1, row by row: a lost or leaked key moves such a row by > 0.5 (host test), rounding by ~1e-2, and the
       failing row names the boundary;
    3. causal: out[:, 0] == v[:, 0] bit for bit -- one visible key, P = exp2(0) = 1, row sum 1 (also as the ones column's product), O = v * 1 * (1 / 1):
       nothing rounds, in any form."""
    form, Tq, Tk, hd = case
    b, h = form.bh
    _knobs(monkeypatch, form)
    for prescaled in (False, True):
        _, scale, ref_scale = AC.scales(hd, prescaled)
        for kind in AC.KINDS:
            cpu, rows = AC.case(kind, Tq, Tk, hd, prescaled, b=b, h=h)
            if kind != "random" and not rows:                       # (1 x 1 has no key i + 1)
                continue
            qkv = cpu.to(DEV)
            for causal in (1, 0):
                out = _packed_call(form, qkv, Tq, Tk, hd, causal, scale).cpu()
                ref = AC.packed_reference(cpu, Tq, Tk, ref_scale, causal)
                err = (out.double() - ref).abs()
                probe = err[:, rows].amax((0, 2)) if rows else torch.zeros(0)
                used = float((err / (TOL + TOL * ref.abs())).max())
                what = "%s %dx%d hd %d %s %s causal %d" % (form.name, Tq, Tk, hd, kind, "prescaled" if prescaled else "scaled", causal)
                print("\n[attention causal] %-58s max %.2e (%.2f of the bound) mean %.2e probe rows %.2e" % (what, float(err.max()), used, float(err.mean()), float(probe.max()) if rows else 0.0))
                assert out.isfinite().all(), what
                if causal:
                    assert torch.equal(out[:, 0].view(torch.int16), cpu[:, 0, 2].reshape(b, h * hd).view(torch.int16)), what + ": row 0 is not v[0]"
                for i, e in zip(rows, probe.tolist()):
                    assert e < 0.1, "%s: probe row %d (deciding key %d) off by %.3f" % (what, i, i + AC.KINDS.index(kind) - 1, e)
                torch.testing.assert_close(out.double(), ref, atol=TOL, rtol=TOL, msg=lambda m: what + "\n" + m)
                assert err.mean() < TOL / 10, what


@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_ids(AC.CASES))
def test_nothing_outside_the_problem_is_read_or_written(case, monkeypatch):
    """Check 4.  Two copies of one problem in a buffer of 3 more rows: the q rows >= Tq and the k / v rows >= Tk are NaN in one and 1000 in the other,
    and with causal and Tk > Tq the keys nobody sees differ too.  `out` has 2 more rows per batch and 8 more columns per row than the problem, filled
    with 0x7fc1.  The two outputs are the same bits without a NaN, and the padding comes back untouched."""
    form, Tq, Tk, hd = case
    b, h = form.bh
    D = h * hd
    _knobs(monkeypatch, form)
    for causal in (1, 0):
        outs = []
        for cpu in AC.poison_case(Tq, Tk, hd, causal, b=b, h=h):
            qkv = cpu.to(DEV)
            q, k, v = AC.split(qkv, Tq, Tk)
            padded, flat = _buffer((b, Tq + 2, D + 8), 4 if form.offset_out else 0)
            o = padded[:, :Tq, :D].view(b, Tq, h, hd).permute(0, 2, 1, 3)
            assert o.data_ptr() % 16 == (8 if form.offset_out else 0)
            _hand_call(q, k, v, o, hd ** -0.5, causal)
            got = padded[:, :Tq, :D].clone()
            assert got.isfinite().all(), "a NaN row was read"
            padded.view(torch.int16)[:, :Tq, :D] = FILL
            assert bool((flat == FILL).all()), "the padding of out was written"
            outs.append(got.view(torch.int16))
        assert torch.equal(outs[0], outs[1]), "the output depends on rows outside the problem (causal %d)" % causal
        ref = AC.packed_reference(cpu[:, :max(Tq, Tk)], Tq, Tk, hd ** -0.5, causal)        # (and it is the problem's answer)
        torch.testing.assert_close(got.double().cpu(), ref, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("name,Tq,Tk,hd", AC.FREE_STRIDES, ids=["%s-%dx%d-hd%d" % c for c in AC.FREE_STRIDES])
def test_free_strides_equal_the_packed_run(name, Tq, Tk, hd, monkeypatch):
    """Check 5.  q, k, v separately allocated in head-major [B, H, T, hd], out token-major [B, Tq, H, hd], causal = 1: the same fragments enter the
    same instructions as in the packed run of the same values, so the outputs are the same bits."""
    form = AC.form(name)
    b, h = form.bh
    _knobs(monkeypatch, form)
    for kind in ("random", "diag"):
        qkv = AC.case(kind, Tq, Tk, hd)[0].to(DEV)
        packed = _packed_call(form, qkv, Tq, Tk, hd, 1, hd ** -0.5)
        q, k, v = (t.contiguous() for t in AC.split(qkv, Tq, Tk))
        assert q.stride() == (h * Tq * hd, Tq * hd, hd, 1) and len({q.data_ptr(), k.data_ptr(), v.data_ptr(), qkv.data_ptr()}) == 4
        out, _ = _buffer((b, Tq, h, hd), 0)
        _hand_call(q, k, v, out.permute(0, 2, 1, 3), hd ** -0.5, 1)
        assert torch.equal(out.view(b, Tq, h * hd).view(torch.int16), packed.view(torch.int16)), kind
