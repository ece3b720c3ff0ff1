"""The descriptor builders of ovo_amd/_lib.py (gemm_desc, attention_packed) against descriptors filled in by hand, field by field, and the
mistakes gemm_desc refuses.  CPU tensors: the builders read data_ptr / stride / shape / dtype only and never load the library."""
import pytest
import torch

from ovo_amd import _lib as L

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _same(built, hand):
    assert type(built) is type(hand)
    for name, _ in hand._fields_:
        assert getattr(built, name) == getattr(hand, name), name


def _hand_gemm(A, lda, W, ldw, bias, Cp, ldc, add, ld_add, M, N, K, in_dtype, out_dtype, act, alpha):
    g = L.Gemm()
    g.A, g.lda, g.W, g.ldw, g.bias, g.C, g.ldc, g.add, g.ld_add = A, lda, W, ldw, bias, Cp, ldc, add, ld_add
    g.M, g.N, g.K, g.in_dtype, g.out_dtype, g.act, g.alpha = M, N, K, in_dtype, out_dtype, act, alpha
    return g


def test_gemm_desc_plain_bf16_to_f32():
    m, n, k = 5, 12, 32
    a, w, bias, add, out = torch.zeros(m, k, dtype=BF), torch.zeros(n, k, dtype=BF), torch.zeros(n), torch.zeros(m, n), torch.zeros(m, n)
    _same(L.gemm_desc(a, w, out, bias=bias, add=add, act=1, alpha=0.5),
          _hand_gemm(a.data_ptr(), k, w.data_ptr(), k, bias.data_ptr(), out.data_ptr(), n, add.data_ptr(), n, m, n, k, 2, 0, 1, 0.5))


def test_gemm_desc_f16_in_bf16_out_no_bias():
    m, n, k = 3, 8, 64
    a, w, out = torch.zeros(m, k, dtype=F16), torch.zeros(n, k, dtype=F16), torch.zeros(m, n, dtype=BF)
    _same(L.gemm_desc(a, w, out), _hand_gemm(a.data_ptr(), k, w.data_ptr(), k, None, out.data_ptr(), n, None, 0, m, n, k, 1, 2, 0, 1.0))


def test_gemm_desc_column_slice_and_inplace_residual():
    m, n, k = 7, 16, 32
    a = torch.zeros(m, k + 32, dtype=BF)[:, :k]                       # lda > K
    w = torch.zeros(n, k + 8, dtype=BF)[:, :k]                        # ldw > K
    x, bias = torch.zeros(m, n), torch.zeros(n)
    _same(L.gemm_desc(a, w, x, bias=bias, add=x),                     # add aliases out
          _hand_gemm(a.data_ptr(), k + 32, w.data_ptr(), k + 8, bias.data_ptr(), x.data_ptr(), n, x.data_ptr(), n, m, n, k, 2, 0, 0, 1.0))


def test_gemm_desc_strided_rows_and_column_block():
    """The SAM decoder's forms: every T-th row of a [P T, c] matrix from row 2 on, and a column block of a wider result."""
    P, T, c, n, nm = 4, 6, 32, 8, 3
    q16, w = torch.zeros(P * T, c, dtype=BF), torch.zeros(n, c, dtype=BF)
    out = torch.zeros(P, n, dtype=BF)
    _same(L.gemm_desc(q16, w, out, act=3, rows=P, lda=T * c, a_off=2 * c),
          _hand_gemm(q16.data_ptr() + 2 * c * 2, T * c, w.data_ptr(), c, None, out.data_ptr(), n, None, 0, P, n, c, 2, 2, 3, 1.0))
    x, hyper = torch.zeros(P, c, dtype=BF), torch.zeros(P, nm * n)
    _same(L.gemm_desc(x, w, hyper, ldc=nm * n, c_off=2 * n),
          _hand_gemm(x.data_ptr(), c, w.data_ptr(), c, None, hyper.data_ptr() + 2 * n * 4, nm * n, None, 0, P, n, c, 2, 0, 0, 1.0))


def test_gemm_desc_without_output_or_operand():
    m, n, k = 9, 4, 32
    a, w, bias = torch.zeros(m, k, dtype=F16), torch.zeros(n, k, dtype=F16), torch.zeros(n)
    _same(L.gemm_desc(a, w, None, bias=bias, out_dtype=F16, act=4, alpha=2.0),          # ovo_gemm_argmax, store_scores = 0
          _hand_gemm(a.data_ptr(), k, w.data_ptr(), k, bias.data_ptr(), None, n, None, 0, m, n, k, 1, 1, 4, 2.0))
    out = torch.zeros(m, n)
    _same(L.gemm_desc(None, w, out, rows=m),                                            # ovo_gemm_f32a: A travels beside the descriptor
          _hand_gemm(None, k, w.data_ptr(), k, None, out.data_ptr(), n, None, 0, m, n, k, 1, 0, 0, 1.0))
    for a_, out_ in ((a, None), (None, out)):                                             # ... and each has to say what replaces the tensor
        with pytest.raises(L.OvoHipError):
            L.gemm_desc(a_, w, out_)


def test_gemm_desc_refuses_mismatches():
    a, w, out = torch.zeros(5, 32, dtype=BF), torch.zeros(12, 32, dtype=BF), torch.zeros(5, 12)
    L.gemm_desc(a, w, out)
    i32, meta = torch.int32, "meta"
    for a_, w_, out_, kw in ((torch.zeros(5, 64, dtype=BF), w, out, {}),                                   # K
                             (a.to(F16), w, out, {}), (a, w.to(F16), out, {}),                             # operand dtypes
                             (a, w, torch.zeros(5, 16), {}), (a, w, torch.zeros(4, 12), {}), (a, w, torch.zeros(60), {}),      # out shape
                             (a.to(i32), w.to(i32), out, {}), (a, w, out.to(torch.int64), {}),             # dtypes without a code
                             (a, w, out, dict(bias=torch.zeros(12, device=meta))), (a, w, out, dict(add=torch.zeros(5, 12, device=meta)))):   # another device
        with pytest.raises(L.OvoHipError):
            L.gemm_desc(a_, w_, out_, **kw)


def _hand_attention(qkv, out, B, H, Tq, Tk, hd, T, scale, causal):
    a, D, base = L.Attention(), H * hd, qkv.data_ptr()
    a.q, a.k, a.v, a.o = base, base + D * 2, base + 2 * D * 2, out.data_ptr()
    a.q_sb = a.k_sb = a.v_sb = T * 3 * D
    a.q_sh = a.k_sh = a.v_sh = hd
    a.q_st = a.k_st = a.v_st = 3 * D
    a.o_sb, a.o_sh, a.o_st = Tq * D, hd, D
    a.B, a.H, a.Tq, a.Tk, a.hd, a.scale, a.causal = B, H, Tq, Tk, hd, scale, causal
    return a


def test_attention_packed_vs_hand_filled():
    B, H, Tq, Tk, hd = 2, 3, 5, 9, 8
    qkv = torch.zeros(B, Tk, 3, H, hd, dtype=BF)                      # Tq != Tk: T = the longer
    out = torch.zeros(B, Tq, H * hd, dtype=BF)
    _same(L.attention_packed(qkv, out, B, H, Tq, Tk, hd, scale=hd ** -0.5), _hand_attention(qkv, out, B, H, Tq, Tk, hd, Tk, hd ** -0.5, 0))
    t = 7
    flat, att = torch.zeros(B * t, 3 * H * hd, dtype=BF), torch.zeros(B * t, H * hd, dtype=BF)          # the text encoder's [R, 3 w]
    _same(L.attention_packed(flat, att, B, H, t, t, hd, T=t, scale=0.0, causal=1), _hand_attention(flat, att, B, H, t, t, hd, t, 0.0, 1))
    with pytest.raises(L.OvoHipError):
        L.attention_packed(flat, att, B, H, t, t, hd, scale=0.0)     # a flat tensor does not say T
    with pytest.raises(L.OvoHipError):
        L.attention_packed(qkv, out, B, H, Tq, Tk + 1, hd, scale=1.0)                                  # more keys than rows
