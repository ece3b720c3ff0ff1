"""Inputs, fp64 reference and case table for the tests of `ovo_window_attention_f32` (tests/test_winattn_cases_host.py,
tests/test_gpu_window_attention.py): a plain helper module, torch on the CPU only; nothing of `ovo_amd` is used.

`reference(case, rounded, mistake=None)` restates the formula of include/ovo_hip.h in fp64, one window at a time:
    att[window-major row, head * 56 + :] = softmax(q k^T) v,    q | k | v = LayerNorm(x; g, b, 1e-6) . Wqkv^T + bias
on the operands as stored (x in f32, the weights in bf16, the q rows carrying log2(e) / sqrt(56): the softmax is exp2 of the scores as they are),
windows in the order (b, wy, wx), rows inside a window in the order of its tokens (ty, tx) or, with pool, of its 2 x 2 max-pooled positions (py, px).
rounded=True rounds to bf16 at the kernel's four documented points -- the LayerNorm output, q | k | v, the softmax numerators inside the P . V product
(the divisor is the unrounded sum) and the output -- and keeps every sum in fp64; rounded=False rounds nowhere.  The distance between the two is the
noise a case carries from the rounding points alone: `noise(case)` gives it per window, E_w(case) is its maximum, and the GPU test holds every
window of the kernel's output to E_w from the rounded reference.

`mistake` makes exactly ONE wrong choice (MISTAKES); the host test proves that each of them moves every window it touches by more than 10 E_w.

Inputs are of two kinds.  `flat` has the scaling of test_window_attention_fused_vs_torch (largest probability ~0.1).  `peaked` multiplies the q and
k rows of W by 3 (one key holds most of a row) and makes column 0 of the q rows a common negative number, which changes little for ordinary tokens
and lets ONE channel decide the sign of q; on top of that two windows of the case hold
  * SPECIAL_ROWS: a constant row (zero variance: LayerNorm gives beta, and only because of eps) and a row with every channel at +3e4 (the same, but
    a mean that is off by one f32 step, 2e-3, is as large as sqrt(eps));
  * SPECIAL_NEGQ: tokens whose channel 0 is an outlier: every q of the window, all heads, is negative, so a max-pool that starts from 0 shows.

CASES has one row per kernel form and edge of the window walk, each the smallest shape that reaches the edge; FORMS quotes the launcher rule
(ovo_amd/csrc/winattn.hip, `win_attn_launch`) every row rests on, so that a change of the launcher is seen to empty the row."""
import collections
import functools
import math
import types
import zlib

import torch

HD = 56                                     # head_dim of every form
EPS = 1e-6
QSCALE = math.log2(math.e) / math.sqrt(HD)
GRID, WG_WAVES = 256, 8                     # both kernels: <<<256 workgroups, 8 waves>>>, `for (slot = blockIdx.x * 8 + wave; slot < n; slot += gridDim.x * 8)`
SLOTS = GRID * WG_WAVES                     # 2048 slots per trip: a window (k_win_attn112) or a task = pair of windows (k_win_attn224)
MIN_WINDOWS = 512

Form = collections.namedtuple("Form", "name d d_out heads ws pool kmin kpad rule")
FORMS = {f.name: f for f in (
    Form("s1", 112, 112, 2, 8, 0, 128, 128,
         "plain = !pool && d_out == C && heads == NH; d == C && ws == 8 && H % 8 == 0 && W % 8 == 0 && ldw >= KP (128) && n_win >= 512 -> k_win_attn112<false>, one pass"),
    Form("chg", 112, 224, 4, 8, 1, 128, 128,
         "change = pool && d_out == 2 * C && heads == 2 * NH; otherwise as plain -> k_win_attn112<true>, two passes of two heads (head0 = 0, 2)"),
    Form("s2", 224, 224, 4, 4, 0, 224, 256,
         "d == 224 && d_out == d && heads == 4 && !pool && ws == 4 && H % 4 == 0 && W % 4 == 0 && ldw >= 224 && n_win >= 512 && n_win % 2 == 0 "
         "-> k_win_attn224, two passes, a task = windows 2 task, 2 task + 1"))}
# kmin: the weight columns the kernel reads ([0, kmin): the launcher's lower bound on ldw); kpad: the padded width a careless LayerNorm would divide by

# ld_att, ldw: None = the forward's own (256; 128 / 256); bias: qkv_b given; lead: `att` starts this many bf16 elements into its buffer
Case = collections.namedtuple("Case", "name form kind B H W edge bias ld_att ldw lead", defaults=(True, None, None, 0))


def _table():
    rows = []
    for f in ("s1", "chg"):
        rows += [Case(f + "-min-flat", f, "flat", 1, 128, 256, "minimum"), Case(f + "-min-peaked", f, "peaked", 1, 128, 256, "minimum"),
                 Case(f + "-ragged", f, "flat", 3, 88, 136, "ragged"), Case(f + "-ragged-tall", f, "flat", 3, 136, 88, "ragged"),
                 Case(f + "-loop", f, "flat", 3, 200, 232, "loop")]
    rows += [Case("s2-min-flat", "s2", "flat", 1, 64, 128, "minimum"), Case("s2-min-peaked", "s2", "peaked", 1, 64, 128, "minimum"),
             Case("s2-ragged", "s2", "flat", 2, 68, 76, "ragged"), Case("s2-ragged-tall", "s2", "flat", 2, 76, 68, "ragged"),
             Case("s2-loop", "s2", "flat", 2, 180, 188, "loop")]
    # the free parts of the contract, one pair per form: no bias, no padding columns, a wider weight pitch, att 8 bytes into its buffer; then ld_att = d_out + 4
    for f, (h, w), ldw in (("s1", (128, 256), 136), ("chg", (128, 256), 136), ("s2", (64, 128), 232)):
        d_out = FORMS[f].d_out
        rows += [Case(f + "-free-nobias", f, "flat", 1, h, w, "free", False, d_out, ldw, 4), Case(f + "-free-pitch", f, "flat", 1, h, w, "free", True, d_out + 4, ldw, 0)]
    return rows


CASES = _table()
FREE = [c for c in CASES if c.edge == "free"]
MISTAKES = ("swap_hw", "pitch_h", "batch_sq", "v_pair", "heads_pass2", "pool_t", "pool_mean", "pool_row", "ln_128", "no_bias")
WALK = ("swap_hw", "pitch_h", "batch_sq")   # the mistakes of the window walk: they touch the windows whose source block moves
SPECIAL_ROWS, SPECIAL_NEGQ = 77, 300        # the two special windows of a peaked case


def case(name):
    return next(c for c in CASES if c.name == name)


def case_ids(cases):
    return [c.name for c in cases]


def form(c):
    return FORMS[c.form]


def geometry(c):
    """(nwh, nww, windows per image, windows, keys per window, att rows per window)"""
    f = form(c)
    nwh, nww, tk = c.H // f.ws, c.W // f.ws, f.ws * f.ws
    return nwh, nww, nwh * nww, c.B * nwh * nww, tk, tk // 4 if f.pool else tk


def ld_att(c):
    return c.ld_att or 256


def ldw(c):
    return c.ldw or (128 if form(c).d == 112 else 256)


def applies(c, mistake):
    f = form(c)
    if mistake == "heads_pass2":
        return f.heads == 4
    if mistake in ("pool_t", "pool_mean", "pool_row", "pool_zero"):
        return bool(f.pool) and (mistake != "pool_zero" or c.kind == "peaked")
    if mistake == "no_bias":
        return c.bias
    return True


# ------------------------------------------------------------------------------------------------------------------ the window walk
def window_rows(c, mistake=None):
    """int64 [windows, keys]: the row of x viewed as [B H W, d] that holds each token of each window.  The walk mistakes index as the kernel would
    with the one wrong choice; what then falls outside x wraps around (the reference has to read something: any other block will do)."""
    f = form(c)
    nwh, nww, per, n_win, _, _ = geometry(c)
    win = torch.arange(n_win).reshape(-1, 1, 1)
    if mistake == "batch_sq":
        per = nwh * nwh
    b, wr = win // per, win % per
    cols = nwh if mistake == "swap_hw" else nww
    wy, wx = wr // cols, wr % cols
    ty, tx = torch.arange(f.ws).reshape(1, -1, 1), torch.arange(f.ws).reshape(1, 1, -1)
    pitch = c.H if mistake == "pitch_h" else c.W
    rows = ((b * c.H + wy * f.ws + ty) * pitch + wx * f.ws + tx) % (c.B * c.H * c.W)
    return rows.reshape(n_win, f.ws * f.ws)


def touched(c, mistake):
    """bool [windows]: the windows the mistake is judged on: those whose output it changes (pool_zero, a max-pool that starts from 0: the window whose
    q are all negative -- in the others it changes the cells that happen to be negative)."""
    n_win = geometry(c)[3]
    if mistake in WALK:
        return (window_rows(c, mistake) != window_rows(c)).any(1)
    if mistake == "pool_zero":
        return torch.arange(n_win) == SPECIAL_NEGQ
    return torch.ones(n_win, dtype=torch.bool)


def judged_rows(c, mistake):
    """bool [att rows per window]: pool_t leaves the diagonal pooled positions where they are."""
    tq = geometry(c)[5]
    if mistake == "pool_t":
        return torch.tensor([py != px for py in range(4) for px in range(4)])
    return torch.ones(tq, dtype=torch.bool)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _seed(c):
    return zlib.crc32(("%s %s %d %d %d" % (c.form, c.kind, c.B, c.H, c.W)).encode())


@functools.lru_cache(maxsize=3)
def inputs(c):
    """x f32 [B, H, W, d]; ln_g, ln_b f32 [d]; w bf16 [3 d_out, ldw] -- columns [d, kmin) zero, columns >= kmin (never read) NaN; bias f32 [3 d_out] or None.
    Read-only by convention.  Cases of one form, kind and shape share their values (the free cases: without the bias, in another pitch)."""
    f = form(c)
    g = torch.Generator().manual_seed(_seed(c))
    x = torch.randn(c.B, c.H, c.W, f.d, generator=g) * 1.5 + (4.0 if c.kind == "peaked" else 0.3)
    ln_g, ln_b = 1.0 + 0.2 * torch.randn(f.d, generator=g), 0.1 * torch.randn(f.d, generator=g)
    w = torch.randn(3 * f.d_out, f.d, generator=g) * f.d ** -0.5
    bias = 0.2 * torch.randn(3 * f.d_out, generator=g)
    if c.kind == "peaked":
        w[:f.d_out, 0] = -0.55
        w[:2 * f.d_out] *= 3.0
        xw = x.reshape(-1, f.d)
        rows = window_rows(c)
        xw[rows[SPECIAL_ROWS, 1]] = 0.7
        xw[rows[SPECIAL_ROWS, 2]] = 3e4
        xw[rows[SPECIAL_NEGQ], 0] = (16.0 if f.d == 112 else 22.0) + 6.0 * torch.rand(rows.shape[1], generator=g)
    w[:f.d_out] *= QSCALE                                         # the q rows carry log2(e) / sqrt(head_dim)
    bias[:f.d_out] *= QSCALE
    wp = torch.zeros(3 * f.d_out, ldw(c))
    wp[:, :f.d] = w
    wp[:, f.kmin:] = float("nan")
    return types.SimpleNamespace(x=x, ln_g=ln_g, ln_b=ln_b, w=wp.to(torch.bfloat16), bias=bias if c.bias else None)


# ------------------------------------------------------------------------------------------------------------------ reference
def r16(t):
    return t.to(torch.bfloat16).double()


def _identity(t):
    return t


def _layer_norm(x, g, b, divisor):
    mean = x.sum(-1, keepdim=True) / divisor
    var = (x - mean).pow(2).sum(-1, keepdim=True) / divisor
    return (x - mean) / (var + EPS).sqrt() * g + b


def qkv(c, rounded, mistake=None, windows=None):
    """f64 q [n, heads, tq, 56], k and v [n, heads, tk, 56] of the windows `windows` (a slice; default: all), q pooled where the form pools."""
    f, inp = form(c), inputs(c)
    rnd = r16 if rounded else _identity
    rows = window_rows(c, mistake if mistake in WALK else None)[windows if windows is not None else slice(None)]
    n, tk = rows.shape
    x = inp.x.reshape(-1, f.d)[rows.reshape(-1)].double()
    xn = rnd(_layer_norm(x, inp.ln_g.double(), inp.ln_b.double(), f.kpad if mistake == "ln_128" else f.d))
    w = inp.w[:, :f.d].double()
    bias = inp.bias.double() if inp.bias is not None and mistake != "no_bias" else torch.zeros(3 * f.d_out, dtype=torch.float64)
    if mistake == "heads_pass2":                                   # the second pass (heads 2, 3) with the first pass's weights and bias
        src = torch.arange(3 * f.d_out).reshape(3, f.heads, HD)
        src[:, 2:] = src[:, :2].clone()
        w, bias = w[src.reshape(-1)], bias[src.reshape(-1)]
    t = rnd(xn @ w.T + bias).reshape(n, tk, 3, f.heads, HD)
    q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    if f.pool:                                                     # 2 x 2 over the window's 8 x 8 tokens: (py, dy, px, dx)
        q = q.reshape(n, f.heads, 4, 2, 4, 2, HD)
        if mistake == "pool_mean":
            q = q.mean(dim=(3, 5))
        elif mistake == "pool_row":
            q = q[:, :, :, 0].amax(dim=4)
        else:
            q = q.amax(dim=(3, 5))
        if mistake == "pool_t":
            q = q.transpose(2, 3)
        if mistake == "pool_zero":
            q = q.clamp(min=0.0)
        q = q.reshape(n, f.heads, 16, HD)
    if mistake == "v_pair":
        v = v[:, :, torch.arange(tk) ^ 1]
    return q, k, v


def probabilities(q, k):
    """(numerators exp2(s - max), their sums): f64 [n, heads, tq, tk], [n, heads, tq, 1]"""
    s = q @ k.transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return p, p.sum(-1, keepdim=True)


def reference(c, rounded, mistake=None):
    """f64 [windows * att rows per window, d_out]"""
    assert mistake is None or applies(c, mistake), (c.name, mistake)
    f = form(c)
    n_win, tq = geometry(c)[3], geometry(c)[5]
    rnd = r16 if rounded else _identity
    out = torch.empty(n_win, tq, f.d_out, dtype=torch.float64)
    for lo in range(0, n_win, 256):
        q, k, v = qkv(c, rounded, mistake, slice(lo, lo + 256))
        p, total = probabilities(q, k)
        o = rnd((rnd(p) @ v) / total)                              # [n, heads, tq, 56]
        out[lo:lo + 256] = o.permute(0, 2, 1, 3).reshape(-1, tq, f.d_out)
    return out.reshape(n_win * tq, f.d_out)


def window_rms(t, c, rows=None):
    """rms of t [windows * tq, d_out] over each window's block (over its rows `rows`): f64 [windows]"""
    n_win, tq = geometry(c)[3], geometry(c)[5]
    t = t.reshape(n_win, tq, -1)
    if rows is not None:
        t = t[:, rows]
    return t.pow(2).mean(dim=(1, 2)).sqrt()


@functools.lru_cache(maxsize=2)
def references(c):
    """(rounded, unrounded) references of a case; read-only by convention."""
    return reference(c, True), reference(c, False)


def noise(c):
    """(per-window rms of rounded - unrounded over the output's global rms [windows], that global rms).  E_w(case) is the maximum of the first."""
    rounded, plain = references(c)
    rms = plain.pow(2).mean().sqrt().item()
    return window_rms(rounded - plain, c) / rms, rms


def walk_case(c):
    """The walk-independence run of a case with B > 1: its LAST image in front, fresh content behind it up to >= 512 windows (an even number for the
    224 form).  (case of the same form whose inputs() is that batch, first window of the image in `c`)"""
    f = form(c)
    per = geometry(c)[2]
    nb = 1
    while nb * per < MIN_WINDOWS or (f.name == "s2" and nb * per % 2):
        nb += 1
    return c._replace(name=c.name + "-walk", B=nb, kind=c.kind + "-walk"), (c.B - 1) * per


def walk_inputs(c):
    """inputs() of walk_case(c): the same weights, image 0 = the last image of c."""
    wc, _ = walk_case(c)
    inp, fresh = inputs(c), inputs(wc)
    x = fresh.x.clone()
    x[0] = inp.x[-1]
    return types.SimpleNamespace(x=x, ln_g=inp.ln_g, ln_b=inp.ln_b, w=inp.w, bias=inp.bias)
