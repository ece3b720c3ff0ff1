"""-m gpu: `ovo_window_attention_f32` (k_win_attn112<false>, k_win_attn112<true>, k_win_attn224) against the fp64 restatement of the header's formula
at every edge of the window walk: H != W both ways round, window counts that are no multiple of a workgroup's 8, images that change inside a
workgroup and inside a pair of windows, second trips of the grid-stride loop with a ragged last trip, a NULL bias, free pitches, peaked softmax rows
and the refusals.  tests/winattn_cases.py has the reference, the inputs and the case table; tests/test_winattn_cases_host.py proves on the CPU that
each planted mistake (H and W exchanged, the wrong pitch, keys paired wrongly in V, a transposed pool, ...) is more than 10 E_w away in every window it
touches.  Every comparison prints its figures before it asserts (pytest -s).

Measured on MI355X, worst window's rms error / E_w(case) (bound: 1), then the global rms error and largest error over the output rms:
    s1-min-flat      0.297  (E_w 3.584e-03)   1.81e-04  2.38e-02
    s1-min-peaked    0.286  (E_w 1.530e-02)   3.50e-04  1.13e-01
    s1-ragged        0.252  (E_w 4.060e-03)   1.84e-04  2.43e-02
    s1-ragged-tall   0.258  (E_w 3.741e-03)   1.69e-04  2.31e-02
    s1-loop          0.267  (E_w 3.730e-03)   1.85e-04  2.46e-02
    chg-min-flat     0.207  (E_w 4.836e-03)   1.79e-04  1.17e-02
    chg-min-peaked   0.190  (E_w 2.030e-02)   3.14e-04  6.69e-02
    chg-ragged       0.334  (E_w 4.790e-03)   2.16e-04  2.35e-02
    chg-ragged-tall  0.166  (E_w 5.980e-03)   1.99e-04  2.14e-02
    chg-loop         0.448  (E_w 5.166e-03)   2.02e-04  3.17e-02
    s2-min-flat      0.340  (E_w 4.314e-03)   2.16e-04  1.78e-02
    s2-min-peaked    0.152  (E_w 1.473e-02)   3.31e-04  3.33e-02
    s2-ragged        0.320  (E_w 4.388e-03)   2.02e-04  3.57e-02
    s2-ragged-tall   0.297  (E_w 4.287e-03)   2.12e-04  1.72e-02
    s2-loop          0.357  (E_w 4.471e-03)   1.97e-04  1.71e-02
    s1-free-nobias   0.255  (E_w 4.438e-03)   2.11e-04  1.58e-02
    s1-free-pitch    0.297  (E_w 3.584e-03)   1.81e-04  2.38e-02
    chg-free-nobias  0.236  (E_w 5.470e-03)   1.96e-04  1.41e-02
    chg-free-pitch   0.207  (E_w 4.836e-03)   1.79e-04  1.17e-02
    s2-free-nobias   0.379  (E_w 4.586e-03)   2.37e-04  2.00e-02
    s2-free-pitch    0.340  (E_w 4.314e-03)   2.16e-04  1.78e-02
The walk-independence test: 0 windows differ in all nine runs; most windows equal the rounded reference bit for bit (median window error 0.000 E_w).
Before the row mean became a true division in winattn.hip (it was a product with the rounded 1 / d) the three peaked cases failed in the window of the
+3e4 row alone: s1-min-peaked window 77 at 6.557 E_w, chg-min-peaked window 77 at 12.781 E_w, s2-min-peaked window 77 at 21.044 E_w; every other figure was as above.
"""
import pytest
import torch

import winattn_cases as WC

pytestmark = pytest.mark.gpu

DEV = "cuda"
FILL = 0x7fc1                               # a bf16 NaN no kernel produces: what `att` holds wherever nothing may be written
SENTINEL_ROWS = 64                          # rows of FILL behind att
GUARD_ROWS = 16                             # rows of NaN (or 1000) behind x
NAN = float("nan")
WALKS = [c for c in WC.CASES if c.edge in ("ragged", "loop")]


def _library():
    from ovo_amd import _lib as L
    return L, L.load()


def _call(lib, L, f, B, H, W, x, ln_g, ln_b, w, ldw, bias, att, ld_att, **over):
    """The entry point on raw addresses (ints); `over` replaces scalar arguments by name."""
    a = dict(B=B, H=H, W=W, ws=f.ws, d=f.d, d_out=f.d_out, heads=f.heads, pool=f.pool, ldw=ldw, ld_att=ld_att)
    a.update(over)
    rc = lib.ovo_window_attention_f32(x, a["B"], a["H"], a["W"], a["ws"], a["d"], a["d_out"], a["heads"], a["pool"], ln_g, ln_b, WC.EPS, w, a["ldw"], bias, att,
                                      a["ld_att"], L.stream())
    torch.cuda.synchronize()
    return rc


def _run(case, inp=None, guard=NAN):
    """One launch of a case (of `inp`, default its own inputs): x with GUARD_ROWS rows of `guard` behind it, the never-read weight columns holding
    `guard`, att `lead` elements into a buffer of FILL with SENTINEL_ROWS more rows.  Returns (status, the [rows, d_out] block that may be written as
    int16 on the device, whether everything else of the buffer still holds FILL)."""
    L, lib = _library()
    f, inp = WC.form(case), inp or WC.inputs(case)
    B = inp.x.shape[0]
    rows, ld = B * WC.geometry(case)[2] * WC.geometry(case)[5], WC.ld_att(case)
    x = torch.full((B * case.H * case.W + GUARD_ROWS, f.d), guard, dtype=torch.float32, device=DEV)
    x[:B * case.H * case.W] = inp.x.reshape(-1, f.d).to(DEV)
    w = torch.where(inp.w.isnan(), torch.tensor(guard, dtype=torch.bfloat16), inp.w).to(DEV)
    ln_g, ln_b, bias = inp.ln_g.to(DEV), inp.ln_b.to(DEV), None if inp.bias is None else inp.bias.to(DEV)
    flat = torch.full((case.lead + (rows + SENTINEL_ROWS) * ld,), FILL, dtype=torch.int16, device=DEV)
    att = flat[case.lead:]
    assert x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 and att.data_ptr() % 16 == 2 * case.lead
    rc = _call(lib, L, f, B, case.H, case.W, x.data_ptr(), ln_g.data_ptr(), ln_b.data_ptr(), w.data_ptr(), w.shape[1], bias.data_ptr() if bias is not None else None,
               att.data_ptr(), ld)
    block = att[:rows * ld].view(rows, ld)[:, :f.d_out]
    got = block.clone()
    block.fill_(FILL)
    return rc, got, bool((flat == FILL).all())


@pytest.mark.parametrize("case", WC.CASES, ids=WC.case_ids(WC.CASES))
def test_window_attention_vs_fp64_in_every_window(case):
    """Every window of the output within E_w(case) of the rounded reference: E_w is the largest per-window rms of (rounded - unrounded reference) over the
    output's global rms, recomputed here from the two references alone.  The kernel shares the rounded reference's rounding points and differs by f32
    summation order and the few values on a bf16 boundary, which test_window_attention_fused_vs_torch measured at ~6 % of that noise globally (the worst window here: 0.15 - 0.45); every planted
    mistake is > 10 E_w away in every window it touches.  Flat cases also meet that test's global bounds."""
    rc, got, untouched = _run(case)
    assert rc == 0
    e, rms = WC.noise(case)
    e_w = float(e.max())
    ref = WC.references(case)[0]
    out = got.view(torch.bfloat16).double().cpu()
    finite = bool(out.isfinite().all())
    err = torch.nan_to_num(out - ref, nan=float("inf"))
    per_window = WC.window_rms(err, case) / rms
    worst = int(per_window.argmax())
    rms_ref = float(ref.pow(2).mean().sqrt())
    g_rms, g_max = float(err.pow(2).mean().sqrt()) / rms_ref, float(err.abs().max()) / rms_ref
    print("\n[winattn gpu] %-16s worst window %4d: rms err / E_w = %.3f (E_w %.3e, median window %.3f); global rms %.2e max %.2e of the output rms" % (
        case.name, worst, float(per_window[worst]) / e_w, e_w, float(per_window.median()) / e_w, g_rms, g_max))
    assert finite, "%s: NaN in the output (first in window %d)" % (case.name, worst)
    assert untouched, "%s: something outside att[:, :d_out] was written" % case.name
    assert float(per_window[worst]) <= e_w, "%s: window %d is %.2f E_w from the reference" % (case.name, worst, float(per_window[worst]) / e_w)
    if case.kind == "flat":
        assert g_rms < 1e-3 and g_max < 8e-2


@pytest.mark.parametrize("case", WC.FREE, ids=WC.case_ids(WC.FREE))
def test_nothing_outside_the_problem_is_read_or_written(case):
    """The free cases twice: NaN, then 1000, in the rows behind x and in the weight columns the kernels never read (>= 128 / 224 of a pitch of 136 / 232).
    The same bits without a NaN both times; the padding columns of att (ld_att = d_out + 4), its 64 sentinel rows and the 8 bytes in front of it keep
    their fill."""
    outs = []
    for guard in (NAN, 1000.0):
        rc, got, untouched = _run(case, guard=guard)
        assert rc == 0 and untouched
        assert got.view(torch.bfloat16).isfinite().all(), "a NaN guard was read"
        outs.append(got)
    assert torch.equal(outs[0], outs[1]), "the output depends on values outside the problem"


@pytest.mark.parametrize("case", WALKS, ids=WC.case_ids(WALKS))
def test_a_window_gives_the_same_bits_in_any_slot(case):
    """The last image of a ragged / loop case run again as image 0 of another grid, with other content behind it: its windows sit in other slots (other
    wave, other workgroup, other trip of the loop, the other half of a 224-form pair: 323 and 2115 windows per image are odd), and their rows come
    out bit for bit.  With the parity test this makes the tail, the second trip and the straddling pair exact statements."""
    per, tq = WC.geometry(case)[2], WC.geometry(case)[5]
    wc, first = WC.walk_case(case)
    rc_a, whole, _ = _run(case)
    rc_b, alone, untouched = _run(wc, WC.walk_inputs(case))
    assert rc_a == 0 and rc_b == 0 and untouched
    a, b = whole[first * tq:(first + per) * tq], alone[:per * tq]
    differ = (a != b).any(1).reshape(per, tq).any(1)
    print("\n[winattn walk] %-16s windows %d..%d against slots 0..%d of %d: %d differ" % (case.name, first, first + per - 1, per - 1, WC.geometry(wc)[3], int(differ.sum())))
    assert torch.equal(a, b), "windows %s" % (differ.nonzero().flatten()[:8].tolist(),)
    assert not torch.equal(whole[:per * tq], b)                    # (and the comparison is of that image, not of any)


def test_refusals_launch_nothing_and_the_same_calls_without_the_fault_go_through():
    """Every shape outside the three forms, every pitch or address the kernels' vector accesses cannot take: OVO_E_UNSUPPORTED (the caller's cue for the
    three-launch path, not an error: ovo_hip_last_error keeps what it held), a sentinel-filled att unchanged.  A NULL x is a bad argument and names the
    entry point."""
    L, lib = _library()
    x = torch.zeros(48000 * 224 + 4, dtype=torch.float32, device=DEV)
    w = torch.zeros(672 * 264 + 8, dtype=torch.bfloat16, device=DEV)
    ln = torch.ones(224, dtype=torch.float32, device=DEV)
    bias = torch.zeros(672, dtype=torch.float32, device=DEV)
    flat = torch.full((36000 * 264,), FILL, dtype=torch.int16, device=DEV)
    base = {"s1": (1, 128, 256, 128, 256), "chg": (1, 128, 256, 128, 256), "s2": (1, 64, 128, 256, 256)}      # B, H, W, ldw, ld_att

    def call(name, xo=0, wo=0, ao=0, x_null=False, **over):
        B, H, W, ldw, ld = base[name]
        a = dict(B=B, H=H, W=W)
        a.update(over)
        return _call(lib, L, WC.FORMS[name], a.pop("B"), a.pop("H"), a.pop("W"), None if x_null else x.data_ptr() + xo, ln.data_ptr(), ln.data_ptr(), w.data_ptr() + wo,
                     a.pop("ldw", ldw), bias.data_ptr(), flat.data_ptr() + ao, a.pop("ld_att", ld), **a)

    assert call("s1", x_null=True) == -1 and b"ovo_window_attention_f32" in lib.ovo_hip_last_error()
    message = lib.ovo_hip_last_error()
    refused = [
        ("s1", dict(H=56, W=584)), ("chg", dict(H=56, W=584)),                            # 511 windows
        ("s1", dict(H=132)), ("chg", dict(W=260)), ("s2", dict(H=66)), ("s2", dict(W=130)),   # H, W no multiple of the window
        ("s2", dict(ws=8)), ("s1", dict(ws=4)), ("chg", dict(ws=4)),                      # 8 x 8 windows at d = 224, 4 x 4 at d = 112
        ("chg", dict(heads=2)), ("chg", dict(d_out=112)), ("s1", dict(pool=1)), ("s2", dict(pool=1)),   # the pool without the stage change's 4 heads / 224 columns; on the 224 form
        ("s1", dict(heads=4)), ("s1", dict(d_out=224)), ("s2", dict(heads=2)), ("s1", dict(d=96)),
        ("s1", dict(ld_att=108)), ("chg", dict(ld_att=220)), ("s2", dict(ld_att=220)), ("s1", dict(ld_att=258)), ("s2", dict(ld_att=226)),
        ("s1", dict(ldw=120)), ("chg", dict(ldw=120)), ("s2", dict(ldw=216)), ("s1", dict(ldw=132)), ("s2", dict(ldw=228)),
        ("s2", dict(H=92, W=92)),                                                         # 529 windows: no whole number of pairs
        ("s1", dict(xo=4)), ("s2", dict(xo=4)), ("s1", dict(wo=2)), ("s2", dict(wo=2)), ("s1", dict(ao=2)), ("chg", dict(ao=2)), ("s2", dict(ao=2)),
    ]
    for name, fault in refused:
        rc = call(name, **fault)
        assert rc == L.E_UNSUPPORTED, (name, fault, rc)
        assert bool((flat == FILL).all()), (name, fault, "att was written")
    assert lib.ovo_hip_last_error() == message
    for name in base:                                              # nothing wrong: launched, and the block is written
        f = WC.FORMS[name]
        B, H, W, _, ld = base[name]
        rows = B * (H // f.ws) * (W // f.ws) * (16 if name != "s1" else 64)
        assert call(name) == 0
        block = flat[:rows * ld].view(rows, ld)
        assert bool((block[:, :f.d_out] != FILL).all()) and bool((block[:, f.d_out:] == FILL).all()) and bool((flat[rows * ld:] == FILL).all())
        assert block[:, :f.d_out].view(torch.bfloat16).isfinite().all()
        flat.fill_(FILL)
    assert call("s1", ao=8) == 0 and call("s2", H=68, W=76, B=2) == 0 and call("s1", H=56, W=592) == 0     # 8-byte aligned att; the ragged shape; 518 windows
