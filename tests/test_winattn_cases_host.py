"""The inputs of tests/test_gpu_window_attention.py are not vacuous (no GPU): every planted mistake of tests/winattn_cases.py moves every window it
touches by more than ten times the case's own rounding noise E_w, the table reaches the edges of the window walk it claims, the peaked inputs are
peaked and their special rows are what they say, and `reference` is the header's formula.  These are conditions on tests/winattn_cases.py, never on
the kernel; a case that fails one gets other inputs, not a weaker condition.  One line per case is printed (pytest -s)."""
import pytest
import torch

import winattn_cases as WC


@pytest.mark.parametrize("case", WC.CASES, ids=WC.case_ids(WC.CASES))
def test_every_mistake_moves_every_window_it_touches_by_ten_times_the_noise(case):
    e, rms = WC.noise(case)
    e_w = float(e.max())
    right = WC.references(case)[0]
    assert right.isfinite().all() and 0.0 < e_w < 0.05             # (the NaN weight columns and nothing else non-finite is in the inputs)
    line = "[winattn case] %-16s %5d windows, rms %.3f, E_w %.3e (mean over windows %.3e); mistakes, smallest distance / E_w:" % (
        case.name, WC.geometry(case)[3], rms, e_w, float(e.mean()))
    smallest = float("inf")
    for mistake in WC.MISTAKES + ("pool_zero",):
        if not WC.applies(case, mistake):
            continue
        windows = WC.touched(case, mistake)
        if not windows.any():                                     # (no walk mistake is invisible in this table: H != W in every case)
            line += " %s -" % mistake
            continue
        wrong = WC.reference(case, True, mistake)
        moved = WC.window_rms(wrong - right, case, WC.judged_rows(case, mistake))[windows] / rms
        line += " %s %.1f (%d)" % (mistake, float(moved.min()) / e_w, int(windows.sum()))
        smallest = min(smallest, float(moved.min()) / e_w)
        assert float(moved.min()) > 10.0 * e_w, (case.name, mistake, float(moved.min()), e_w)
        untouched = WC.window_rms(wrong - right, case)[~windows]
        if mistake != "pool_zero":                              # (that one is judged in the all-negative window alone; it moves others too)
            assert not untouched.numel() or float(untouched.max()) < 1e-9, (case.name, mistake)
    print("\n" + line + "; smallest of all %.1f" % smallest)
    for mistake in WC.WALK:
        assert WC.touched(case, mistake).any(), (case.name, mistake)


def test_the_table_reaches_the_edges_it_claims():
    by_edge = lambda edge, f: [c for c in WC.CASES if c.edge == edge and c.form == f]
    assert len({c.name for c in WC.CASES}) == len(WC.CASES) and {c.form for c in WC.CASES} == set(WC.FORMS) and all(f.rule for f in WC.FORMS.values())
    for c in WC.CASES:
        f = WC.form(c)
        nwh, nww, per, n_win, tk, tq = WC.geometry(c)
        assert c.H % f.ws == 0 and c.W % f.ws == 0 and c.H != c.W
        assert n_win >= WC.MIN_WINDOWS and (f.name != "s2" or n_win % 2 == 0)
        assert WC.ld_att(c) >= f.d_out and WC.ld_att(c) % 4 == 0 and WC.ldw(c) >= f.kmin and WC.ldw(c) % 8 == 0
        assert (tk, tq) == {"s1": (64, 64), "chg": (64, 16), "s2": (16, 16)}[f.name]
    for f in WC.FORMS:
        minimum, ragged, loop, free = (by_edge(e, f) for e in ("minimum", "ragged", "loop", "free"))
        assert {c.kind for c in minimum} == {"flat", "peaked"} and all(WC.geometry(c)[3] == WC.MIN_WINDOWS and c.B == 1 for c in minimum)
        assert len(ragged) == 2 and ragged[0][3:6] == (ragged[1].B, ragged[1].W, ragged[1].H) and ragged[0].H < ragged[0].W     # and its H > W twin
        for c in ragged:
            per, n_win = WC.geometry(c)[2:4]
            assert c.B > 1 and n_win < WC.SLOTS
            if f == "s2":       # 646 windows = 323 tasks of a pair; 323 windows per image: task 161 = windows 322 | 323 = the last of image 0 | the first of image 1
                assert (n_win, per) == (646, 323) and (2 * 161) // per == 0 and (2 * 161 + 1) // per == 1
                assert (n_win // 2) % WC.WG_WAVES != 0              # and the last workgroup with work is not full
            else:               # 561 windows, 187 per image: not a multiple of 8, and both image changes fall inside a workgroup's 8 windows
                assert (n_win, per) == (561, 187) and n_win % WC.WG_WAVES != 0 and all((b * per) % WC.WG_WAVES != 0 for b in range(1, c.B))
        (c,) = loop
        slots = WC.geometry(c)[3] // (2 if f == "s2" else 1)
        assert WC.SLOTS < slots < 2 * WC.SLOTS and slots % WC.WG_WAVES != 0 and c.B > 1        # some waves take a second trip; the last trip is ragged
        assert slots == (2115 if f == "s2" else 2175)
        assert [(c.bias, WC.ld_att(c) - WC.FORMS[f].d_out, c.lead) for c in free] == [(False, 0, 4), (True, 4, 0)] and all(WC.ldw(c) == WC.FORMS[f].kmin + 8 for c in free)
    # the walk-independence runs: the last image in slot 0 of a grid the launcher takes
    for c in WC.CASES:
        if c.edge in ("ragged", "loop"):
            wc, first = WC.walk_case(c)
            n = WC.geometry(wc)[3]
            assert n >= WC.MIN_WINDOWS and (c.form != "s2" or n % 2 == 0) and first == WC.geometry(c)[3] - WC.geometry(c)[2] > 0


@pytest.mark.parametrize("case", [c for c in WC.CASES if c.kind == "peaked"], ids=lambda c: c.name)
def test_peaked_inputs_are_peaked_and_their_special_rows_are_special(case):
    f, inp = WC.form(case), WC.inputs(case)
    q, k, _ = WC.qkv(case, False)
    p, total = WC.probabilities(q, k)
    largest = float((p / total).amax(-1).mean())
    flat = WC.case(case.name.replace("peaked", "flat"))
    pf, tf = WC.probabilities(*WC.qkv(flat, False)[:2])
    largest_flat = float((pf / tf).amax(-1).mean())
    rows = WC.window_rows(case)
    x = inp.x.reshape(-1, f.d)
    const, big = x[rows[WC.SPECIAL_ROWS, 1]], x[rows[WC.SPECIAL_ROWS, 2]]
    assert (const == const[0]).all() and (big == 3e4).all()
    # LayerNorm of both is beta -- and a mean one f32 step off 3e4 would not be: (2^-9)^2 against eps
    xn = WC._layer_norm(torch.stack([const, big]).double(), inp.ln_g.double(), inp.ln_b.double(), f.d)
    assert torch.equal(xn[0], inp.ln_b.double()) and torch.equal(xn[1], inp.ln_b.double())
    assert (2.0 ** -9) ** 2 > WC.EPS
    qn = WC.qkv(case, False, windows=slice(WC.SPECIAL_NEGQ, WC.SPECIAL_NEGQ + 1))[0]
    qr = WC.qkv(case, True, windows=slice(WC.SPECIAL_NEGQ, WC.SPECIAL_NEGQ + 1))[0]
    print("\n[winattn peaked] %-16s mean largest probability %.3f (flat: %.3f); largest q of the negative window %.3f" % (case.name, largest, largest_flat, float(qn.max())))
    assert largest > 0.8 and largest_flat < 0.3                 # (16 keys in the 4 x 4 windows: uniform is 0.06)
    assert float(qn.max()) < 0.0 and float(qr.max()) < 0.0         # (pooled where the form pools: the max of each cell is negative, so every q is)
    assert float(WC.qkv(case, False, windows=slice(0, 64))[0].max()) > 0.0   # ... which is special


def test_reference_is_the_header_formula_window_by_window():
    """`reference` (gathers, batched products) against the formula written out with loops for a few windows of the two-image cases, both ways round;
    and r16 is bf16's round-to-nearest-even."""
    for name, wins in (("s1-ragged", (0, 186, 187, 560)), ("chg-ragged-tall", (0, 17, 373, 374)), ("s2-ragged", (0, 322, 323, 645))):
        c = WC.case(name)
        f, inp = WC.form(c), WC.inputs(c)
        nwh, nww, per, n_win, tk, tq = WC.geometry(c)
        got = WC.references(c)[1].reshape(n_win, tq, f.d_out)
        w, bias = inp.w[:, :f.d].double(), inp.bias.double()
        for win in wins:
            b, wy, wx = win // per, (win % per) // nww, win % nww
            block = inp.x[b, wy * f.ws:(wy + 1) * f.ws, wx * f.ws:(wx + 1) * f.ws].double()                   # [ws, ws, d]
            xn = torch.nn.functional.layer_norm(block, (f.d,), inp.ln_g.double(), inp.ln_b.double(), WC.EPS)
            t = (xn @ w.T + bias).reshape(f.ws, f.ws, 3, f.heads, WC.HD)
            for h in range(f.heads):
                q, k, v = (t[:, :, i, h] for i in range(3))                                                       # [ws, ws, 56]
                if f.pool:
                    q = torch.stack([torch.stack([q[2 * py:2 * py + 2, 2 * px:2 * px + 2].reshape(4, WC.HD).amax(0) for px in range(4)]) for py in range(4)])
                q, k, v = q.reshape(-1, WC.HD), k.reshape(-1, WC.HD), v.reshape(-1, WC.HD)
                want = torch.softmax((q @ k.T) * 0.6931471805599453, -1) @ v                                      # exp2(s) = exp(s ln 2)
                torch.testing.assert_close(got[win, :, h * WC.HD:(h + 1) * WC.HD], want, atol=1e-12, rtol=1e-10)
    assert torch.equal(WC.r16(torch.tensor([1.01171875, 1.00390625, 1.005], dtype=torch.float64)), torch.tensor([1.015625, 1.0, 1.0078125], dtype=torch.float64))   # 8 bits, ties to even


def test_inputs_are_seeded_and_the_guards_are_where_no_kernel_reads():
    for c in (WC.case("s1-min-peaked"), WC.case("s2-free-nobias")):
        a = WC.inputs(c)
        WC.inputs.cache_clear()
        b = WC.inputs(c)
        f = WC.form(c)
        assert torch.equal(a.x, b.x) and torch.equal(a.w.view(torch.int16), b.w.view(torch.int16)) and a.w.dtype == torch.bfloat16
        assert a.w.shape == (3 * f.d_out, WC.ldw(c)) and a.w[:, :f.d].isfinite().all() and (a.w[:, f.d:f.kmin] == 0).all() and a.w[:, f.kmin:].isnan().all()
        assert (a.bias is None) == (not c.bias)
    free, full = WC.inputs(WC.case("s1-free-nobias")), WC.inputs(WC.case("s1-min-flat"))          # same values, other pitch, no bias
    assert torch.equal(free.x, full.x) and torch.equal(free.w[:, :128], full.w[:, :128]) and free.w.shape[1] == 136 and free.w[:, 128:].isnan().all()
    c = WC.case("s2-ragged")
    wc, first = WC.walk_case(c)
    wi = WC.walk_inputs(c)
    assert torch.equal(wi.x[0], WC.inputs(c).x[-1]) and not torch.equal(wi.x[1], WC.inputs(c).x[0]) and wi.x.shape[0] == wc.B == 2
