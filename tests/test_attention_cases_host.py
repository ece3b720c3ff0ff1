"""The inputs of tests/test_gpu_attention_causal.py are not vacuous (no GPU): in every probe case of the table one key decides each probe row, the two
off-by-one masks move every probe row by far more than the GPU test tolerates, the poison copies differ only where no kernel may look, and
`reference` is the plain softmax.  These are conditions on tests/attention_cases.py, never on the kernel; a case that fails one gets other inputs,
not a weaker condition.  One line per probe case is printed (pytest -s)."""
import pytest
import torch

import attention_cases as AC


def _id(c):
    return "%dx%d-hd%d-shift%d-%s-%dx%d" % (c[:4] + ("prescaled" if c[4] else "scaled",) + c[5:])


@pytest.mark.parametrize("case", AC.PROBE_CASES, ids=_id)
def test_one_key_decides_every_probe_row_and_an_off_by_one_mask_shows(case):
    Tq, Tk, hd, shift, prescaled, b, h = case
    rows = AC.probe_rows(Tq, Tk, shift)
    qkv = AC.probe_case(Tq, Tk, hd, shift, prescaled, b=b, h=h)
    scale = AC.scales(hd, prescaled)[2]
    q, k, v = AC.split(qkv, Tq, Tk)
    # ---- the deciding key holds >= 0.9 of its row (for superdiag: if the mask let it through), with and without the mask
    keys = [i + shift for i in rows]
    weight = min(float(AC.probabilities(q, k, scale, causal, widen=shift)[:, :, rows, keys].min()) for causal in (1, 0))
    assert weight >= 0.9
    # ---- the mistake this input is there for moves every probe row of every (batch, head) pair by more than 0.5 in some element:
    # diag under j < i (row 0 is left without a key: NaN counts as moved), superdiag under j <= i + 1
    right, wrong = (AC.reference(q, k, v, scale, 1, widen=w)[:, :, rows] for w in (0, 1 if shift else -1))
    moved = torch.nan_to_num((wrong - right).abs(), nan=float("inf")).amax(-1)                  # [b, h, probe row]
    if b * h > 100:             # 65539 pairs of 8 elements: a pair whose v rows differ by < 0.5 everywhere exists by chance; every ROW still shows
        moved = moved.amax((0, 1))
    assert float(moved.min()) > 0.5                                 # (check 2 of the GPU test allows 0.1 on these rows)
    print("\n[attention probe] %-34s rows %s weight >= %.6f moved >= %.2f" % (_id(case), rows, weight, float(moved.min())))


def test_probe_rows_sit_on_every_boundary():
    assert AC.probe_rows(600, 600, 0) == [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 575, 576, 577, 599]
    assert AC.probe_rows(600, 600, 1)[-1] == 598                    # the last row whose key i + 1 exists
    assert AC.probe_rows(70, 200, 1)[-3:] == [64, 65, 69]           # key 70: past every query, masked for all of them
    assert AC.probe_rows(200, 70, 0)[-1] == 69 and AC.probe_rows(200, 70, 1)[-1] == 68     # rows >= Tk have no key of their own
    assert AC.probe_rows(1, 1, 0) == [0] and AC.probe_rows(1, 1, 1) == []
    for f, tq, tk, hd in AC.CASES:                                  # every case of the table has probe rows, both shifts, but the 1 x 1 problem
        assert AC.probe_rows(tq, tk, 0) and (AC.probe_rows(tq, tk, 1) or (tq, tk) == (1, 1))
        assert len(AC.probe_rows(tq, tk, 0)) < hd or hd >= 24


def test_reference_is_softmax_with_the_header_mask_rule():
    g = torch.Generator().manual_seed(5)
    for Tq, Tk in ((5, 5), (7, 3), (3, 7)):
        q, k, v = (torch.randn(1, 2, n, 8, generator=g).double() for n in (Tq, Tk, Tk))
        for causal in (0, 1):
            out = AC.reference(q, k, v, 0.3, causal)
            for i in range(Tq):                                     # row by row, over the visible keys only
                n = min(i + 1, Tk) if causal else Tk
                s = (q[0, :, i:i + 1] @ k[0, :, :n].transpose(-1, -2)) * 0.3
                want = torch.softmax(s, -1) @ v[0, :, :n]
                torch.testing.assert_close(out[0, :, i:i + 1], want, atol=1e-12, rtol=1e-12)
    q, k, v = (torch.randn(1, 1, 7, 8, generator=g) for _ in range(3))
    assert AC.reference(q, k, v, 1.0, 1, widen=-1)[0, 0, 0].isnan().all() and not AC.reference(q, k, v, 1.0, 1, widen=-1)[0, 0, 1:].isnan().any()
    assert torch.equal(AC.reference(q, k, v, 1.0, 1)[0, 0, 0], v[0, 0, 0].double())            # one visible key: the row IS v[0] (check 3 of the GPU test)


@pytest.mark.parametrize("Tq,Tk", [(70, 200), (200, 70), (33, 33)])
@pytest.mark.parametrize("causal", [0, 1])
def test_poison_copies_differ_only_where_nothing_may_be_read(Tq, Tk, causal):
    hd = 40
    first, second = AC.poison_case(Tq, Tk, hd, causal)
    assert first.shape == second.shape == (AC.B, max(Tq, Tk) + 3, 3, AC.H, hd)
    assert first[:, Tq:, 0].isnan().all() and first[:, Tk:, 1:].isnan().all() and second.isfinite().all()
    assert (second[:, Tq:, 0] == 1000).all() and (second[:, Tk:, 1:] == 1000).all()
    assert torch.equal(first[:, :Tq, 0], second[:, :Tq, 0]) and first[:, :Tq, 0].isfinite().all()
    seen = min(Tq, Tk) if causal else Tk                            # keys some query sees
    assert torch.equal(first[:, :seen, 1:], second[:, :seen, 1:]) and first[:, :Tk, 1:].isfinite().all()
    if causal and Tk > Tq:
        assert (first[:, Tq:Tk, 1:] != second[:, Tq:Tk, 1:]).float().mean() > 0.9
        a, b = (AC.packed_reference(t, Tq, Tk, hd ** -0.5, 1) for t in (first, second))
        assert torch.equal(a, b) and a.isfinite().all()             # the reference itself does not see them
    else:
        assert torch.equal(first[:, :Tk, 1:], second[:, :Tk, 1:])


def test_builders_are_seeded_and_the_table_is_whole():
    for fn, args in ((AC.random_case, (33, 33, 24)), (AC.probe_case, (70, 200, 56, 1))):
        a = fn(*args)
        fn.cache_clear()
        assert torch.equal(a, fn(*args)) and a.dtype == torch.bfloat16
    assert len({f.name for f in AC.FORMS}) == len(AC.FORMS) == 10 and all(f.cases and f.rule for f in AC.FORMS)
    assert {AC.form(n).name for n, *_ in AC.FREE_STRIDES} >= {"tiny", "a32_128q", "a16"}
    for f, tq, tk, hd in AC.CASES:                                  # the table's rows against the rules they quote
        tiny, no32 = tq <= 16 and tk <= 64 and hd <= 64, f.env.get("OVO_ATTN32") == "0"
        if f.name == "tiny":
            assert tiny and not f.env
        elif f.name.startswith("a32"):
            assert not f.env and not f.offset_out and not (tq <= 16 and tk <= 64)
            assert {"a32_64q": tq <= 64 and hd <= 64, "a32_128q": tq > 64 and hd <= 64, "a32_wide_hd": hd > 64}[f.name]
        else:
            assert no32 or f.offset_out
            assert not tiny or "OVO_ATTN_NO_TINY" in f.env
            trimmed = hd <= 64 and tk <= 64 and "OVO_ATTN_WIDE" not in f.env
            assert trimmed == (f.name == "a16_trim") or f.name in ("a16_by_alignment", "a16_gridy")
        if f.name == "a16_grid2d":
            assert tq > 64
        if f.name == "a16_gridy":
            assert f.bh[0] * f.bh[1] > 65535 and tq <= 64
