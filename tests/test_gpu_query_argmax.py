"""-m gpu: the fused query argmax (ovo_cast_f32 -> ovo_gemm_argmax -> ovo_decode_best) against an exact float64 reference in every epilogue form.

The per-row first-max argmax exists in four hand-written copies (the ring kernels' generic epilogue, the ping-pong kernel's running form, its
`argmax_only` form and its staged 16-bit form), all ending in one 64-bit atomicMax on (order-preserving score bits << 32 | ~column).  A wrong class
is silent, so the inputs here are built to make every branch decisive: rows whose scores are ALL negative (the sign branch of the key; the zero
columns of the vocabulary padding would win if they were let in), columns that tie bit for bit in every lane group, wave and workgroup tile, and
thresholds that equal a returned confidence exactly.  Every input is generated on the CPU from a seeded generator; the reference is the float64
product of the inputs rounded to the map's dtype (SigLIP epilogue in float64).

Bounds: |conf - reference maximum| <= 3e-6 (same rounded inputs, accumulation only: the bound of test_large_vocabulary_query).  A row is
AMBIGUOUS when the reference's two best distinct scores lie within 6e-6 (twice that bound): either column is accepted there, and at most 1 % of
the rows may be such.  Under SigLIP a row is ambiguous only when BOTH gaps are below 6e-6: the one between the reference's scores (the sigmoid
values: the plain rule) and the one between the scores before the sigmoid.  The sigmoid is monotone, so the winner is the same in both; the second
condition only ever removes rows from the ambiguous set.  It matters on the all-negative rows, where the scores are ~1e-3 and 6e-6 on them alone
would call over 40 % of the rows ambiguous (a cosine gap of 5e-4): there a cosine gap of 6e-6 is 7e-5 in the logit, ~100 times the f32 rounding
of alpha * s + bias, __expf and the division, and the exact column is demanded.  On mixed-sign rows (sigmoid slope up to ~3) the first condition
is the binding one.

Measured on an MI355X (the figures are _check_against_reference's return value): every (form, dtype, q) has 0 to 4 ambiguous rows (at most
2 of 300) and the kernel returned the reference's own column on each of them, so no alternative column had to be accepted; |conf - reference|
<= 3.8e-7 everywhere.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CONF_TOL = 3e-6
AMBIGUOUS = 6e-6
LS, LB = 2.5, -1.0                       # the SigLIP epilogue of every siglip form: sigmoid(exp(2.5) s - 1); padded columns sit at sigmoid(-1) = 0.269
VOCABS = (64, 130, 257, 1001)            # the large-path threshold, three kinds of ragged last tile, 2 or 3 padded columns
DTYPES = [torch.float16, torch.bfloat16]
RING_TILES = ("64x64", "64x128", "128x64", "128x128")
PP_TILES = ("256x256", "256x128")
RING_KIND = {"128x128": 4, "128x64": 5, "64x128": 6, "64x64": 7}     # csrc/common.h: the profiler's kinds
PP_KIND = {"256x256": 3, "256x128": 0}


class Form:
    """One way of reaching one of the four argmax epilogues through clip_utils.similarity."""

    def __init__(self, name, tile, shapes, want_sim=True, sim16=False, staged=None, siglip=False):
        self.name, self.tile, self.shapes, self.want_sim, self.sim16, self.staged, self.siglip = name, tile, shapes, want_sim, sim16, staged, siglip

    def __repr__(self):
        return self.name


def _forms():
    out = []
    ring = [(5, 128), (300, 128), (5, 96), (300, 96)]             # d = 96: K % 64 != 0, the BK = 32 instantiations
    pp = [(300, 128), (513, 128)]                                   # d % 64 == 0, or the dispatcher falls back to a ring kernel without saying so
    for sig in (False, True):
        s = "-siglip" if sig else ""
        for t in RING_TILES:
            out.append(Form(f"ring-{t}{s}", t, ring, siglip=sig))
        for t in PP_TILES:
            out.append(Form(f"running-{t}{s}", t, pp, siglip=sig))
            out.append(Form(f"argmax_only-{t}{s}", t, pp, want_sim=False, siglip=sig))
        out.append(Form(f"auto{s}", None, [(2309, 768)], want_sim=False, siglip=sig))
    for t in PP_TILES:                                              # (act must be 0 for the staged epilogue: no SigLIP form of it exists)
        out.append(Form(f"staged-{t}", t, pp, sim16=True, staged=True))
        out.append(Form(f"unstaged16-{t}", t, pp, sim16=True, staged=False))
    return out


FORMS = _forms()
form_params = pytest.mark.parametrize("form", FORMS, ids=repr)
dtype_params = pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])


# ---- inputs (CPU, seeded) and float64 references; computed once per shape and shared by every form ----

def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _round(x, dtype):
    """float64 values of x (f32) rounded to `dtype` by torch on the CPU."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).double().numpy()


def _epilogue(s, siglip):
    return 1.0 / (1.0 + np.exp(-(s * math.exp(LS) + LB))) if siglip else s


@functools.lru_cache(maxsize=None)
def _cluster(n, d, q, seed=11):
    """All-negative scores: u a unit vector, T_j = unit(u + 0.7 g_j / sqrt d), F_i = -unit(u + 0.7 h_i / sqrt d)."""
    rng = np.random.default_rng([seed, n, d, q])
    u = _unit(rng.standard_normal(d))
    T = _unit(u + 0.7 * rng.standard_normal((q, d)) / math.sqrt(d))
    F = -_unit(u + 0.7 * rng.standard_normal((n, d)) / math.sqrt(d))
    return F.astype(np.float32), T.astype(np.float32), u.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _mixed(n, d, q, seed=12):
    rng = np.random.default_rng([seed, n, d, q])
    return _unit(rng.standard_normal((n, d))).astype(np.float32), _unit(rng.standard_normal((q, d))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _scores(kind, dtype, n, d, q):
    """(F f32, T f32, float64 scores of the rounded inputs before any epilogue)."""
    F, T = _cluster(n, d, q)[:2] if kind == "negative" else _mixed(n, d, q)
    ref = _round(F, dtype) @ _round(T, dtype).T
    ref.setflags(write=False)
    return F, T, ref


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _run(form, monkeypatch, Fd, Td, th, **kw):
    """One query through `form`; (scores | None, classes, confidences) as numpy."""
    from ovo_amd.utils import clip_utils as CU
    if form.tile is None:
        monkeypatch.delenv("OVO_GEMM_TILE", raising=False)
    else:
        monkeypatch.setenv("OVO_GEMM_TILE", form.tile)
    if form.staged is False:
        monkeypatch.setenv("OVO_8P_BEST_STAGED", "0")
    else:
        monkeypatch.delenv("OVO_8P_BEST_STAGED", raising=False)
    if th is not None:
        kw["th"] = th
    if form.siglip:
        kw.update(siglip=True, logit_scale=LS, logit_bias=LB)
    sim, cls, conf = CU.similarity(Fd, Td, want_argmax=True, want_sim=form.want_sim, sim_dtype=(Fd.dtype if form.sim16 else None), **kw)
    assert (sim is not None) == form.want_sim
    if sim is not None:
        assert sim.shape == (Fd.shape[0], Td.shape[0]) and sim.dtype == (Fd.dtype if form.sim16 else torch.float32)
        sim = sim.float().cpu().numpy()
    return sim, cls.cpu().numpy(), conf.cpu().numpy()


def _check_against_reference(form, monkeypatch, dtype, kind):
    """Section 2: classes / confidences of one form at th = -10 against the float64 reference, for every shape and vocabulary of the form.
    Returns, per case, (q, n, d, ambiguous rows, ambiguous rows on which the second-best column was returned and accepted, largest |conf error|)."""
    figures = []
    for q in VOCABS:
        for n, d in form.shapes:
            F, T, pre = _scores(kind, dtype, n, d, q)
            ref = _epilogue(pre, form.siglip)
            if kind == "negative":
                assert pre.max() < -0.4 and pre.min() > -0.9           # every row all-negative: a padded column (0, or sigmoid(-1)) would win each of them
                assert _epilogue(0.0, form.siglip) > ref.max()
            sim, cls, conf = _run(form, monkeypatch, _dev(F, dtype), _dev(T), -10.0)
            want = ref.argmax(1)
            order = np.argsort(pre, axis=1)[:, -2:]                    # second best, best (the epilogue is monotone: the same two columns after it)
            rows = np.arange(n)
            gap_pre = pre[rows, order[:, 1]] - pre[rows, order[:, 0]]
            gap_ref = ref[rows, order[:, 1]] - ref[rows, order[:, 0]]
            ambiguous = (gap_ref < AMBIGUOUS) & (gap_pre < AMBIGUOUS)   # plain forms: one and the same gap
            took_other = ambiguous & (cls != want) & (cls == order[:, 0])
            figures.append((q, n, d, int(ambiguous.sum()), int(took_other.sum()), float(np.abs(conf - ref.max(1)).max())))
            assert cls.min() >= 0 and cls.max() < q, (form, q, n, d, int(cls.max()))     # never a padded column
            bad = np.flatnonzero((cls != want) & ~took_other)
            assert bad.size == 0, (str(form), q, n, d, bad[:8], cls[bad[:8]], want[bad[:8]])
            assert float(np.abs(conf - ref.max(1)).max()) <= CONF_TOL, (str(form), q, n, d)
            assert ambiguous.mean() <= 0.01, (str(form), q, n, d, int(ambiguous.sum()))
            if sim is not None and not form.sim16:                      # the f32 scores the same launch stored: the winner is THEIR first maximum, exactly
                assert np.array_equal(cls, sim.argmax(1)) and np.array_equal(conf, sim.max(1))
                assert float(np.abs(sim - ref).max()) <= CONF_TOL
    return figures


# ---- 1. every form runs the kernel it names ----

@form_params
def test_forms_reach_the_kernel_they_name(form, monkeypatch):
    """The profiler's launch kinds (csrc/common.h) for one query per shape and dtype of the form: a forced tile that the dispatcher declined would
    otherwise run a ring kernel silently and the tests below would cover something else.
    What this establishes: WHICH KERNEL ran (ring tile, or the 256 x 256 / 256 x 128 ping-pong kernel).  What it does not: the profiler has one
    kind per tile, so the ping-pong kernel's choice among its running, argmax_only, staged and unstaged epilogues is not observed.  That choice is
    read off the code (gemm8p.hip: launch8p, k_gemm8p): argmax_only = no score matrix stored (want_sim=False); staged = 2-byte scores stored, no
    activation, OVO_8P_BEST_STAGED unset and OVO_8P_NO_SLAB16 unset; everything else runs finish4 / finish_best.  The forms below set exactly
    those inputs, and the suite runs with neither knob set in its environment."""
    from ovo_amd import _lib as L
    lib = L.load()
    assert "OVO_8P_NO_SLAB16" not in os.environ
    for dtype in DTYPES:
        for n, d in form.shapes:
            F, T, _ = _scores("mixed", dtype, n, d, 257)
            Fd, Td = _dev(F, dtype), _dev(T)
            L.check(lib.ovo_profile_start())
            _run(form, monkeypatch, Fd, Td, -10.0)
            ms, work, cnt = (C.c_double * 10)(), (C.c_double * 10)(), (C.c_int64 * 10)()
            L.check(lib.ovo_profile_stop(ms, work, cnt, 10))
            kinds = [i for i in range(10) for _ in range(cnt[i])]
            if form.tile is None:
                assert len(kinds) == 1 and kinds[0] in (0, 3, 4, 5, 6, 7), kinds
            else:
                assert kinds == [RING_KIND[form.tile] if form.tile in RING_KIND else PP_KIND[form.tile]], (str(form), dtype, n, d, kinds)


# ---- 2. all-negative rows with a padded vocabulary; mixed signs ----

@dtype_params
@form_params
def test_all_negative_rows_never_take_a_padded_column(form, dtype, monkeypatch):
    """Every reference score lies in [-0.9, -0.4]: a padded column, at exactly 0 (sigmoid(-1) under SigLIP), wins every row it is let into --
    the `n + r < g.n_valid` guards decide the class -- and the key's sign branch, at its encode site and in the decoder, runs on every row."""
    _check_against_reference(form, monkeypatch, dtype, "negative")


@dtype_params
@form_params
def test_mixed_sign_rows(form, dtype, monkeypatch):
    """Plain random unit vectors through the same harness: scores of both signs in every row, positive maxima."""
    _check_against_reference(form, monkeypatch, dtype, "mixed")


# ---- 3. exact ties at every level of the reduction ----

TIE_Q, TIE_G = 1001, 7


TIE_GAP_SIGLIP = 2e-6


def _separable(top2):
    """Rows of (second best, best) reference scores before the epilogue that every form must tell apart (see _tie_case)."""
    return (top2[:, 1] - top2[:, 0] > AMBIGUOUS) & (_epilogue(top2[:, 1], True) - _epilogue(top2[:, 0], True) > TIE_GAP_SIGLIP)


@functools.lru_cache(maxsize=None)
def _tie_case(construction, dtype, n, d, s):
    """q = 1001 columns carrying G = 7 distinct text vectors: columns [0, s) the designated loser (vector 0), the rest a seeded random choice among
    the others.  Identical weight rows accumulate in the same order, so tied columns are bit-equal; each winner is attained at ~140 columns spread
    over every lane group, wave and workgroup tile.  The LAST descriptor row is all zeros (an unobserved map point).

    The test demands the exact column on EVERY row, so every row's best and second-best vector must be separable by a correct kernel in every form.
    Random rows are not always: of 2n + 8 candidates the first n are kept whose two best vectors are
      more than 6e-6 apart before the epilogue (AMBIGUOUS, the plain rule: twice the accumulation bound), and
      more than 2e-6 apart after the SigLIP epilogue.  The kernel's f32 sigmoid(alpha s + b) is monotone in s, so it can only get two separated
        scores wrong by rounding them to the SAME value, which needs their true values within twice its error; that error is <= 1e-6: |logit|
        <= 13.2, so the two f32 roundings of alpha s + b and that of alpha are <= 1.8e-6 in the logit, x the sigmoid's slope <= 1/4, plus 2 ulp of
        __expf and the division's rounding, ~2e-7.  This is what bites near saturation: cosines of 0.8 are logits of ~9, where the sigmoid's slope
        is 1e-4 and a cosine gap of 1e-4 is one f32 ulp of the score.
    One table serves every form, SigLIP or not.  The test asserts both gaps again on the rows it is handed."""
    rng = np.random.default_rng([13, n, d, s, construction == "positive"])
    m = 2 * n + 8
    if construction == "positive":
        base = _unit(rng.standard_normal((TIE_G, d)))
        F = _unit(rng.random((m, TIE_G - 1)) @ base[1:] - 0.5 * base[0])
    else:
        Fc, Tc, u = _cluster(m, d, TIE_G - 1, seed=14)
        base, F = np.concatenate([u[None], Tc]), Fc
    base = base.astype(np.float32)
    top2 = np.sort(_round(F, dtype) @ _round(base, dtype).T, axis=1)[:, -2:]
    F = F[_separable(top2)][:n]
    assert F.shape[0] == n
    F = np.concatenate([F, np.zeros((1, d))]).astype(np.float32)
    col = np.concatenate([np.zeros(s, np.int64), rng.integers(1, TIE_G, TIE_Q - s)])
    pre = _round(F, dtype) @ _round(base, dtype).T                       # float64 scores of the 7 distinct vectors
    first = np.array([int(np.flatnonzero(col == k)[0]) if (col == k).any() else -1 for k in range(TIE_G)])
    return F, base[col], pre, first


@pytest.mark.parametrize("construction", ["positive", "negative"])
@dtype_params
@form_params
def test_tied_columns_keep_the_first(form, dtype, construction, monkeypatch):
    """Equal scores keep the smaller column -- in the lane, in the two shuffles, across waves (the atomicMax) and across workgroups (the complemented
    column in the key's low half).  The class of a row is the FIRST column that carries its best vector."""
    for n, d in form.shapes:
        for s in (0, 70, 300, 800):
            F, T, pre, first = _tie_case(construction, dtype, n, d, s)
            rows = pre[:-1]
            top2 = np.sort(rows, axis=1)[:, -2:]
            assert _separable(top2).all()                                 # best and second-best VECTOR never come close: no row is ambiguous here
            best = rows.argmax(1)
            assert best.min() >= 1                                        # the loser never wins
            if n >= 300:
                assert set(best.tolist()) == set(range(1, TIE_G))         # every other vector wins some rows (5 rows cannot show 6 winners)
            Fd, Td = _dev(F, dtype), _dev(T)
            sim, cls, conf = _run(form, monkeypatch, Fd, Td, -1.0)
            want = first[best]
            bad = np.flatnonzero(cls[:-1] != want)
            assert bad.size == 0, (str(form), n, d, s, bad[:8], cls[bad[:8]], want[bad[:8]])
            ref = _epilogue(rows.max(1), form.siglip)
            assert float(np.abs(conf[:-1] - ref).max()) <= CONF_TOL
            if sim is not None and not form.sim16:
                assert np.array_equal(cls, sim.argmax(1)) and np.array_equal(conf, sim.max(1))
            # the all-zero row: every valid column ties at epilogue(0) -- class 0; kept at th = -1, and at the default th = 0 an unobserved point
            # stays unlabelled (plain scores: 0 <= 0).  Under SigLIP its score is sigmoid(-1) > 0, so it keeps class 0 at either threshold.
            zero = float(_epilogue(0.0, form.siglip))
            assert cls[-1] == 0 and abs(float(conf[-1]) - zero) <= (CONF_TOL if form.siglip else 0.0)
            _, cls0, conf0 = _run(form, monkeypatch, Fd, Td, None)
            if form.siglip:
                assert cls0[-1] == 0 and conf0[-1] == conf[-1]
            else:
                assert cls0[-1] == -1 and conf0[-1] == 0.0
            keep = conf[:-1] > 0.0                                        # default threshold on the other rows: strictly positive scores survive, unchanged
            assert np.array_equal(cls0[:-1], np.where(keep, cls[:-1], -1)) and np.array_equal(conf0[:-1], np.where(keep, conf[:-1], np.float32(0)))


# ---- 4. threshold semantics on the large path ----

@pytest.mark.parametrize("kind", ["negative", "mixed"])
@dtype_params
@form_params
def test_threshold_equal_to_a_returned_confidence(form, dtype, kind, monkeypatch):
    """th = one row's returned confidence, bit for bit: rows with conf <= th (that row included) come back as class -1 / confidence 0, every other
    row unchanged -- the atomicMax makes the result independent of the order the workgroups arrive in."""
    q = 1001
    for n, d in form.shapes:
        F, T, _ = _scores(kind, dtype, n, d, q)
        Fd, Td = _dev(F, dtype), _dev(T)
        _, cls, conf = _run(form, monkeypatch, Fd, Td, -10.0)
        assert (conf < 0).all() if (kind == "negative" and not form.siglip) else (conf > 0).all()
        pick = int(np.argsort(conf, kind="stable")[n // 2])              # the median row: both sides of the threshold are populated (n >= 5)
        th = float(conf[pick])
        _, cls2, conf2 = _run(form, monkeypatch, Fd, Td, th)
        drop = conf <= np.float32(th)
        assert drop[pick] and drop.any() and not drop.all()
        assert np.array_equal(cls2, np.where(drop, -1, cls)), (str(form), n, d)
        assert np.array_equal(conf2.view(np.uint32), np.where(drop, np.float32(0), conf).view(np.uint32)), (str(form), n, d)


# ---- 5. direct tests of ovo_decode_best, ovo_row_argmax, ovo_cast_f32 ----

def _key(score, col):
    """The documented encoding: order-preserving bits of the f32 score in the high half (negative: all bits complemented; else sign bit set),
    0xffffffff - column in the low half."""
    u = np.asarray(score, np.float32).view(np.uint32).astype(np.uint64)
    hi = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xffffffff), u | np.uint64(0x80000000))
    return (hi << np.uint64(32)) | (np.uint64(0xffffffff) - np.asarray(col, np.uint64))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_decode_best_vs_host_restatement(n):
    from ovo_amd import _lib as L
    lib = L.load()
    scores = np.array([0.0, -0.0, 1.0, -1.0, 1e-40, -1e-40, 3e38, -3e38, np.inf], np.float32)
    cols = np.array([0, 1, 2 ** 31 - 2], np.uint64)
    s_all, c_all = np.repeat(scores, cols.size), np.tile(cols, scores.size)
    keys_all = np.concatenate([_key(s_all, c_all), np.zeros(1, np.uint64)])                 # + the key 0: no column ever arrived
    s_all, c_all = np.concatenate([s_all, np.zeros(1, np.float32)]), np.concatenate([c_all.astype(np.int64), -np.ones(1, np.int64)])
    # keys order as (score, then smaller column): what the atomicMax relies on (-0.0 sorts below +0.0 in the key, as its bits do)
    finite = np.array([-3e38, -1.0, -1e-40, -0.0, 0.0, 1e-40, 1.0, 3e38, np.inf], np.float32)
    ordered = _key(np.repeat(finite, 3), np.tile(cols[::-1], finite.size))
    assert (np.diff(ordered.astype(object)) > 0).all() and ordered.min() > 0
    ths = []
    for s in scores:
        ths += [s, np.nextafter(s, np.float32(-np.inf)), np.nextafter(s, np.float32(np.inf))]
    ths += [np.float32(-np.inf), np.float32(-10.0)]
    for t_i, th in enumerate(ths):
        idx = (np.arange(n) + 5 * t_i) % keys_all.size                                      # a rotating window of the key table, the key 0 included
        if n == 1:
            idx = np.array([t_i % keys_all.size])
        keys, sc, co = keys_all[idx], s_all[idx], c_all[idx]
        best = torch.from_numpy(keys.view(np.int64).copy()).to(DEV)
        cls = torch.full((n,), -7, dtype=torch.int64, device=DEV)
        conf = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
        L.check(lib.ovo_decode_best(L.ptr(best), n, float(th), L.ptr(cls), L.ptr(conf), L.stream()))
        drop = (keys == 0) | (sc <= np.float32(th))                                         # threshold semantics of the reference: conf <= th is unlabelled
        want_cls, want_conf = np.where(drop, -1, co), np.where(drop, np.float32(0), sc)
        assert np.array_equal(cls.cpu().numpy(), want_cls), (n, float(th))
        assert np.array_equal(conf.cpu().numpy().view(np.uint32), want_conf.view(np.uint32)), (n, float(th))


# |kernel sigmoid - float64 sigmoid| over logits exp(2.5) s - 1, s in [-1, 1]: MEASURED on an MI355X (the kernel uses __expf), the test asserts twice that
ROW_ARGMAX_SIGMOID_ERR_MEASURED = 9.8e-8           # largest of the 15 cases below: 9.787e-08 (n = 16389, Q = 1004)
_ROW_ARGMAX_N = (1, 5, 16389)            # 16389 rows = 4098 blocks of 4 waves: beyond the 4096-block cap, so the grid-stride loop runs


@functools.lru_cache(maxsize=None)
def _row_scores(n, Q):
    """All-negative rows in [-0.9, -0.4) with the row maximum planted twice, at distance 1, 4, 256 and Q - 1 (row i takes the (i % 4)-th that fits)."""
    rng = np.random.default_rng([15, n, Q])
    S = (-0.9 + 0.5 * rng.random((n, Q))).astype(np.float32)
    dist = [t for t in (1, 4, 256, Q - 1) if t < Q]
    for i in range(n if n < 64 else 64):                             # the first 64 rows, and the last few (they run in the grid-stride loop's second trip)
        for r in {i, n - 1 - i}:
            t = dist[r % len(dist)]
            c = int(rng.integers(0, Q - t))
            S[r, c] = S[r, c + t] = np.float32(-0.39)
    S.setflags(write=False)
    return S


@pytest.mark.parametrize("Q", [4, 252, 256, 260, 1004])
@pytest.mark.parametrize("n", _ROW_ARGMAX_N)
def test_row_argmax_vs_numpy(n, Q):
    from ovo_amd import _lib as L
    lib = L.load()
    S0 = _row_scores(n, Q)

    def run(S, siglip, th, with_out=True):
        Sd = torch.from_numpy(S.copy()).to(DEV)
        cls = torch.full((n,), -7, dtype=torch.int64, device=DEV) if with_out else None
        conf = torch.full((n,), -7.0, dtype=torch.float32, device=DEV) if with_out else None
        L.check(lib.ovo_row_argmax(L.ptr(Sd), n, Q, int(siglip), LS, LB, float(th), L.ptr(cls), L.ptr(conf), L.stream()))
        return Sd.cpu().numpy(), (cls.cpu().numpy() if with_out else None), (conf.cpu().numpy() if with_out else None)

    # plain, all-negative, tied maxima: first maximum exactly, S untouched
    S, cls, conf = run(S0, False, -10.0)
    assert np.array_equal(S, S0)
    assert np.array_equal(cls, S0.argmax(1)) and np.array_equal(conf, S0.max(1))
    assert (np.sum(S0 == S0.max(1, keepdims=True), axis=1) >= 2)[: min(n, 64)].all()          # the ties are there
    # th equal to one row's confidence: that row and every row below it unlabelled, the others unchanged
    lo = S0.copy()
    lo[::2] -= np.float32(0.05)                                        # half the rows sit lower, so both sides are populated (n = 1: the row itself)
    _, cls_a, conf_a = run(lo, False, -10.0)
    th = float(conf_a[n // 2])
    _, cls_b, conf_b = run(lo, False, th)
    drop = conf_a <= np.float32(th)
    assert drop[n // 2] and (n == 1 or not drop.all())
    assert np.array_equal(cls_b, np.where(drop, -1, cls_a)) and np.array_equal(conf_b, np.where(drop, np.float32(0), conf_a))
    # SigLIP: S rewritten in place, classes exact against the kernel's own written S; S against the float64 sigmoid
    rng = np.random.default_rng([16, n, Q])
    X = (2.0 * rng.random((n, Q)) - 1.0).astype(np.float32)
    X[:: max(1, n // 64), Q - 1] = X[:: max(1, n // 64), 0] = np.float32(1.0)                    # the row maximum, tied at distance Q - 1, bit-equal after the sigmoid too
    Ss, cls_s, conf_s = run(X, True, 0.5)
    keep = Ss.max(1) > np.float32(0.5)
    assert np.array_equal(cls_s, np.where(keep, Ss.argmax(1), -1)) and np.array_equal(conf_s, np.where(keep, Ss.max(1), np.float32(0)))
    assert keep.any()
    err = float(np.abs(Ss.astype(np.float64) - _epilogue(X.astype(np.float64), True)).max())
    assert err <= 2 * ROW_ARGMAX_SIGMOID_ERR_MEASURED
    # out_cls = NULL with SigLIP only rewrites S: the same bits
    Sn, _, _ = run(X, True, 0.5, with_out=False)
    assert np.array_equal(Sn, Ss)
    # out_cls = NULL without SigLIP: nothing to do, S untouched
    Sp, _, _ = run(X, False, 0.5, with_out=False)
    assert np.array_equal(Sp, X)


def _cast_specials():
    h = [2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -15 + 2.0 ** -25, 6e-8, 5.96e-8, 1e-7,
         65504.0, 65519.996, 65520.0, 65536.0, 1e5, 3e38,                                       # fp16 overflow: 65520 is the tie that rounds to inf
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -10,            # fp16 halfway cases: to even (down, up), just above
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -7,                # bf16 halfway cases
         3.3895314e38, 3.4028235e38, 3.39e38,                                                    # bf16: the largest finite value, f32 max (-> inf), between
         1e-40, 1.1754944e-38, 9.18355e-41, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134,             # f32 subnormals: bf16 keeps them (its own subnormal range)
         0.0, np.inf]
    x = np.array(h, np.float32)
    return np.concatenate([x, -x, np.array([np.nan], np.float32), np.array([0x7f800001, 0xffc12345], np.uint32).view(np.float32)])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("n", [4, 1020, 1028, 4 * (524288 + 5)])
def test_cast_f32_bit_equal_to_torch(n, dtype):
    """ovo_cast_f32 (round to nearest even) against tensor.to(dtype) on the CPU; 4 x (524288 + 5) elements run the grid-stride loop's second trip."""
    from ovo_amd import _lib as L
    lib = L.load()
    sp = _cast_specials()
    rng = np.random.default_rng([17, n])
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 18, n))).astype(np.float32)        # every binade from far under fp16's subnormals to past its maximum
    if n == 4:
        xs = [np.array([-0.0, np.inf, np.nan, 2.0 ** -25], np.float32), np.array([65520.0, -np.inf, 1 + 2.0 ** -11, 1 + 2.0 ** -8], np.float32)]
    else:
        x[: sp.size] = sp
        x[-sp.size:] = sp[::-1]                                        # at both ends: the last elements belong to the loop's last trip
        xs = [x]
    for x in xs:
        xt = torch.from_numpy(x)
        want = xt.to(dtype)
        y = torch.full((n,), 7.0, dtype=dtype, device=DEV)
        L.check(lib.ovo_cast_f32(L.ptr(xt.to(DEV)), n, L.ptr(y), {torch.float16: 1, torch.bfloat16: 2}[dtype], L.stream()))
        got = y.cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan) and bool(nan.any()) == bool(np.isnan(x).any())
        assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
