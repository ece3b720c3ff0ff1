"""Inputs, reference and case table for the causal-mask tests of `ovo_attention` (tests/test_attention_cases_host.py, tests/test_gpu_attention_causal.py):
a plain helper module, torch on the CPU only; nothing of `ovo_amd` is used.

`reference` is fp64 softmax attention on the bf16-rounded operands with the mask rule of include/ovo_hip.h: key j is visible to query i iff j <= i on
absolute indices, so with Tq > Tk the queries i >= Tk see every key and with Tq < Tk the keys j >= Tq are visible to nobody.

Random data cannot see a mask that is off by one key: a lost or leaked key moves row i by about |v| / (i + 1), under the tolerance from row ~50 on.
`probe_case` therefore plants, for each probe row i, ONE key whose scaled score with q[i] is G while every other score stays O(1): that key holds
all of the row's probability (the host test asserts >= 0.9 in fp64).  With shift = 0 (`diag`) it is key i, the last visible one -- a kernel that
masks j == i loses it; with shift = 1 (`superdiag`) it is key i + 1, the first masked one -- a kernel that lets it through returns v[i + 1].
`reference(..., widen=+-1)` makes exactly these two mistakes, and the host test proves that each moves every probe row by more than 0.5.

FORMS is the table of kernel forms the GPU test walks; every row quotes the dispatcher rule (ovo_amd/csrc/attention.hip, `ovo_attention`) that sends
its cases to the form, so that a change of the dispatcher is seen to empty the row."""
import collections
import functools
import math

import torch

B, H = 2, 3                                 # every case but the one with more than 65535 (batch, head) pairs
G = 24.0                                    # scaled score of a probe row with its deciding key (e^24 against a row of O(1) scores)
LOG2E = 1.4426950408889634
KINDS = ("random", "diag", "superdiag")     # the inputs of a case: random_case, probe_case with shift 0, with shift 1
# probe rows sit on both sides of every boundary the kernels have: 16-key sub-tile, 32-key block / 32-query wave, 64-key tile / 64-query workgroup,
# 128-query workgroup (and its multiples 256, 512), 192 = 3 tiles, 576 = 9 tiles
BOUNDARIES = (0, 16, 32, 64, 128, 192, 256, 512, 576)


# ------------------------------------------------------------------------------------------------------------------ reference
def split(qkv, Tq, Tk):
    """q [B, H, Tq, hd], k and v [B, H, Tk, hd]: views of the packed [B, T, 3, H, hd] tensor."""
    return tuple(qkv[:, :n, i].permute(0, 2, 1, 3) for i, n in ((0, Tq), (1, Tk), (2, Tk)))


def probabilities(q, k, scale, causal, widen=0):
    """f64 [B, H, Tq, Tk].  widen: the mask is j <= i + widen (0: the rule; +1 lets the first masked key through, -1 loses the last visible one --
    a row without a visible key is NaN)."""
    s = q.double() @ k.double().transpose(-1, -2) * scale
    if causal:
        i, j = torch.arange(q.shape[-2]).reshape(-1, 1), torch.arange(k.shape[-2]).reshape(1, -1)
        s = s.masked_fill(j > i + widen, float("-inf"))
    return torch.softmax(s, dim=-1)


def reference(q, k, v, scale, causal, widen=0):
    """f64 [B, H, Tq, hd] = softmax(q k^T scale + mask) v on the operands as given (the callers pass them bf16-rounded)."""
    return probabilities(q, k, scale, causal, widen) @ v.double()


def packed_reference(qkv, Tq, Tk, scale, causal, widen=0):
    """`reference` of a packed tensor, in the layout of the kernel's output: f64 [B, Tq, H hd]."""
    b, _, _, h, hd = qkv.shape
    return reference(*split(qkv, Tq, Tk), scale, causal, widen).permute(0, 2, 1, 3).reshape(b, Tq, h * hd)


def scales(hd, prescaled):
    """(what multiplies q before its bf16 rounding, ovo_attention_t.scale, the reference's scale).  prescaled: scale == 0, the queries carry
    log2(e) / sqrt(hd) and the scores are in log2 units, so the reference softmax takes ln 2 (test_attention_prescaled_queries)."""
    return (LOG2E / hd ** 0.5, 0.0, math.log(2.0)) if prescaled else (1.0, hd ** -0.5, hd ** -0.5)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _raw(b, h, T, hd, seed):
    return torch.randn(b, T, 3, h, hd, generator=torch.Generator().manual_seed(seed))


def _seed(*key):
    return sum(int(x) * m for x, m in zip(key, (1, 7, 131, 1009, 4099, 65537)))


def _pack(raw, q_mul):
    raw[:, :, 0] *= q_mul
    return raw.to(torch.bfloat16)


def _cached(build):
    """The builders are pure functions of their arguments: the forms share their inputs (the result is read-only by convention; the 25 MB inputs of
    the 65539-pair case are built when asked for and not kept)."""
    keep = functools.lru_cache(maxsize=32)(build)

    @functools.wraps(build)
    def get(*args, b=B, h=H, **kw):
        return (keep if b * h <= 100 else build)(*args, b=b, h=h, **kw)
    get.cache_clear = keep.cache_clear
    return get


@_cached
def random_case(Tq, Tk, hd, prescaled=False, b=B, h=H, T=None):
    """bf16 [b, T, 3, h, hd] as in test_attention_vs_torch: N(0, 1) with q doubled (peaked rows)."""
    raw = _raw(b, h, T or max(Tq, Tk), hd, _seed(Tq, Tk, hd, 2, b))
    raw[:, :, 0] *= 2.0
    return _pack(raw, scales(hd, prescaled)[0])


def probe_rows(Tq, Tk, shift):
    """Rows i in {b - 1, b, b + 1 : b in BOUNDARIES} whose deciding key i + shift exists, plus the last such row."""
    last = min(Tq - 1, Tk - 1 - shift)
    return sorted({i for b in BOUNDARIES for i in (b - 1, b, b + 1) if 0 <= i <= last} | ({last} if last >= 0 else set()))


@_cached
def probe_case(Tq, Tk, hd, shift, prescaled=False, b=B, h=H):
    """bf16 [b, T, 3, h, hd]: q ~ N(0, 1), k ~ 0.5 N(0, 1), v ~ N(0, 1), and for every probe row i
    k[i + shift] = G sqrt(hd) q[i] / |q[i]|^2 -- the scaled score of that one pair is G.
    hd < 24: random queries cross-talk too much (a deciding key scores high with OTHER probe queries too), so the probe queries are distinct
    coordinate axes there and the other queries have no component along those axes, which allows fewer than hd probe rows.  (With components
    the other rows score up to 57 against the axis keys; the kernel's second bf16 rounding of scale * q -- ovo_hip.h -- then moves 234 of
    the 4 M outputs of the 65539-pair case by up to 0.10, in fp64 on the CPU just as on the GPU: outside what the 2e-2 bound was stated for.)"""
    raw = _raw(b, h, max(Tq, Tk), hd, _seed(Tq, Tk, hd, shift, b))
    raw[:, :, 1] *= 0.5
    rows = probe_rows(Tq, Tk, shift)
    if hd < 24:
        assert len(rows) < hd, "no coordinate axis left for the other queries"
        raw[:, :, 0, :, :len(rows)] = 0.0
        for n, i in enumerate(rows):
            raw[:, i, 0] = 0.0
            raw[:, i, 0, :, n] = 2.0
    for i in rows:
        q = raw[:, i, 0].to(torch.bfloat16).float()                # what the kernel multiplies
        raw[:, i + shift, 1] = G * hd ** 0.5 * q / q.pow(2).sum(-1, keepdim=True)
    return _pack(raw, scales(hd, prescaled)[0])


def case(kind, Tq, Tk, hd, prescaled=False, b=B, h=H):
    """kind: "random", "diag" (probe_case, shift 0) or "superdiag" (shift 1); with the probe rows ([] for random)."""
    if kind == "random":
        return random_case(Tq, Tk, hd, prescaled, b=b, h=h), []
    shift = KINDS.index(kind) - 1
    return probe_case(Tq, Tk, hd, shift, prescaled, b=b, h=h), probe_rows(Tq, Tk, shift)


def poison_case(Tq, Tk, hd, causal, b=B, h=H, pad=3):
    """Two copies of a `random_case` in a buffer of T = max(Tq, Tk) + pad rows that differ only in what no correct kernel may use: the q rows >= Tq
    and the k / v rows >= Tk are NaN in the first and 1000 in the second, and with causal and Tk > Tq the k / v rows in [Tq, Tk) -- keys after every
    query -- hold other finite values in the second."""
    first = random_case(Tq, Tk, hd, b=b, h=h, T=max(Tq, Tk) + pad).clone()
    second = first.clone()
    for t, fill in ((first, float("nan")), (second, 1000.0)):
        t[:, Tq:, 0] = fill
        t[:, Tk:, 1:] = fill
    if causal and Tk > Tq:
        second[:, Tq:Tk, 1:] = (3.0 * _raw(b, h, Tk - Tq, hd, _seed(Tq, Tk, hd, 5, b))[:, :, 1:]).to(torch.bfloat16)
    return first, second


# ------------------------------------------------------------------------------------------------------------------ the forms
# env: the dispatcher knobs the form needs; offset_out: `out` is a view 8 bytes into its buffer; cases: (Tq, Tk, hd); bh: (batch, heads)
Form = collections.namedtuple("Form", "name rule env offset_out cases bh", defaults=((B, H),))

# the smallest shapes that take each branch of k_attention32's tile schedule (first / in-loop / last tile, half_last) and of k_attention's
TINY = [(1, 1), (16, 64), (4, 16)]                                  # the smallest problem; 4 sub-tiles of keys, Tq < Tk; one sub-tile
ONE_TILE = [(20, 20), (33, 33), (64, 64)]                           # a single half tile; both key blocks; one full tile, masked only because causal
MULTI_TILE = [(65, 65), (130, 130), (230, 230), (256, 256), (70, 200), (200, 70)]
#              second tile = one key (half_last); the in-loop tile runs once; ragged last tile, not half; no ragged tile; Tq < Tk; Tq > Tk
LONG = (600, 600)                                                   # five 128-query workgroups: probe rows 512 and 576 (hd 64 and 56 only)
NO32 = {"OVO_ATTN32": "0"}


def _x(shapes, hds):
    return [(tq, tk, hd) for hd in hds for tq, tk in shapes]


FORMS = [
    Form("tiny", "use32 = !(Tq <= 16 && Tk <= 64); then hd <= 64 && Tk <= 64 && Tq <= 16 && !no_tiny -> k_attention_tiny<64>",
         {}, False, _x(TINY, (8, 40, 64))),
    Form("a32_64q", "use32 && fits32, qpw = (Tq <= 64 && hd <= 64) ? 64 : 128; qpw == 64 -> k_attention32<2,4,2, hd <= 56>",
         {}, False, _x(ONE_TILE, (24, 56, 64))),
    Form("a32_128q", "use32 && fits32, Tq > 64, hd <= 56 -> k_attention32<4,4,2,true>, hd <= 64 -> <4,4,2,false>",
         {}, False, _x(MULTI_TILE + [LONG], (56, 64))),
    Form("a32_wide_hd", "use32 && fits32, hd > 64 (qpw = 128 at any Tq): <= 80 -> <4,5,3,true>, <= 88 -> <4,6,3,true>, <= 96 -> <4,6,3,false>, "
         "<= 120 -> <4,8,4,true>, else <4,8,4,false>", {}, False, _x([(20, 20), (65, 65), (130, 130), (230, 230), (70, 200), (200, 70)], (72, 88, 96, 120, 128))),
    Form("a16_trim", "OVO_ATTN32=0, OVO_ATTN_NO_TINY=1; hd <= 64 && Tk <= 64 && !wide -> k_attention<64,1,true>",
         {**NO32, "OVO_ATTN_NO_TINY": "1"}, False, _x(TINY + ONE_TILE, (40, 64))),
    Form("a16", "OVO_ATTN32=0; not the trimmed form (Tk > 64 or hd > 64): hd <= 64 -> k_attention<64,1>, <= 96 -> <96,1>, else <128,1>",
         NO32, False, _x(MULTI_TILE, (56, 96, 128)) + _x([(20, 20)], (96, 128)) + [LONG + (56,)]),
    Form("a16_wide", "OVO_ATTN32=0, OVO_ATTN_WIDE=1 (wide = kn.wide && !kn.narrow): hd <= 64 -> k_attention<64,2>, > 96 -> <128,2>; 128 queries per workgroup",
         {**NO32, "OVO_ATTN_WIDE": "1"}, False, _x([(20, 20)] + MULTI_TILE, (64, 128)) + [LONG + (64,)]),
    Form("a16_by_alignment", "no knob: fits32 needs ((uintptr_t)o & 15) == 0, the dispatcher only ((uintptr_t)o & 7) == 0 -> k_attention<64,1> "
         "(trimmed at Tk <= 64)", {}, True, _x([(33, 33), (130, 130), (70, 200)], (64,))),
    Form("a16_grid2d", "OVO_ATTN32=0, OVO_ATTN_NO_CHUNK=1, Tq > 64: grid.x > 1 and the grid stays (q-tiles, B H), a.chunk = 0",
         {**NO32, "OVO_ATTN_NO_CHUNK": "1"}, False, _x([(130, 130), (70, 200), (200, 70)], (64,))),
    Form("a16_gridy", "OVO_ATTN32=0, OVO_ATTN_NO_TINY=1, B H = 65539: grid.y > 65535 -> the chunked 1-D grid although grid.x == 1 (25 MB of q | k | v)",
         {**NO32, "OVO_ATTN_NO_TINY": "1"}, False, [(8, 8, 8)], (65539, 1)),
]

# (form, Tq, Tk, hd) of the free-stride check: one per kernel family
FREE_STRIDES = [("tiny", 16, 64, 40), ("a32_64q", 33, 33, 56), ("a32_128q", 70, 200, 64), ("a32_wide_hd", 130, 130, 88), ("a16", 130, 130, 56)]


def form(name):
    return next(f for f in FORMS if f.name == name)


def case_ids(cases):
    return ["%s-%dx%d-hd%d" % ((c[0].name,) + tuple(c[1:])) for c in cases]


CASES = [(f, tq, tk, hd) for f in FORMS for tq, tk, hd in f.cases]
# every distinct probe input of the table: (Tq, Tk, hd, shift, prescaled, b, h)
PROBE_CASES = sorted({(tq, tk, hd, shift, pre) + f.bh for f, tq, tk, hd in CASES for shift in (0, 1) for pre in (False, True) if probe_rows(tq, tk, shift)})
