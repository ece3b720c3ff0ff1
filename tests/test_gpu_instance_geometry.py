"""-m gpu: `ovo_instance_geometry` (csrc/insgeo.hip; include/ovo_hip.h has the contract) against numpy.  `cnt`, `lo`, `hi` are compared as raw bits
everywhere; `sums` / `prods` for equality where every partial sum is exact in f64 in any order (a lattice of coordinates k/64, |k| <= 512: the
reference is integer arithmetic), and within the header's bound (n_slot - 1) * 2^-53 * sum |term| on random f32 data.

1. the lattice case: 20 011 rows, 37 slots, ids from [-1, 40): an empty slot, a slot with one row, a slot with 60 % of the rows; the first half sorted
   by id (long runs), the second half shuffled; cnt and sums also equal `ovo_instance_moments`';
2. tails n = 0, 1, 63, 64, 65, 257; one slot; 5000 slots (the path beside the LDS window); 300 001 rows with OVO_INSGEO_GRID_CAP = 8;
3. non-finite rows, signed zeros, every output alone, random data, per-slot axes against the exact chain, a repeated launch."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import render_restatement as RR
from ovo_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = ("cnt", "lo", "hi", "sums", "prods")
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
INF_BITS, NINF_BITS = np.uint32(0x7F800000), np.uint32(0xFF800000)


def _gpu(xyz, ins, n_slots, want=ALL, axes=None):
    """One call on arrays of garbage: whatever is asked for comes back as numpy (lo / hi as f32), the rest is NULL."""
    n = len(ins)
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)).to(DEV)
    d_ins = torch.from_numpy(np.ascontiguousarray(ins, np.int32)).to(DEV)
    d_axes = None if axes is None else torch.from_numpy(np.ascontiguousarray(axes, np.float32)).to(DEV)
    bufs = {"cnt": torch.full((n_slots,), 0x7f7f7f7f, dtype=torch.int32, device=DEV),
            "lo": torch.full((n_slots, 3), -7.5, dtype=torch.float32, device=DEV), "hi": torch.full((n_slots, 3), 7.5, dtype=torch.float32, device=DEV),
            "sums": torch.full((n_slots, 3), -1.5e300, dtype=torch.float64, device=DEV),
            "prods": torch.full((n_slots, 6), 2.5e300, dtype=torch.float64, device=DEV)}
    p = {k: L.ptr(bufs[k] if k in want else None) for k in ALL}
    L.check(L.load().ovo_instance_geometry(L.ptr(d_xyz), L.ptr(d_ins), n, n_slots, L.ptr(d_axes), p["cnt"], p["lo"], p["hi"], p["sums"], p["prods"],
                                           L.stream()))
    torch.cuda.synchronize()
    return {k: bufs[k].cpu().numpy() for k in want}, {k: bufs[k].cpu().numpy() for k in ALL if k not in want}


def _ordered(f32):
    b = np.ascontiguousarray(f32, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b ^ np.uint32(0x80000000))


def _unordered(o):
    return np.where(o >> 31 != 0, o ^ np.uint32(0x80000000), ~o).astype(np.uint32)


def _contributes(xyz, ins, n_slots):
    return (ins >= 0) & (ins < n_slots) & np.isfinite(xyz).all(1)


def _ref_box(values, ins, ok, n_slots):
    """(cnt i32, lo bits u32[n_slots,3], hi bits) in the total order of the sign-flipped image."""
    o, ids = _ordered(values)[ok], ins[ok]
    cnt = np.bincount(ids, minlength=n_slots).astype(np.int32)
    lo, hi = np.full((n_slots, 3), 0xFFFFFFFF, np.uint32), np.zeros((n_slots, 3), np.uint32)
    np.minimum.at(lo, ids, o)
    np.maximum.at(hi, ids, o)
    empty = (cnt == 0)[:, None]
    return cnt, np.where(empty, INF_BITS, _unordered(lo)), np.where(empty, NINF_BITS, _unordered(hi))


def _assert_box(got, xyz, ins, n_slots, values=None):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    ok = _contributes(xyz, ins, n_slots)
    cnt, lo, hi = _ref_box(xyz if values is None else values, ins, ok, n_slots)
    if "cnt" in got:
        assert np.array_equal(got["cnt"], cnt)
    if "lo" in got:
        assert np.array_equal(got["lo"].view(np.uint32), lo)
    if "hi" in got:
        assert np.array_equal(got["hi"].view(np.uint32), hi)
    return cnt


def _lattice(n, n_slots, seed, id_hi=None):
    """k i64[n,3] in [-512, 512] and ids in [-1, id_hi): the integer scene; xyz = k / 64 is exact in f32."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-512, 513, (n, 3))
    ins = rng.integers(-1, (n_slots + 3) if id_hi is None else id_hi, n).astype(np.int32)
    return k, ins


def _assert_lattice(got, k, ins, n_slots):
    xyz = (k / 64.0).astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64) * 64, k)
    _assert_box(got, xyz, ins, n_slots)
    ok = (ins >= 0) & (ins < n_slots)
    sums, prods = np.zeros((n_slots, 3), np.int64), np.zeros((n_slots, 6), np.int64)
    np.add.at(sums, ins[ok], k[ok])
    np.add.at(prods, ins[ok], np.stack([k[ok, i] * k[ok, j] for i, j in PAIRS], 1))
    if "sums" in got:
        assert np.array_equal(got["sums"], sums / 64.0)
    if "prods" in got:
        assert np.array_equal(got["prods"], prods / 4096.0)


# ---------------------------------------------------------------------------------------------------- 1. the lattice case
def _lattice_case():
    n, n_slots = 20_011, 37
    k, ins = _lattice(n, n_slots, 1, id_hi=40)
    rng = np.random.default_rng(2)
    ins[ins == 5] = 6                                               # slot 5 stays empty
    ins[ins == 9] = 10
    ins[rng.random(n) < 0.6] = 3                                    # a wall: 60 % of the rows in one slot
    ins[: n // 2].sort()                                            # first half: long runs; second half: shuffled
    ins[n // 2 + 17] = 9                                            # slot 9 holds one row
    return k, ins, n_slots


def test_lattice_case_is_exact():
    k, ins, n_slots = _lattice_case()
    n = len(ins)
    cnt = np.bincount(ins[(ins >= 0) & (ins < n_slots)], minlength=n_slots)
    assert cnt[5] == 0 and cnt[9] == 1 and 0.58 * n < cnt[3] < 0.65 * n and (ins == -1).any() and (ins >= n_slots).any()      # the fixture says what it set out to
    assert (np.diff(ins[: n // 2]) >= 0).all() and (np.diff(ins[n // 2:]) < 0).any() and n * 2 ** 18 < 2 ** 53
    got, _ = _gpu(k / 64.0, ins, n_slots)
    _assert_lattice(got, k, ins, n_slots)
    assert (got["lo"][5] == np.inf).all() and (got["hi"][5] == -np.inf).all() and np.array_equal(got["lo"][9], got["hi"][9])
    # the per-point-atomic pass gives the same counts and sums
    xyz, d_ins = torch.from_numpy((k / 64.0).astype(np.float32)).to(DEV), torch.from_numpy(ins).to(DEV)
    sums = torch.empty((n_slots, 3), dtype=torch.float64, device=DEV)
    cnt_m = torch.empty(n_slots, dtype=torch.int32, device=DEV)
    L.check(L.load().ovo_instance_moments(L.ptr(xyz), L.ptr(d_ins), n, n_slots, L.ptr(sums), L.ptr(cnt_m), L.stream()))
    assert np.array_equal(cnt_m.cpu().numpy(), got["cnt"]) and np.array_equal(sums.cpu().numpy(), got["sums"])


# ---------------------------------------------------------------------------------------------------- 2. tails and windows
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_tails(n):
    k, ins = _lattice(n, 37, 100 + n)
    if n:
        ins[0] = 2
    got, _ = _gpu(k / 64.0, ins, 37)
    _assert_lattice(got, k, ins, 37)
    assert int(got["cnt"].sum()) == int(((ins >= 0) & (ins < 37)).sum()) and (n == 0 or got["cnt"][2] >= 1)


def test_one_slot():
    k, ins = _lattice(1000, 1, 7)                                   # ids from [-1, 4): slot 0 and three kinds of rows outside
    got, _ = _gpu(k / 64.0, ins, 1)
    _assert_lattice(got, k, ins, 1)
    assert 100 < got["cnt"][0] < 400


def test_slots_beside_the_window():
    n, n_slots = 20_011, 5000
    k, ins = _lattice(n, n_slots, 8)
    ins[: n // 2].sort()
    got, _ = _gpu(k / 64.0, ins, n_slots)
    _assert_lattice(got, k, ins, n_slots)
    assert (got["cnt"][1024:] > 0).sum() > 3500 and (got["cnt"][:1024] > 0).sum() > 900      # both sides of the 1024-slot LDS window are busy


def test_every_workgroup_loops(monkeypatch):
    n, n_slots = 300_001, 37
    k, ins = _lattice(n, n_slots, 9)
    ins[np.random.default_rng(10).random(n) < 0.6] = 3
    ins[: n // 2].sort()
    assert n * 2 ** 18 < 2 ** 53
    default, _ = _gpu(k / 64.0, ins, n_slots)
    _assert_lattice(default, k, ins, n_slots)                       # 74 workgroups of 4096 rows, one trip each and a ragged last one
    monkeypatch.setenv("OVO_KNOBS_DYNAMIC", "1")
    monkeypatch.setenv("OVO_INSGEO_GRID_CAP", "8")                  # 8 workgroups x 4096 rows per trip: 10 trips
    capped, _ = _gpu(k / 64.0, ins, n_slots)
    _assert_lattice(capped, k, ins, n_slots)


# ---------------------------------------------------------------------------------------------------- 3. the other cases
def test_non_finite_rows_are_skipped():
    k, ins = _lattice(3000, 37, 11)
    xyz = (k / 64.0).astype(np.float32)
    rng = np.random.default_rng(12)
    bad = rng.choice(3000, 300, replace=False)
    xyz[bad, rng.integers(0, 3, 300)] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), 300)
    got, _ = _gpu(xyz, ins, 37)
    cnt = _assert_box(got, xyz, ins, 37)
    ok = _contributes(xyz, ins, 37)
    assert cnt.sum() == ok.sum() < ((ins >= 0) & (ins < 37)).sum() and np.isfinite(got["sums"]).all() and np.isfinite(got["prods"]).all()
    kk, ii = k[ok], ins[ok]
    _assert_lattice({"sums": got["sums"], "prods": got["prods"]}, kk, ii, 37)              # the skipped rows are in no sum either
    assert np.isfinite(got["lo"][cnt > 0]).all() and np.isfinite(got["hi"][cnt > 0]).all()


def test_signed_zeros_are_ordered():
    xyz = np.array([[0.0, -0.0, 0.0], [-0.0, 0.0, 0.0], [0.0, 0.0, -0.0], [-0.0, -0.0, -0.0]], np.float32)
    got, _ = _gpu(xyz, np.array([1, 1, 1, 0], np.int32), 2)
    assert np.array_equal(got["lo"].view(np.uint32)[1], [0x80000000] * 3) and np.array_equal(got["hi"].view(np.uint32)[1], [0, 0, 0])
    assert np.array_equal(got["lo"].view(np.uint32)[0], [0x80000000] * 3) and np.array_equal(got["hi"].view(np.uint32)[0], [0x80000000] * 3)
    _assert_box(got, xyz, np.array([1, 1, 1, 0], np.int32), 2)


@pytest.mark.parametrize("want", [("cnt",), ("lo",), ("hi",), ("sums",), ("prods",), ("lo", "hi"), ("cnt", "sums"), ()])
def test_every_output_is_optional(want):
    k, ins, n_slots = _lattice_case()
    got, untouched = _gpu(k[:5000] / 64.0, ins[7000:12000], n_slots, want=want)
    _assert_lattice(got, k[:5000], ins[7000:12000], n_slots)
    fill = {"cnt": 0x7f7f7f7f, "lo": -7.5, "hi": 7.5, "sums": -1.5e300, "prods": 2.5e300}
    for name, arr in untouched.items():                             # (they were never passed: a guard that the helper passes what it says)
        assert (arr == fill[name]).all()


def test_random_data_within_the_bound():
    n, n_slots = 50_000, 37
    rng = np.random.default_rng(13)
    xyz = (rng.standard_normal((n, 3)) * np.array([4.0, 0.5, 30.0]) + np.array([2.0, -1.0, 100.0])).astype(np.float32)
    ins = rng.integers(-1, 40, n).astype(np.int32)
    ins[ins == 9] = 10
    ins[rng.random(n) < 0.6] = 3
    ins[: n // 2].sort()
    ins[n // 2 + 5] = 9
    got, _ = _gpu(xyz, ins, n_slots)
    cnt = _assert_box(got, xyz, ins, n_slots)
    assert cnt[9] == 1 and cnt[3] > 0.55 * n
    x = xyz.astype(np.float64)
    terms = np.concatenate([x, np.stack([x[:, i] * x[:, j] for i, j in PAIRS], 1)], 1)     # exact in f64: 24 + 24 bits
    have = np.concatenate([got["sums"], got["prods"]], 1)
    worst = 0.0
    for s in range(n_slots):
        t = terms[ins == s]
        ref, bound = t.sum(0), (max(len(t), 1) - 1) * 2.0 ** -53 * np.abs(t).sum(0)
        err = np.abs(have[s] - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if len(t) > 1 else 0.0)
        assert (err <= bound).all(), (s, len(t), err, bound)
    print(f"largest error / bound over all slots and quantities: {worst:.3e}")


def _chain3(a, x, y, z):
    """dot3 of csrc/projection.h: fl(fl(fl(a0 x) + a1 y) + a2 z), every fl one rounding of the exact value."""
    c = RR.round_f32(Fraction(float(a[0])) * Fraction(float(x)))
    c = RR.round_f32(Fraction(float(a[1])) * Fraction(float(y)) + Fraction(float(c)))
    return RR.round_f32(Fraction(float(a[2])) * Fraction(float(z)) + Fraction(float(c)))


def test_extent_along_per_slot_axes():
    n, n_slots = 2000, 3
    rng = np.random.default_rng(14)
    xyz = (rng.standard_normal((n, 3)) * 2.0 + np.array([1.0, -2.0, 3.0])).astype(np.float32)
    ins = rng.integers(-1, 4, n).astype(np.int32)
    axes = np.stack([(RR.rot(0, a) @ RR.rot(1, b) @ RR.rot(2, c))[:3, :3] for a, b, c in ((0.3, -0.2, 0.9), (1.2, 0.4, -0.7), (-0.5, 2.0, 0.1))]).astype(np.float32)
    along = np.zeros((n, 3), np.float32)
    for i in np.nonzero((ins >= 0) & (ins < n_slots))[0]:
        along[i] = [_chain3(axes[ins[i], k], *xyz[i]) for k in range(3)]
    plain = np.einsum("nkj,nj->nk", axes[np.clip(ins, 0, 2)], xyz)
    assert (along.view(np.uint32) != plain.astype(np.float32).view(np.uint32)).any()        # the chain is not numpy's f32 arithmetic
    got, _ = _gpu(xyz, ins, n_slots, axes=axes)
    _assert_box(got, xyz, ins, n_slots, values=along)
    raw, _ = _gpu(xyz, ins, n_slots)
    assert np.array_equal(got["cnt"], raw["cnt"]) and not np.array_equal(got["lo"], raw["lo"])
    x = xyz.astype(np.float64)
    for s in range(n_slots):                                        # the moments do not see the axes
        assert np.abs(got["sums"][s] - x[ins == s].sum(0)).max() < 1e-9


def test_repeated_launch_is_bit_identical():
    k, ins, n_slots = _lattice_case()
    rng = np.random.default_rng(15)
    xyz = (k / 64.0 + rng.standard_normal(k.shape) * 1e-3).astype(np.float32)
    a, _ = _gpu(xyz, ins, n_slots)
    b, _ = _gpu(xyz, ins, n_slots)
    for name in ("cnt", "lo", "hi"):
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name
    _assert_box(a, xyz, ins, n_slots)
