"""-m gpu: the kernels that maintain the instance map, called through the C ABI and held to exact references written here in numpy.

  1. `ovo_fuse_views` (fusion.hip): mean / l1 medoid / cosine medoid against float64, at descriptor widths below, at and across the 256-thread stride,
     several updates per launch, the first-index tie rule.
  2. `ovo_near_fraction`, `ovo_instance_moments`, `ovo_remap_instances` (loopclose.hip) on a lattice of coordinates k/64, |k| <= 512, th = 5/64:
     every difference, square and three-term sum of k_near_fraction is then exact in f32 (3 * 1024^2 < 2^24, and so is th * th = 25/4096), and the
     reference is integer arithmetic.  No tolerance anywhere in that part.
  3. the mask bit and byte kernels (image.hip, `ovo_paint_segmap` of samdec.hip) at pixel counts that are no multiple of 64, mask bytes other than 0 / 1,
     repeated rows; integer references, bit equality.

The only fixture conditions are the float64 score gap of part 1 and the lattice bounds of part 2; both are asserted from the reference alone.
"""
import numpy as np
import pytest
import torch

from ovo_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
OK, E_ARG = 0, -1                       # OVO_OK, OVO_E_ARG (include/ovo_hip.h)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.cpu().numpy()


# ---- 1. ovo_fuse_views -----------------------------------------------------------------------------------------------------------------------------------

SENTINEL = np.float32(-12345.678)       # fills the table before a launch: a row nobody names has to keep it
GAP = 1e-4                              # best and second-best float64 score differ by more than this, relative: the kernel's f32 tree reduction over at
                                        # most 33 x 1152 terms is some 1e-6 relative, so its winner is then the float64 winner


def _views(seed, V, D):
    """V descriptors of length D whose columns carry different weight (amplitude 2 .. 0.5 across the row): a kernel that drops, repeats or
    double-counts a stretch of columns then ranks the views differently."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((V, D)) * np.linspace(2.0, 0.5, D)).astype(np.float32)


def _scores64(X, mode):
    """score[i] = sum_j dist(x_i, x_j) in float64 -- mode 1: l1 distance, mode 2: cosine similarity with each norm clamped at 1e-8
    (torch.cosine_similarity)."""
    X = X.astype(np.float64)
    if mode == 1:
        return np.abs(X[:, None, :] - X[None, :, :]).sum(-1).sum(1)
    n = np.maximum(np.sqrt((X * X).sum(1)), 1e-8)
    dots = (X[:, None, :] * X[None, :, :]).sum(-1)               # (elementwise, not BLAS: identical rows then give identical bits)
    return (dots / (n[:, None] * n[None, :])).sum(1)


def _medoid64(X, mode, distinct=None):
    """(float64 medoid position: first index of the best score, relative gap between the best score and the best score of any OTHER candidate).
    `distinct` names positions that hold the same row as the winner and are therefore no other candidate."""
    s = _scores64(X, mode)
    s = s if mode == 2 else -s                                   # larger is better
    best = int(np.argmax(s))
    others = np.delete(s, [best] + list(distinct or []))
    second = others.max()
    return best, float((s[best] - second) / max(abs(s[best]), abs(second)))


def _mean_f32(X):
    """The order k_fuse_views documents: sequential f32 sum in view order, then one divide."""
    s = X[0].astype(np.float32).copy()
    for v in range(1, X.shape[0]):
        s = (s + X[v]).astype(np.float32)
    return s if X.shape[0] == 1 else (s / np.float32(X.shape[0])).astype(np.float32)


def _fuse(store, off, rows, mode, n_table, table_rows):
    """One launch of ovo_fuse_views; returns (table [n_table, D], out_view [n_updates]); both were filled with sentinels first."""
    D, n = store.shape[1], len(off) - 1
    table = torch.full((n_table, D), float(SENTINEL), dtype=torch.float32, device=DEV)
    out_view = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    s, o, r, tr = _t(store), _t(np.asarray(off, np.int32)), _t(np.asarray(rows, np.int32)), _t(np.asarray(table_rows, np.int32))
    L.check(L.load().ovo_fuse_views(L.ptr(s), D, L.ptr(o), L.ptr(r), n, mode, L.ptr(table), L.ptr(tr), L.ptr(out_view), L.stream()))
    torch.cuda.synchronize()
    return _np(table), _np(out_view)[:n]


def _check_update(X, mode, row, view):
    """One update's table row and out_view against the float64 references.  X: its views, in CSR order."""
    V = X.shape[0]
    if V == 1:
        assert view == 0 and np.array_equal(row.view(np.uint32), X[0].view(np.uint32))
        return
    if mode == 0:
        assert view == -1
        if V <= 3:
            assert np.array_equal(row.view(np.uint32), _mean_f32(X).view(np.uint32))
        else:
            bound = V * 2.0 ** -23 * float(np.abs(X).max())
            err = float(np.abs(row.astype(np.float64) - X.astype(np.float64).mean(0)).max())
            assert err <= bound, (err, bound)
        return
    if V == 2:
        # Two views have no medoid: score[0] = d(0,0) + d(0,1) and score[1] = d(1,0) + d(1,1) are equal in exact arithmetic, for any data.
        #   l1:     |x - y| = |y - x| and d(i,i) = 0 exactly, summed in the same order: the kernel's two scores are the same bits, and the
        #           first-index rule makes view 0 the answer;
        #   cosine: d(i,i) = p / (sqrt(p) sqrt(p)) is 1 only to an ulp, separately for each view: either view is a correct answer.
        # What is defined either way: the table row is a copy of the view that out_view names.
        assert (view == 0) if mode == 1 else (view in (0, 1))
    else:
        best, gap = _medoid64(X, mode)
        assert gap > GAP, f"fixture: float64 scores too close ({gap:.2e})"
        assert view == best
    assert np.array_equal(row.view(np.uint32), X[view].view(np.uint32))            # a copy, not arithmetic


@pytest.mark.parametrize("V", [1, 2, 3, 7, 33])
@pytest.mark.parametrize("D", [64, 200, 768, 1152])
def test_fuse_views_vs_float64(D, V):
    """One update per launch, every mode: D = 200 is below the 256-thread stride and no multiple of 64, 768 is three strides, 1152 four and a half.
    The views sit at scattered store rows and the table row is not row 0."""
    X = _views(1000 * D + V, V, D)
    rng = np.random.default_rng(V)
    store = rng.standard_normal((V + 5, D)).astype(np.float32)
    rows = rng.permutation(V + 5)[:V]
    store[rows] = X
    for mode in (0, 1, 2):
        table, view = _fuse(store, [0, V], rows, mode, 3, [2])
        _check_update(X, mode, table[2], int(view[0]))
        assert (table[:2].view(np.uint32) == SENTINEL.view(np.uint32)).all()


@pytest.mark.parametrize("D", [200, 768])
def test_fuse_views_seven_updates_one_launch(D):
    """Seven updates of different V in one launch, one of them empty, two of them sharing three store rows, their table rows a permutation into an
    11-row table: every named row against float64, the empty update's row and the four unnamed rows bit-unchanged."""
    Vs = [3, 0, 1, 7, 2, 33, 4]
    table_rows = [9, 2, 5, 0, 7, 3, 10]
    rng = np.random.default_rng(D)
    n_store = sum(Vs) + 9
    store = _views(77 + D, n_store, D)
    perm = rng.permutation(n_store)
    off, rows = [0], []
    for k, V in enumerate(Vs):
        mine, perm = perm[:V], perm[V:]
        if k == 6:
            mine = np.concatenate([rows[:3], mine[:1]])           # update 6 = the three views of update 0 and one of its own
        rows.extend(int(r) for r in mine)
        off.append(len(rows))
    assert set(rows[off[0]:off[1]]) < set(rows[off[6]:off[7]])
    for mode in (0, 1, 2):
        table, view = _fuse(store, off, rows, mode, 11, table_rows)
        for k, V in enumerate(Vs):
            if V == 0:
                continue
            _check_update(store[rows[off[k]:off[k + 1]]], mode, table[table_rows[k]], int(view[k]))
        untouched = sorted(set(range(11)) - set(table_rows)) + [table_rows[1]]
        assert len(untouched) == 5
        assert (table[untouched].view(np.uint32) == SENTINEL.view(np.uint32)).all()


def _contested(seed, V, D, split, mode):
    """Views whose medoid is decided by the balance between the columns below `split` and those from `split` on: the float64 medoid changes when the
    latter are counted twice (l1: doubled; cosine: times sqrt 2).  Random rows rarely are that delicate, so the columns below `split` are scaled by the
    first factor of a fixed grid (and the rows drawn with the first of eight seeds) for which they are -- found and checked with the float64
    reference alone.  Returns (views, the medoid if the columns
    from `split` on counted twice)."""
    twice = np.where(np.arange(D) < split, 1.0, 2.0 if mode == 1 else np.sqrt(2.0))
    for s in range(seed, seed + 8):                              # (rows whose medoid is the same on both sides of `split` have no such balance)
        base = _views(s, V, D)
        for alpha in np.geomspace(1 / 16, 16, 65):
            X = (base * np.where(np.arange(D) < split, alpha, 1.0)).astype(np.float32)
            (best, gap), (other, other_gap) = _medoid64(X, mode), _medoid64(X.astype(np.float64) * twice, mode)
            if best != other and gap > 10 * GAP and other_gap > 10 * GAP:
                return X, other
    raise AssertionError("fixture: no column balance on the grid makes the medoid depend on it")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("D,split", [(768, 128), (768, 512), (1152, 128), (1152, 1024)])
def test_fuse_views_medoid_weighs_every_column_once(D, split, mode):
    """A medoid loop that visits a stretch of columns twice, or with another weight than the rest, still picks A view and copies it faithfully; on rows
    built so that the choice hangs on the balance between the first half-stride (or the last, partial stride) and the rest, it picks the wrong one."""
    X, if_twice = _contested(D + split + mode, 7, D, split, mode)
    best, gap = _medoid64(X, mode)
    assert gap > GAP and best != if_twice
    table, view = _fuse(X, [0, 7], list(range(7)), mode, 1, [0])
    assert int(view[0]) == best
    assert np.array_equal(table[0].view(np.uint32), X[best].view(np.uint32))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("D", [200, 1152])
def test_fuse_views_exact_tie_takes_first_index(D, mode):
    """The same store row at view positions 2 and 5, built as the mean of the other five views so that it is the medoid (checked in float64 against
    the third candidate with the gap rule).  Positions 2 and 5 then have bit-identical scores, and the first index wins."""
    others = _views(5 * D + mode, 5, D)
    centre = others.astype(np.float64).mean(0).astype(np.float32)
    store = np.concatenate([others, centre[None]])
    rows = [0, 1, 5, 2, 3, 5, 4]
    X = store[rows]
    best, gap = _medoid64(X, mode, distinct=[5])
    assert best == 2 and gap > GAP, (best, gap)
    s = _scores64(X, mode)
    assert s[2] == s[5]
    table, view = _fuse(store, [0, 7], rows, mode, 1, [0])
    assert int(view[0]) == 2
    assert np.array_equal(table[0].view(np.uint32), centre.view(np.uint32))


# ---- 2. loop-closure passes on an exact lattice ------------------------------------------------------------------------------------------------------------

KMAX, TH_K = 512, 5                     # coordinates k / 64 with |k| <= KMAX; th = TH_K / 64


def _lattice(k):
    k = np.asarray(k, np.int64).reshape(-1, 3)
    assert np.abs(k).max(initial=0) <= KMAX and 3 * (2 * KMAX) ** 2 < 2 ** 24           # the lattice bounds that make f32 exact
    return k


def _near_ref(A, B, th_k):
    """How many points of A have a point of B at squared lattice distance < th_k^2: integers."""
    hit = np.zeros(len(A), bool)
    for c in range(0, len(B), 512):
        d = A[:, None, :] - B[None, c:c + 512, :]
        hit |= ((d * d).sum(-1) < th_k * th_k).any(1)
    return int(hit.sum())


def _near_scene():
    """(slots: list of int lattice point sets, pairs [(a, b)], names of the special pairs -> pair index)."""
    rng = np.random.default_rng(5)
    slots, pairs, special = [], [], {}

    def add(k):
        slots.append(_lattice(k))
        return len(slots) - 1

    # |a| x |b| across the 256-point block and chunk boundaries.  a: half its points in a small box, half in a wide one; b: a box whose volume grows
    # with |b|, so that every pair has points with and without a close neighbour wherever its sizes allow
    a_slots = {na: add(np.where(rng.random((na, 1)) < 0.5, rng.integers(-8, 9, (na, 3)), rng.integers(-40, 41, (na, 3)))) for na in (1, 255, 256, 257, 1000)}
    b_slots = {}
    for nb in (1, 255, 256, 257, 513, 3000):
        h = max(4, int(round((nb * 743.0) ** (1 / 3) / 2)))
        b_slots[nb] = add(rng.integers(-h, h + 1, (nb, 3)))
    for na, sa in a_slots.items():
        for nb, sb in b_slots.items():
            pairs.append((sa, sb))
    special["small_a"] = pairs.index((a_slots[1], b_slots[3000]))                         # |a| = 1 in a launch shaped for max_points_a = 1000
    empty = add(np.zeros((0, 3)))
    special["empty_b"] = len(pairs)
    pairs.append((a_slots[257], empty))
    special["self"] = len(pairs)
    pairs.append((a_slots[1000], a_slots[1000]))
    # every point of a has its only close neighbour in the LAST 256-chunk of b: 150 centres 12 apart, two points of a at each (+-1 in x), one point
    # of b two steps off in y; b = 768 far points, those 150, 50 more far points
    c = np.stack([12 * (np.arange(150) % 20) - 200, 12 * (np.arange(150) // 20) - 200, np.zeros(150, np.int64)], 1)
    a_last = add(np.concatenate([c + [1, 0, 0], c - [1, 0, 0]]))
    far = np.stack([rng.integers(300, KMAX + 1, 818), rng.integers(-KMAX, KMAX + 1, 818), rng.integers(-KMAX, KMAX + 1, 818)], 1)
    b_last = add(np.concatenate([far[:768], c + [0, 2, 0], far[768:]]))
    special["last_chunk"] = len(pairs)
    pairs.append((a_last, b_last))
    # 260 points of a 12 apart, each with ONE point of b nearby: the first 130 at (3, 4, 0) -- distance exactly th -- the other 130 at (3, 3, 0)
    g = np.stack([12 * (np.arange(260) % 20) - 120, 12 * (np.arange(260) // 20) - 120, np.full(260, 7)], 1)
    a_edge = add(g)
    b_edge = add(g + np.where(np.arange(260)[:, None] < 130, [[3, 4, 0]], [[3, 3, 0]]))
    special["edge"] = len(pairs)
    pairs.append((a_edge, b_edge))
    return slots, pairs, special


def _near_call(pts, off, pairs, n_pairs, max_a, th, near):
    return L.load().ovo_near_fraction(L.ptr(pts), L.ptr(off), L.ptr(pairs), n_pairs, max_a, th, L.ptr(near), L.stream())


def test_near_fraction_exact_counts():
    slots, pairs, special = _near_scene()
    off = np.concatenate([[0], np.cumsum([len(s) for s in slots])]).astype(np.int64)
    pts = _t((np.concatenate(slots) / 64.0).astype(np.float32))
    assert np.array_equal(_np(pts).astype(np.float64) * 64, np.concatenate(slots))           # k / 64 is exact in f32
    d_off, d_pairs = _t(off), _t(np.asarray(pairs, np.int32))
    n_pairs, max_a = len(pairs), max(len(slots[a]) for a, _ in pairs)
    assert n_pairs >= 34 and max_a == 1000 and np.float32(TH_K / 64.0) ** 2 == np.float32(TH_K * TH_K / 4096.0)
    want = np.array([_near_ref(slots[a], slots[b], TH_K) for a, b in pairs], np.int32)
    # the fixture says what it set out to say (from the reference alone)
    assert want[special["empty_b"]] == 0 and want[special["self"]] == 1000 and want[special["last_chunk"]] == 300 and want[special["edge"]] == 130
    assert len(slots[pairs[special["small_a"]][0]]) == 1
    assert ((want > 0) & (want < [len(slots[a]) for a, _ in pairs])).sum() >= 12             # counts that are neither nothing nor everything

    near = torch.full((n_pairs,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    L.check(_near_call(pts, d_off, d_pairs, n_pairs, max_a, TH_K / 64.0, near))
    torch.cuda.synchronize()
    got = _np(near)
    assert np.array_equal(got, want), [(i, pairs[i], int(got[i]), int(want[i])) for i in np.flatnonzero(got != want)]
    # the second half of the edge pair, nothing of the first: the comparison is strict
    edge_a, edge_b = slots[pairs[special["edge"]][0]], slots[pairs[special["edge"]][1]]
    assert _near_ref(edge_a[:130], edge_b, TH_K) == 0 and _near_ref(edge_a[130:], edge_b, TH_K) == 130

    # th = 0: nothing is closer than nothing, a point to itself included
    near.fill_(0x5a5a5a5a)
    L.check(_near_call(pts, d_off, d_pairs, n_pairs, max_a, 0.0, near))
    torch.cuda.synchronize()
    assert not _np(near).any()

    # no pair: OVO_OK and nothing written;  no point of a: OVO_OK and the counts zeroed
    near.fill_(0x5a5a5a5a)
    assert _near_call(pts, d_off, d_pairs, 0, max_a, TH_K / 64.0, near) == OK
    torch.cuda.synchronize()
    assert (_np(near) == 0x5a5a5a5a).all()
    assert _near_call(pts, d_off, d_pairs, n_pairs, 0, TH_K / 64.0, near) == OK
    torch.cuda.synchronize()
    assert not _np(near).any()


N_SLOTS = 7
ID_POOL = np.array([-1, 0, 1, 2, 3, 5, 6, 7, 1000, -5], np.int32)        # slot 4 never appears; 7 = n_slots, 1000 and the negatives are outside


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100003])
def test_instance_moments_exact(n):
    rng = np.random.default_rng(n)
    k = _lattice(rng.integers(-KMAX, KMAX + 1, (n, 3)))
    ids = rng.choice(ID_POOL, n)
    if n:
        ids[0] = 2                                                       # at least one point that counts
    sums = torch.full((N_SLOTS, 3), -1.5e300, dtype=torch.float64, device=DEV)
    cnt = torch.full((N_SLOTS,), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    xyz, ins = _t((k / 64.0).astype(np.float32)), _t(ids)
    L.check(L.load().ovo_instance_moments(L.ptr(xyz), L.ptr(ins), n, N_SLOTS, L.ptr(sums), L.ptr(cnt), L.stream()))
    torch.cuda.synchronize()
    want_cnt, want_sum = np.zeros(N_SLOTS, np.int32), np.zeros((N_SLOTS, 3), np.int64)
    for s in range(N_SLOTS):
        want_cnt[s] = (ids == s).sum()
        want_sum[s] = k[ids == s].sum(0)
    assert want_cnt[4] == 0 and (n < 255 or (ids == 7).any() and (ids == 1000).any() and (ids < 0).any())
    assert np.array_equal(_np(cnt), want_cnt)
    assert np.array_equal(_np(sums), want_sum / 64.0)                    # sums of lattice values are exact in f64 in any order


@pytest.mark.parametrize("n", [0, 1, 257, 100003])
def test_remap_instances_one_pass_in_place(n):
    """table[1] = 2 and table[2] = 5: an id of 1 becomes 2, not 5.  Ids outside [0, n_slots) stay as they are."""
    table = np.array([0, 2, 5, 3, 6, 5, 0], np.int32)
    pool = np.array([-1, 0, 1, 2, 3, 4, 5, 6, N_SLOTS, N_SLOTS + 3], np.int32)
    rng = np.random.default_rng(n + 1)
    ids = rng.choice(pool, n)
    if n:
        ids[0] = 1
    want = np.where((ids >= 0) & (ids < N_SLOTS), table[np.clip(ids, 0, N_SLOTS - 1)], ids)
    assert n == 0 or want[0] == 2
    ins, tab = _t(ids), _t(table)
    L.check(L.load().ovo_remap_instances(L.ptr(ins), n, L.ptr(tab), N_SLOTS, L.stream()))
    torch.cuda.synchronize()
    assert np.array_equal(_np(ins), want)
    if n > 1000:
        assert all((ids == v).any() and (want[ids == v] == v).all() for v in (-1, N_SLOTS, N_SLOTS + 3))


# ---- 3. mask bit and byte kernels at ragged sizes ----------------------------------------------------------------------------------------------------------

MASK_BYTES = np.array([0, 1, 2, 255], np.uint8)                          # non-zero means set


def _masks(seed, n, pixels, values=MASK_BYTES, p_zero=0.5):
    rng = np.random.default_rng(seed)
    p = np.full(len(values), (1 - p_zero) / (len(values) - 1))
    p[0] = p_zero
    return rng.choice(values, (n, pixels), p=p)


def _pack_ref(m, words):
    """bit p of row i = (m[i, p] != 0), little-endian inside u64 words, zero beyond the last pixel."""
    b = np.zeros((m.shape[0], words * 64), np.uint8)
    b[:, :m.shape[1]] = m != 0
    return np.packbits(b, axis=1, bitorder="little").view("<u8")


def _pack(m, words):
    n, pixels = m.shape
    bits = torch.full((n, words), -1, dtype=torch.int64, device=DEV)                         # all ones: tail bits and spare words must be WRITTEN zero
    d = _t(m)
    L.check(L.load().ovo_pack_masks(L.ptr(d), n, pixels, L.ptr(bits), words, L.stream()))
    torch.cuda.synchronize()
    return bits


def _unpack(bits, n, pixels, words):
    out = torch.full((n, pixels), 0xAA, dtype=torch.uint8, device=DEV)
    L.check(L.load().ovo_unpack_masks(L.ptr(bits), n, pixels, words, L.ptr(out), L.stream()))
    torch.cuda.synchronize()
    return _np(out)


@pytest.mark.parametrize("pixels", [16, 48, 100, 1000, 4112])
def test_pack_masks_ragged(pixels):
    for n in (1, 3):
        for spare in (0, 1):
            words = (pixels + 63) // 64 + spare
            m = _masks(pixels + n, n, pixels)
            got = _np(_pack(m, words)).view(np.uint64)
            assert np.array_equal(got, _pack_ref(m, words)), (n, words)


@pytest.mark.parametrize("pixels", [16, 48, 1040, 4112])
def test_unpack_masks_ragged(pixels):
    """Bits packed by numpy and bits packed by ovo_pack_masks both unpack to (m != 0), one byte 0 / 1 per pixel."""
    for n in (1, 3):
        for spare in (0, 1):
            words = (pixels + 63) // 64 + spare
            m = _masks(7 * pixels + n, n, pixels)
            want = (m != 0).astype(np.uint8)
            ref_bits = _pack_ref(m, words)
            if spare:
                ref_bits[:, -1] = np.uint64(0xFFFFFFFFFFFFFFFF)                                 # a spare word is not the masks' business
            for bits in (_t(ref_bits.view(np.int64)), _pack(m, words)):
                got = _unpack(bits, n, pixels, words)
                assert np.array_equal(got, want), (n, words)


@pytest.mark.parametrize("words", [1, 63, 65])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_mask_intersections_popcount(n, words):
    rng = np.random.default_rng(100 * n + words)
    bits = rng.integers(0, 2 ** 64, (n, words), dtype=np.uint64)
    bits[0] &= rng.integers(0, 2 ** 64, words, dtype=np.uint64)          # a sparser row
    if n > 2:
        bits[2] = 0                                                      # an empty mask
    if n > 3:
        bits[3] = np.uint64(0xFFFFFFFFFFFFFFFF)                          # a full one
    b = np.unpackbits(bits.view(np.uint8), axis=1).astype(np.int64)
    want = (b @ b.T).astype(np.int32)                                    # popcount(a & b)
    inter = torch.full((n, n), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    d = _t(bits.view(np.int64))
    L.check(L.load().ovo_mask_intersections(L.ptr(d), n, words, L.ptr(inter), L.stream()))
    torch.cuda.synchronize()
    got = _np(inter)
    assert np.array_equal(got, want)
    assert np.array_equal(got, got.T) and np.array_equal(np.diag(got), b.sum(1))


def _mask_or(d, pixels, pairs):
    p = _t(np.asarray(pairs, np.int32))
    rc = L.load().ovo_mask_or(L.ptr(d), pixels, L.ptr(p), len(pairs), L.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("pixels", [16, 4112])
def test_mask_or_bytes(pixels):
    m = _masks(pixels, 6, pixels)
    m[0, 0], m[3, 0], m[4, 0] = 2, 1, 0                                  # 2 | 1 == 3: bytes are OR-ed as bytes
    for pairs in ([(0, 3), (0, 4), (2, 5)], [(1, 4)]):                   # a dst named twice with two sources; one pair
        want = m.copy()
        for dst, src in pairs:
            want[dst] |= m[src]
        d = _t(m)
        assert _mask_or(d, pixels, pairs) == OK
        got = _np(d)
        assert np.array_equal(got, want)
        assert got[0, 0] == (3 if len(pairs) > 1 else 2)
        named = {dst for dst, _ in pairs}
        assert all(np.array_equal(got[r], m[r]) for r in range(6) if r not in named)


def test_mask_or_rejects_ragged_pixels():
    m = _masks(3, 4, 24)
    d = _t(m)
    assert _mask_or(d, 24, [(0, 1)]) == E_ARG
    assert np.array_equal(_np(d), m)                                     # nothing launched


@pytest.mark.parametrize("pixels", [1, 777, 4112])
def test_mask_area_any_pixel_count(pixels):
    m = _masks(pixels, 5, pixels)
    m[3] = 0
    m[0, 0] = 255
    rows = np.array([4, 0, 3, 0, 2], np.int32)
    area = torch.full((len(rows),), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    d, r = _t(m), _t(rows)
    L.check(L.load().ovo_mask_area(L.ptr(d), pixels, L.ptr(r), len(rows), L.ptr(area), L.stream()))
    torch.cuda.synchronize()
    want = (m[rows] != 0).sum(1).astype(np.int32)
    assert want[2] == 0 and want[1] == want[3] > 0
    assert np.array_equal(_np(area), want)


def _gather(src, row_bytes, idx, dst):
    i = _t(np.asarray(idx, np.int32))
    rc = L.load().ovo_gather_rows(L.ptr(src), row_bytes, L.ptr(i), len(idx), L.ptr(dst), L.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("row_bytes", [16, 48, 4112])
def test_gather_rows_repeats_unsorted(row_bytes):
    src = np.random.default_rng(row_bytes).integers(0, 256, (7, row_bytes), dtype=np.uint8)
    idx = [5, 0, 5, 2, 6, 0]
    dst = torch.full((len(idx), row_bytes), 0xAA, dtype=torch.uint8, device=DEV)
    assert _gather(_t(src), row_bytes, idx, dst) == OK
    assert np.array_equal(_np(dst), src[idx])


def test_gather_rows_rejects_ragged_rows():
    src = np.random.default_rng(24).integers(0, 256, (7, 24), dtype=np.uint8)
    dst = torch.full((2, 24), 0xAA, dtype=torch.uint8, device=DEV)
    assert _gather(_t(src), 24, [1, 0], dst) == E_ARG
    assert (_np(dst) == 0xAA).all()                                      # nothing launched


@pytest.mark.parametrize("pixels", [16, 1000])
@pytest.mark.parametrize("n", [1, 5])
def test_paint_segmap_first_mask_wins(n, pixels):
    m = _masks(31 * n + pixels, n, pixels, values=np.array([0, 1, 255], np.uint8), p_zero=0.6)
    m[:, 0] = 0                                                          # a pixel nobody covers
    m[:, 1] = 255                                                        # a pixel everybody covers
    want = np.where((m != 0).any(0), (m != 0).argmax(0), -1).astype(np.int32)
    assert want[0] == -1 and want[1] == 0 and (n == 1 or ((m != 0).sum(0) > 1).any() and want.max() == n - 1)
    seg = torch.full((pixels,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    d = _t(m)
    L.check(L.load().ovo_paint_segmap(L.ptr(d), n, pixels, L.ptr(seg), L.stream()))
    torch.cuda.synchronize()
    assert np.array_equal(_np(seg), want)
