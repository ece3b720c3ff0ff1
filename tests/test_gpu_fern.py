"""ovo_fern_encode and ovo_fern_search on the GPU, BIT FOR BIT against tests/fern_restatement.py: a code from the GPU's own pyramid
read back, the distances, and every word of the pinned result block -- with guard bytes around whatever a call writes, under OVO_FERN_GRID_CAP=2 and from
run to run.  Refused calls launch nothing and write nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fern_restatement as FR  # noqa: E402
import icp_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 0x5A5A5A5A
SEQ = 91
_cache = {}


def _libs():
    from ovo_amd import _lib as L
    from ovo_amd.utils import fern_utils as F
    from ovo_amd.utils import icp_utils as U
    return L, L.load(), F, U


# ------------------------------------------------------------------------------------------------ 1. encode
def _depth(h, w, seed):
    """Depths in 0.3 .. 6 m with every kind of invalid value sprinkled in: 0, NaN, +inf, negative, and values above max_depth = 4."""
    g = np.random.default_rng(seed)
    d = g.uniform(0.3, 6.0, size=(h, w)).astype(np.float32)
    for value in (0.0, np.nan, np.inf, -1.0):
        d[g.random((h, w)) < 0.04] = value
    return d


K_SMALL = np.array([[20.0, 0, 17.5], [0, 20.0, 11.5], [0, 0, 1]], np.float32)
# (h, w, levels, level, M): the smallest level a pyramid can have (3 x 4: ovo_icp_prepare takes no coarsest level under 3 x 3, so the 2 x 3 level of
# the issue's list cannot be made) with the smallest M; an odd W; the largest M; levels other than the coarsest
ENCODE_CASES = [(6, 8, 2, None, 8), (24, 36, 3, None, 40), (24, 36, 3, None, 4096), (24, 36, 3, 0, 256), (24, 36, 3, 1, 40), (25, 37, 2, 1, 264)]


@pytest.mark.parametrize("h,w,levels,level,M", ENCODE_CASES)
def test_encode(h, w, levels, level, M):
    L, lib, F, U = _libs()
    depth = _depth(h, w, h * w + M)
    frame = U.prepare_frame(torch.from_numpy(depth).to(DEV), K_SMALL, levels, 4.0, 0.1)
    lv = levels - 1 if level is None else level
    hl, wl = h >> lv, w >> lv
    pix, tau = FR.draw(M, (hl, wl), 5, (0.2, 4.5))
    table = F.FernTable(M, (hl, wl), seed=5, tau_range=(0.2, 4.5), device=DEV)
    assert np.array_equal(table.pix, pix) and np.array_equal(table.tau.view(np.int32), tau.view(np.int32))      # the shipped draw IS the restated one
    Wn = M // 8
    buf = torch.full((Wn + 8,), GUARD, dtype=torch.int32, device=DEV)      # 4 guard words on either side
    pyramid_before = frame.pyramid.clone()
    out = F.encode(frame, table, level=level, out=buf[4:4 + Wn])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() + 16
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[:4] == GUARD).all() and (got[4 + Wn:] == GUARD).all() and torch.equal(frame.pyramid, pyramid_before)
    px = frame.level(lv).cpu().numpy()
    z, flag = px[..., 2], (px[..., 3].view(np.int32) & 1) != 0
    want = FR.bits_of(z, flag, pix, tau)
    assert np.array_equal(got[4:4 + Wn], FR.pack(want))
    assert np.array_equal(FR.unpack(got[4:4 + Wn], M), want)
    # and from the restated pyramid: the same code (the level's depths are f32 in both)
    assert np.array_equal(want, FR.encode(R.prepare(depth, K_SMALL, levels, 4.0, 0.1, np.float32), pix, tau, level))
    ones = int(want.sum())
    print(f"{h}x{w} level {lv} M={M}: {ones} of {4 * M} tests set, {int((~flag).sum())} of {flag.size} pixels invalid")
    assert 0 < ones < 4 * M and ((~flag).any() or lv == levels - 1)      # (2 x 2 means fill the holes of a coarsest level)
    again = F.encode(frame, table, level=level)
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy().view(np.uint32), got[4:4 + Wn])


# ------------------------------------------------------------------------------------------------ 2. search
def _database(n, M, seed):
    """(code u32[W], db u32[n, W]): every row is the query with some of its ferns changed -- few in most rows, so that small distances are crowded
    and tie -- and some rows are copies of others."""
    key = ("db", n, M, seed)
    if key not in _cache:
        g = np.random.default_rng(seed)
        Wn = M // 8
        code = g.integers(0, 1 << 32, size=Wn, dtype=np.uint64).astype(np.uint32)
        density = np.where(g.random(n) < 0.02, 0.0, 0.02 + 0.9 * g.random(n) ** 2)      # a few exact copies of the query, the rest spread out
        nib = (g.integers(0, 16, size=(n, M), dtype=np.uint8) * (g.random((n, M), dtype=np.float32) < density[:, None])).astype(np.uint32)
        shifted = nib.reshape(n, Wn, 8) << (4 * np.arange(8, dtype=np.uint32))[None, None, :]
        db = (np.bitwise_or.reduce(shifted, axis=2) ^ code[None, :]).astype(np.uint32)
        if n > 3:
            db[n // 3] = db[0]
            db[n - 1] = db[n // 2]
            db[1] = code                                   # distance 0, twice
            db[n - 2] = code
        dist = FR.distances(FR.unpack(code, M), FR.unpack_rows(db, M)) if n else np.zeros(0, np.int64)
        _cache[key] = (code, db, dist)
    return _cache[key]


class _Raw:
    """ovo_fern_search called directly, guard words around the code, dist_out and the result block."""

    def __init__(self):
        self.L, self.lib, self.F, _ = _libs()
        self.host = self.L.PinnedRing(66 + 16, np.int64, slots=1)      # 8 guard words on either side of the block

    def run(self, code, db, limits, k, with_dist, seq=SEQ):
        n, Wn = db.shape
        L, lib = self.L, self.lib
        code_buf = torch.from_numpy(np.concatenate([np.full(4, GUARD, np.uint32), code, np.full(4, GUARD, np.uint32)]).view(np.int32)).to(DEV)
        db_dev = torch.from_numpy(np.ascontiguousarray(db).view(np.int32).reshape(n, Wn)).to(DEV) if n else torch.zeros((1, Wn), dtype=torch.int32, device=DEV)
        dist = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        ws = torch.empty(int(lib.ovo_fern_search_workspace_bytes(n, k)), dtype=torch.uint8, device=DEV)
        self.host.view[:] = 0x5A5A
        status = lib.ovo_fern_search(C.c_void_p(code_buf.data_ptr() + 16), L.ptr(db_dev), n, Wn, (C.c_int32 * len(limits))(*limits), len(limits), k,
                                     C.c_void_p(dist.data_ptr() + 16) if with_dist else None, C.c_void_p(self.host.base + 64), seq, L.ptr(ws), ws.numel(),
                                     L.stream())
        L.check(status)
        torch.cuda.synchronize()
        block = np.array(self.host.view[0])
        assert (block[:8] == 0x5A5A).all() and (block[8 + 66:] == 0x5A5A).all()
        got_code = code_buf.cpu().numpy().view(np.uint32)
        assert (got_code[:4] == GUARD).all() and (got_code[-4:] == GUARD).all() and np.array_equal(got_code[4:-4], code)
        d = dist.cpu().numpy()
        assert (d[:4] == 0x5A5A5A5A).all() and (d[4 + n:] == 0x5A5A5A5A).all()
        if not with_dist:
            assert (d == 0x5A5A5A5A).all()
        return block[8:8 + 66].copy(), d[4:4 + n].copy()


def _raw():
    if "raw" not in _cache:
        _cache["raw"] = _Raw()
    return _cache["raw"]


def _expected_block(n, dist, limits, k, seq=SEQ):
    block = np.full(66, -1, dtype=np.int64)
    block[0], block[1] = seq, n
    for i, keys in enumerate(FR.result_lists(dist, limits, k)):
        block[2 + 16 * i:2 + 16 * i + k] = keys
    return block


# n: none, one, fewer than k, more than a wave's trip and no multiple of it, several virtual workgroups; W: one word (64 rows a wave trip), an odd
# count (8 lanes a row, 3 idle), the largest (a lane walks 8 words) -- the largest only at small n
SEARCH_CASES = [(0, 8), (1, 8), (5, 8), (257, 8), (70000, 8), (0, 40), (1, 40), (5, 40), (257, 40), (70000, 40), (1, 4096), (5, 4096), (257, 4096), (1500, 256),
                (300000, 8)]                                 # above 2^18 rows a virtual workgroup takes 2048 rows, not 1024


@pytest.mark.parametrize("n,M", SEARCH_CASES)
def test_search(n, M, monkeypatch):
    raw = _raw()
    code, db, dist = _database(n, M, 11)
    db = db.reshape(n, M // 8)
    limits = [0, n // 2, n]
    blocks = {}
    for k in (1, 4, 16):
        block, got_dist = raw.run(code, db, limits, k, with_dist=True)
        assert np.array_equal(got_dist.astype(np.int64), dist)
        want = _expected_block(n, dist, limits, k)
        assert np.array_equal(block, want), (k, block[:2 + 48], want[:2 + 48])
        without, _ = raw.run(code, db, limits, k, with_dist=False)      # dist_out NULL: the same block
        assert np.array_equal(without, block)
        blocks[k] = block
    full = blocks[16][2 + 32:2 + 48]
    found = full[full >= 0]
    ties = int((np.diff(found >> 32) == 0).sum())
    print(f"n={n} M={M}: nearest {[(int(x & 0xFFFFFFFF), int(x >> 32)) for x in found[:6]]}, {ties} ties among the {len(found)} best")
    if n > 3:
        assert ties >= 1 and int(found[0] >> 32) == 0 and int(found[1] >> 32) == 0      # the two copies of the query (at least), the lower row first
    if n < 16:
        assert len(found) == n                               # k > n: the list ends in -1
    # other limit sets: one limit, four limits, equal limits
    for lims in ([n], [0, 0, n, n], sorted([min(n, 1), min(n, 3), n // 2, n])):
        block, _ = raw.run(code, db, lims, 4, with_dist=False)
        assert np.array_equal(block, _expected_block(n, dist, lims, 4)), lims
    again, _ = raw.run(code, db, limits, 16, with_dist=True)    # run to run
    assert np.array_equal(again, blocks[16])
    monkeypatch.setenv("OVO_FERN_GRID_CAP", "2")               # two workgroups loop over all virtual ones
    capped, capped_dist = raw.run(code, db, limits, 16, with_dist=True)
    assert np.array_equal(capped, blocks[16]) and np.array_equal(capped_dist.astype(np.int64), dist)


def test_database_follows_the_restatement():
    """FernDatabase: add, search through the ring, the row -> keyframe map; a search sees the rows added before it and none after."""
    L, lib, F, U = _libs()
    M = 40
    code, db, dist = _database(257, M, 12)
    table = F.FernTable(M, (3, 4), seed=1, device=DEV)
    base = F.FernDatabase(table, 300, device=DEV)
    q = torch.from_numpy(code.view(np.int32)).to(DEV)
    assert [(len(r), len(d)) for r, d in base.search(q, [0], 4)] == [(0, 0)]      # empty: n = 0
    rows_dev = torch.from_numpy(db.view(np.int32).reshape(257, M // 8)).to(DEV)
    seqs = []
    for r in range(257):
        assert base.add(rows_dev[r]) == r
        base.set_row_keyframe(r, 2 * r)
        if r in (0, 99, 256):
            seqs.append((r + 1, base.queue(q, [(r + 1) // 2, r + 1], 16)))
    for n, seq in seqs:                                      # three searches in flight, read in order
        lists = base.wait(seq)
        for (rows, dists), lim in zip(lists, [n // 2, n]):
            want = FR.top_k(dist, lim, 16)
            assert rows.dtype == np.int32 and dists.dtype == np.int32
            assert [(int(a), int(b)) for a, b in zip(rows, dists)] == want
    assert base.keyframe_of(7) == 14 and base.n == 257
    with pytest.raises(L.OvoHipError, match="rows are taken"):
        for r in range(44):
            base.add(rows_dev[r])


def test_refused_calls_launch_nothing():
    L, lib, F, U = _libs()
    raw = _raw()
    assert lib.ovo_fern_search_workspace_bytes(-1, 4) == 0 and lib.ovo_fern_search_workspace_bytes((1 << 20) + 1, 4) == 0
    assert lib.ovo_fern_search_workspace_bytes(10, 0) == 0 and lib.ovo_fern_search_workspace_bytes(10, 17) == 0
    assert lib.ovo_fern_search_workspace_bytes(0, 1) > 0 and lib.ovo_fern_search_workspace_bytes(1 << 20, 16) >= lib.ovo_fern_search_workspace_bytes(70000, 16)
    n, M = 257, 40
    Wn = M // 8
    code, db, dist = _database(n, M, 11)
    code_dev = torch.from_numpy(code.view(np.int32)).to(DEV)
    db_dev = torch.from_numpy(db.view(np.int32).reshape(n, Wn)).to(DEV)
    out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    ws = torch.full((int(lib.ovo_fern_search_workspace_bytes(n, 16)),), 0x5A, dtype=torch.uint8, device=DEV)
    raw.host.view[:] = 0x5A5A
    block = raw.host.base + 64

    def search(code_p=code_dev.data_ptr(), db_p=db_dev.data_ptr(), n_=n, W_=Wn, limits=(0, n), n_limits=None, k=4, host=block, seq=SEQ, ws_p=ws.data_ptr(),
               ws_bytes=ws.numel(), limits_null=False):
        lims = (C.c_int32 * max(len(limits), 1))(*limits)
        return lib.ovo_fern_search(C.c_void_p(code_p), C.c_void_p(db_p), n_, W_, None if limits_null else lims, len(limits) if n_limits is None else n_limits, k,
                                   L.ptr(out), C.c_void_p(host), seq, C.c_void_p(ws_p), ws_bytes, L.stream())

    refused = [search(code_p=0), search(db_p=0), search(limits_null=True), search(host=0), search(ws_p=0), search(n_=-1), search(n_=(1 << 20) + 1),
               search(W_=0), search(W_=513), search(k=0), search(k=17), search(limits=(), n_limits=0), search(limits=(0, 1, 2, 3, 4)),
               search(limits=(0, n + 1)), search(limits=(-1, n)), search(limits=(5, 4)), search(code_p=code_dev.data_ptr() + 2),
               search(db_p=db_dev.data_ptr() + 1), search(host=block + 4), search(seq=0), search(ws_bytes=ws.numel() - 1), search(ws_p=ws.data_ptr() + 4)]
    # encode
    depth = _depth(24, 36, 3)
    frame = U.prepare_frame(torch.from_numpy(depth).to(DEV), K_SMALL, 3, 4.0, 0.1)
    table = F.FernTable(M, (6, 9), seed=5, device=DEV)       # made for the coarsest level, 6 x 9
    big = F.FernTable(M, (12, 18), seed=5, device=DEV)       # made for level 1
    pyramid_before = frame.pyramid.clone()
    word = torch.full((Wn,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)

    def enc(pyr=frame.pyramid.data_ptr(), desc=frame.desc, level=2, pix=table.pix_dev.data_ptr(), tau=table.tau_dev.data_ptr(), M_=M, limit=54, out_p=word.data_ptr()):
        return lib.ovo_fern_encode(C.c_void_p(pyr), C.byref(desc) if desc is not None else None, level, C.c_void_p(pix), C.c_void_p(tau), M_, limit,
                                   C.c_void_p(out_p), L.stream())

    bad_desc = U.frame_desc(24, 36, K_SMALL, 5, 4.0, 0.1)
    refused += [enc(pyr=0), enc(desc=None), enc(pix=0), enc(tau=0), enc(out_p=0), enc(level=-1), enc(level=3), enc(M_=0), enc(M_=12), enc(M_=4104),
                enc(limit=55), enc(limit=0), enc(level=2, pix=big.pix_dev.data_ptr(), limit=big.pixels), enc(desc=bad_desc), enc(pyr=frame.pyramid.data_ptr() + 8),
                enc(out_p=word.data_ptr() + 2)]
    torch.cuda.synchronize()
    assert refused == [-1] * len(refused)
    with pytest.raises(L.OvoHipError, match="ovo_fern_encode"):
        L.check(refused[-1])
    with pytest.raises(L.OvoHipError, match="the pix table was made for more pixels than the level has"):
        F.encode(frame, big, level=2)
    assert (out == 0x5A5A5A5A).all() and (ws == 0x5A).all() and (np.array(raw.host.view) == 0x5A5A).all() and (word == 0x5A5A5A5A).all()
    assert torch.equal(frame.pyramid, pyramid_before)
    assert search() == 0 and enc() == 0 and enc(level=1, pix=big.pix_dev.data_ptr(), limit=big.pixels) == 0      # the same calls with nothing wrong go through
    torch.cuda.synchronize()
    assert int(raw.host.view[0, 8]) == SEQ and int(raw.host.view[0, 9]) == n
    with pytest.raises(ValueError, match="outside the 6 x 9 level"):
        F.FernTable(M, (6, 9), device=DEV, pix=big.pix, tau=big.tau)
