"""The host side of the keyframe chain (no GPU): the argument checks of ovo_map_step, ovo_track_step and ovo_keyframe_step -- every one of them before
anything is queued, and under the name of the entry point that was called -- and the size of the tracking workspace."""
import pytest

H, W, DS = 32, 32, 2                      # 1024 pixels: a shape ovo_keyframe_step's merged launches take
N_SUB = (H // DS) * (W // DS)
N_UPPER, N_MASKS, COLS = 100, 3, 5


def _map_step(L, lib, h=H, w=W, **kw):
    """An ovo_map_step_t that passes every check, on made-up, well separated, never dereferenced addresses: a call that passes the checks would reach
    the device, so every case here has to fail them."""
    n_sub = -(-h // DS) * -(-w // DS)
    a = L.MapStep()
    a.map = L.MapRef(0x10000, 0x20000, 0x30000, 0x40000, N_UPPER + n_sub, 0x50000, -1, -1)
    a.depth, a.rgb, a.h, a.w, a.ds, a.n_upper = 0x60000, 0x70000, h, w, DS, N_UPPER
    a.explained, a.ws, a.ws_bytes = 0x80000, 0x90000, lib.ovo_compact_workspace_bytes(n_sub) + 8
    for k, v in kw.items():
        setattr(a.map if k in ("cap", "n") else a, k, v)
    return a


def _short(step):
    step.ws_bytes -= 1
    return step


def _track_step(L, lib, **kw):
    t = L.TrackStep()
    t.map = L.MapRef(0x10000, 0x20000, 0x30000, 0x40000, N_UPPER + N_SUB, 0x50000, -1, -1)
    t.depth, t.seg_map, t.seg_h, t.seg_w, t.point_seg = 0x110000, 0x120000, H, W, 0x130000
    t.n_masks, t.hist_cols, t.n_upper, t.next_ins, t.next_ins_host = N_MASKS, COLS, N_UPPER, 0x140000, -1
    t.ws, t.ws_bytes = 0x150000, lib.ovo_track_workspace_bytes(N_MASKS, COLS)
    for k, v in kw.items():
        setattr(t.map if k in ("cap", "n") else t, k, v)
    return t


_HITS = {"hits": 0x160000, "n_hits": 0x170000}
TRACK_CASES = [
    ("hits without n_hits", {"hits": 0x160000}),
    ("hit shard rank out of range", {**_HITS, "hit_shard_count": 2, "hit_shard_rank": 2, "hit_shard_block": 64}),
    ("negative hit shard rank", {**_HITS, "hit_shard_count": 2, "hit_shard_rank": -1, "hit_shard_block": 64}),
    ("hit shard block not a power of two", {**_HITS, "hit_shard_count": 2, "hit_shard_rank": 1, "hit_shard_block": 48}),
    ("filter_depth without depth_scratch", {"filter_depth": 1}),
    ("workspace one byte short", None),
    ("map.n > n_upper", {"n": N_UPPER + 1}),
    ("no masks", {"n_masks": 0}),
    ("8193 masks", {"n_masks": 8193}),
]
MAP_CASES = [
    ("null explained", {"explained": 0}),
    ("ds == 0", {"ds": 0}),
    ("map.cap one below n_upper + n_sub", {"cap": N_UPPER + N_SUB - 1}),
    ("workspace one byte short", None),
]


def _failed(lib, rc, name, case):
    assert rc == -1, case                                                             # OVO_E_ARG: not a launch error, not OVO_OK
    assert lib.ovo_hip_last_error().startswith(name + b": "), (case, lib.ovo_hip_last_error())


@pytest.mark.parametrize("case, kw", TRACK_CASES)
def test_track_step_argument_errors_are_reported_before_any_launch(case, kw):
    from ovo_amd import _lib as L
    lib = L.load()
    t = _short(_track_step(L, lib)) if kw is None else _track_step(L, lib, **kw)
    _failed(lib, lib.ovo_track_step(L.C.byref(t), None), b"ovo_track_step", case)


@pytest.mark.parametrize("case, kw", MAP_CASES)
def test_map_step_argument_errors_are_reported_before_any_launch(case, kw):
    from ovo_amd import _lib as L
    lib = L.load()
    a = _short(_map_step(L, lib)) if kw is None else _map_step(L, lib, **kw)
    _failed(lib, lib.ovo_map_step(L.C.byref(a), None), b"ovo_map_step", case)


@pytest.mark.parametrize("h, w", [(H, W), (30, 36)])              # a shape the merged form takes; one it hands to the single steps (h * w % 16 != 0)
@pytest.mark.parametrize("case, kw", [
    ("bad hit shard rank", {**_HITS, "hit_shard_count": 2, "hit_shard_rank": 2, "hit_shard_block": 64}),
    ("filter_depth without depth_scratch", {"filter_depth": 1}),
])
def test_keyframe_step_checks_both_halves_before_any_launch(h, w, case, kw):
    """A valid map half with a bad tracking half: nothing of the map half may be queued (a memset or a launch without a device would not come back as
    OVO_E_ARG under ovo_keyframe_step's name)."""
    from ovo_amd import _lib as L
    lib = L.load()
    a, t = _map_step(L, lib, h=h, w=w), _track_step(L, lib, **kw)
    _failed(lib, lib.ovo_keyframe_step(L.C.byref(a), L.C.byref(t), None), b"ovo_keyframe_step", case)


def test_round_chain_refuses_a_frame_past_the_one_workgroup_scan():
    """258 x 512 at ds = 1: 2064 flag words, 16 more than the single workgroup of the one-launch form scans.  `ovo_round_chain` answers OVO_E_UNSUPPORTED (the
    caller then goes keyframe by keyframe) before it writes a parameter slot or launches: the addresses here are made up.  A production build carries no
    one-launch form at all and says so with the same code."""
    from ovo_amd import _lib as L
    lib = L.load()
    h, w = 258, 512
    a = _map_step(L, lib, h=h, w=w, ds=1, cap=N_UPPER + h * w, ws_bytes=lib.ovo_compact_workspace_bytes(h * w) + 8)
    ctx = L.RoundChain(0x200000, 0x210000, 0, 0, 0)
    rc = lib.ovo_round_chain(L.C.byref(ctx), (L.MapStep * 1)(a), (L.TrackStep * 1)(_track_step(L, lib)), 1, None)
    assert rc == L.E_UNSUPPORTED == -3
    if lib.ovo_round_chain_params_bytes() == 0:
        assert lib.ovo_hip_last_error().startswith(b"ovo_round_chain: not in this build")
    else:
        assert lib.ovo_hip_last_error() == b"ovo_round_chain: frame too large for the one-workgroup scan"
        assert (ctx.next_slot, ctx.arrivals) == (0, 0)


@pytest.mark.parametrize("n", [1, 2, 3, 168, 1024, 8192])
@pytest.mark.parametrize("c", [1, 2, 3, 64, 257])
def test_track_workspace_bytes(n, c):
    """hist | stats[4 n] | counters (32 slots x 16 u64 words) | tickets (2 + n) | dst[n] | result block [8 + 6 n], + 4 words (alignment of the counters)."""
    from ovo_amd import _lib as L
    assert L.load().ovo_track_workspace_bytes(n, c) == (n * c + 4 * n + 2 * 32 * 16 + 2 + n + n + 8 + 6 * n + 4) * 4
