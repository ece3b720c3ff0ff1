"""No device: the host bookkeeping both tracking paths share (ovo_amd/entities/ovo.py: `_walk_masks` + `_keep_rows`) against values worked
by hand from the reference's rules (ovo.py:255-322) -- a mask with more than track_th projected points either joins the mode instance of its
assigned points (more than track_th of them) or, with more than track_th unassigned points, opens the next instance id; an instance keeps
the row of its FIRST mask, and every mask names the kept row it contributes to."""
import pytest

from ovo_amd import _lib as L
from ovo_amd.entities.instance3d import Instance3D
from ovo_amd.entities.ovo import OVO

# rows (projected points, assigned points, mode instance of the assigned points, mask area); track_th = 10
KF0 = [(5, 0, -1, 100), (50, 0, -1, 200), (40, 0, -1, 300)]
KF1 = [(60, 30, 0, 150), (45, 20, 0, 120), (30, 5, 1, 90), (12, 11, 1, 80), (25, 10, 0, 70)]
# kf 0: mask 0 too few points; masks 1, 2: 50 / 40 unassigned -> new instances 0, 1
WANT0 = ([0, 1], [1, 2], [-1, 0, 1])
# kf 1: masks 0, 1 -> instance 0 (30, 20 assigned); mask 2: 5 assigned, 25 unassigned -> new instance 2; mask 3: 11 assigned -> instance 1;
# mask 4: 10 assigned is not MORE than 10, 15 unassigned -> new instance 3.  Rows in order of first appearance: 0, 2, 1, 3
WANT1 = ([0, 2, 1, 3], [0, 2, 3, 4], [0, 0, 1, 2, 3])
DEVICE_TARGETS1 = [-1, -1, 2, -1, 3]


def _ovo():
    ovo = object.__new__(OVO)                                       # the bookkeeping needs no encoder, bank or device
    ovo.config, ovo.n_top_views, ovo.bank = {"track_th": 10}, 0, None
    ovo.objects, ovo.next_ins_id = {}, 0
    Instance3D.n_top_kf = 0
    return ovo


def _keyframe(ovo, table, kf_id, device_next=None):
    info, target = ovo._walk_masks(table, kf_id, device_next)
    areas = {m: row[5] for m, row in enumerate(table) if len(row) > 5}
    return ovo._keep_rows(info, kf_id, len(table), areas.__getitem__), target


def _six(table, targets):
    return [row + (t, row[3]) for row, t in zip(table, targets)]


@pytest.mark.parametrize("device", [False, True])
def test_walk_and_keep_rows_by_hand(device):
    ovo = _ovo()
    got0, target0 = _keyframe(ovo, _six(KF0, [-1, 0, 1]) if device else KF0, 0, 2 if device else None)
    assert got0 == WANT0 and target0 == [-1, 0, 1] and ovo.next_ins_id == 2
    got1, target1 = _keyframe(ovo, _six(KF1, DEVICE_TARGETS1) if device else KF1, 1, 4 if device else None)
    assert got1 == WANT1 and target1 == [0, 0, 2, 1, 3] and ovo.next_ins_id == 4
    assert sorted(ovo.objects) == [0, 1, 2, 3]
    assert ovo.objects[0].kfs_ids == [0, 1] and ovo.objects[1].kfs_ids == [0, 1]
    assert ovo.objects[2].kfs_ids == [1] and ovo.objects[3].kfs_ids == [1]
    assert all(o._bank is None for o in ovo.objects.values())


def test_device_ids_that_diverge_are_an_error():
    ovo = _ovo()
    _keyframe(ovo, KF0, 0)
    with pytest.raises(L.OvoHipError, match="instance ids diverged"):
        ovo._walk_masks(_six(KF1, [-1, -1, 3, -1, 2]), 1, 4)
    ovo = _ovo()
    _keyframe(ovo, KF0, 0)
    with pytest.raises(L.OvoHipError, match="next instance id diverged"):
        ovo._walk_masks(_six(KF1, DEVICE_TARGETS1), 1, 5)


def test_fused_area_feeds_the_top_view_heap():
    """n_top_views = 1: the heap holds one view per instance.  Instance 0 enters it at keyframe 0 with area 200; at keyframe 1 its masks 0
    and 1 (areas 150, 120) are fused and the fused area 260 -- column 5 of the first mask -- replaces it; instance 1 (area 300 at keyframe
    0, 80 at keyframe 1) keeps keyframe 0, so its mask gets no row at keyframe 1."""
    ovo = _ovo()
    ovo.n_top_views = Instance3D.n_top_kf = 1
    try:
        assert _keyframe(ovo, KF0, 0)[0] == WANT0
        table = _six(KF1, DEVICE_TARGETS1)
        table[0] = table[0][:5] + (260,)
        got, _ = _keyframe(ovo, table, 1, 4)
        assert got == ([0, 2, 3], [0, 2, 4], [0, 0, 1, -1, 2])
        assert ovo.objects[0].top_kf == [(260, 1)] and ovo.objects[1].top_kf == [(300, 0)]
    finally:
        Instance3D.n_top_kf = 0
