"""CPU: the host half of the evaluation step (utils/eval_utils.py: get_iou, iou_acc_from_confmat, process_txt) against what the reference's
own functions returned for the same matrices (tests/golden/eval_host.npz, tools/gen_eval_golden.py).  Exact: the same numpy
expressions on the same integers -- NaNs in the same places, every other value `==`."""
import numpy as np
import pytest

from conftest import golden

CASES = ("m21", "m51", "m7")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("name", CASES)
def test_get_iou_matches_reference(name):
    from ovo_amd.utils import eval_utils as E
    d = golden("eval_host")
    conf = d[f"{name}_confusion"]
    got = np.array([E.get_iou(i, conf) for i in range(conf.shape[0])], dtype=np.float64)
    assert np.isnan(d[f"{name}_get_iou"]).any()                      # the fixture does hold empty classes
    _same(got, d[f"{name}_get_iou"])


@pytest.mark.parametrize("mask_nan", (True, False))
@pytest.mark.parametrize("name", CASES)
def test_iou_acc_from_confmat_matches_reference(name, mask_nan):
    from ovo_amd.utils import eval_utils as E
    d = golden("eval_host")
    conf, ignore = d[f"{name}_confusion"], [int(v) for v in d[f"{name}_ignore"]]
    tag = f"{name}_{'masknan' if mask_nan else 'keepnan'}"
    iou, iou_ok, w, acc, acc_ok = E.iou_acc_from_confmat(conf, conf.shape[0], ignore, mask_nan)
    assert len(iou) == conf.shape[0] - len(ignore)
    _same(iou, d[f"{tag}_iou"])
    _same(acc, d[f"{tag}_acc"])
    assert w.dtype == d[f"{tag}_w"].dtype and np.array_equal(w, d[f"{tag}_w"])
    assert iou_ok.dtype == bool and np.array_equal(iou_ok, d[f"{tag}_iou_ok"])
    assert acc_ok.dtype == bool and np.array_equal(acc_ok, d[f"{tag}_acc_ok"])


def test_iou_acc_verbose_prints_one_line_per_kept_class(capsys):
    from ovo_amd.utils import eval_utils as E
    d = golden("eval_host")
    conf = d["m7_confusion"]
    E.iou_acc_from_confmat(conf, 7, [3], True, True, [f"c{i}" for i in range(7)])
    out = capsys.readouterr().out.splitlines()
    assert out[1] == " classes \t IoU \t Acc" and out[2] == "-" * 28
    assert [line.split(":")[0].strip() for line in out[3:]] == ["c0", "c1", "c2", "c4", "c5", "c6"]


def test_process_txt_matches_reference(tmp_path):
    from ovo_amd.utils import eval_utils as E
    d = golden("eval_host")
    path = tmp_path / "labels.txt"
    path.write_bytes(d["txt_bytes"].tobytes())
    assert E.process_txt(str(path)) == [str(s) for s in d["txt_lines"]]
    assert E.process_txt(path) == [str(s) for s in d["txt_lines"]]


def test_reference_names_are_present():
    from ovo_amd.utils import eval_utils as E
    for name in ("match_labels_to_vtx", "update_confmat", "evaluate_scan", "process_txt", "get_iou", "iou_acc_from_confmat", "eval_semantics"):
        assert callable(getattr(E, name))
