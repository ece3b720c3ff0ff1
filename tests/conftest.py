import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")
# several tests flip the library's OVO_* tuning knobs (monkeypatch.setenv) between launches of this one process: the library reads them once
# per process unless this is set before its first launch (ovo_amd/csrc/common.h: ovo_knobs_dynamic)
os.environ.setdefault("OVO_KNOBS_DYNAMIC", "1")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_modifyitems(config, items):
    """A plain `pytest tests/` on a GPU-less host runs the CPU suite and SKIPS the `gpu`-marked tests (they need a real MI355X)."""
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="needs a real MI355X (run with -m gpu on the GPU box)")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


class _Parts(dict):
    """The members of a fixture stored in parts, with the `files` list of np.load's result."""

    @property
    def files(self):
        return list(self)


def golden(name: str):
    """tests/golden/<name>.npz; a fixture over the 1 MiB file limit continues in <name>.part1.npz, ... (tools/gen_golden.py: save_parts)."""
    first = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    parts = sorted(glob.glob(os.path.join(GOLDEN, glob.escape(name) + ".part*.npz")), key=lambda p: int(p[:-len(".npz")].rsplit(".part", 1)[1]))
    if not parts:
        return first
    return _Parts((k, f[k]) for f in [first] + [np.load(p, allow_pickle=False) for p in parts] for k in f.files)


def unpack(bits: np.ndarray, w: int) -> np.ndarray:
    return np.unpackbits(bits, axis=-1)[..., :w].astype(bool)


@pytest.fixture(scope="session")
def has_gpu():
    import torch
    return torch.cuda.is_available()
