"""embed_type "learned" without a GPU: the fp32 restatement against the reference's recorded outputs, layer shapes, ABI symbols."""
import json
import os
import re

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, ROOT, golden
from merger_restatement import forward


def load_golden():
    z = golden("clips_merging")
    cfgs = json.loads(bytes(z["configs"]).decode())
    out = {}
    for name, cfg in cfgs.items():
        sd = {k[len(name) + 4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "/sd/")}
        out[name] = (cfg, sd, torch.from_numpy(z[name + "/x"]), torch.from_numpy(z[name + "/y"]))
    return out


@pytest.mark.parametrize("name", ["per_channel", "per_row"])
def test_restatement_reproduces_reference(name):
    cfg, sd, x, y = load_golden()[name]
    got = forward(sd, cfg, x)
    err = (got - y).abs().max().item()
    print(f"{name}: restatement vs reference max abs {err:.3e}")
    assert err <= 2e-6
    assert torch.allclose(y.norm(dim=-1), torch.ones(len(y)), atol=1e-5)


def test_golden_weights_are_not_uniform():
    for name, (cfg, sd, x, y) in load_golden().items():
        _, w = forward(sd, cfg, x, want_weights=True)
        assert w.max(dim=1).values.mean().item() >= 0.5, name


def test_base_layer_shapes_without_gpu():
    from ovo_amd.entities.clips_merging import WeightsPredictorMerger
    with open(os.path.join(GOLDEN, "weights_predictor_base_hparams.yaml")) as f:
        hp = yaml.safe_load(f)
    m = WeightsPredictorMerger(hp["model"], device=None)
    sh = m.layer_shapes
    assert sh["n_encoder_layers"] == 5 and m.nhead == 8 and m.d == 1152
    assert [s for _, s in sh["encoder_layer"]] == [(3456, 1152), (1152, 1152), (1152, 1152), (1152, 1152)]
    assert sh["mlp"] == [(13824, 3456)] + [(13824, 13824)] * 4 + [(3456, 13824)]
    assert sum(o * i for o, i in sh["mlp"]) == 859963392
    assert m.layers == [] and m.mlp == []


def test_abi_declares_merger_symbols():
    from ovo_amd import _lib
    header = open(os.path.join(ROOT, "include", "ovo_hip.h")).read()
    for sym in ("ovo_gemm_fewrows", "ovo_attention_short", "ovo_merge_clips"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
        assert sym in _lib.exported_symbols()
    assert _lib.ABI_VERSION >= 14
