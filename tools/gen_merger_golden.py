"""Golden fixture of the learned crop-merging weights predictor: `python tools/gen_merger_golden.py --reference DIR`.

Imports the reference's ovo/entities/clips_merging.py on the CPU, builds two reduced configurations (o_dim = 3 d and o_dim = 3), seeds
the weights (every Linear scaled by GAIN so that the softmax over the clips is far from uniform), and writes state dict, inputs and
outputs to tests/golden/clips_merging.npz; copies the base hparams.yaml (settings only) next to it.
"""
import argparse
import importlib.util
import json
import os
import shutil

import numpy as np
import torch

CONFIGS = {
    "per_channel": {"transformer": {"d_model": 64, "dim_feedforward": 48, "dropout": 0.4, "n_layers": 2},
                    "mlp": {"act_key": "leaky_relu", "i_dim": 192, "h_dim": 80, "n_layers": 1, "o_dim": 192}},
    "per_row": {"transformer": {"d_model": 64, "dim_feedforward": 64, "dropout": 0.4, "n_layers": 1},
                "mlp": {"act_key": "silu", "i_dim": 192, "h_dim": 96, "n_layers": 2, "o_dim": 3}},
}
GAIN, ROWS = 3.0, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_clips_merging", os.path.join(a.reference, "ovo", "entities", "clips_merging.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    arrays = {"configs": np.frombuffer(json.dumps(CONFIGS).encode(), dtype=np.uint8)}
    for k, (name, cfg) in enumerate(CONFIGS.items()):
        torch.manual_seed(100 + k)
        model = ref.WeightsPredictorMerger(cfg).eval()
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, torch.nn.Linear):
                    m.weight.mul_(GAIN)
            model.att_encoder.layers[0].self_attn.in_proj_weight.mul_(GAIN)
            x = torch.nn.functional.normalize(torch.randn(ROWS, 3, cfg["transformer"]["d_model"]), dim=-1)
            y = model(x)
        for key, v in model.state_dict().items():
            arrays[f"{name}/sd/{key}"] = v.numpy().astype(np.float32)
        arrays[f"{name}/x"], arrays[f"{name}/y"] = x.numpy(), y.numpy()
    np.savez_compressed(os.path.join(a.out, "clips_merging.npz"), **arrays)
    shutil.copyfile(os.path.join(a.reference, "data", "input", "weights_predictor", "base", "hparams.yaml"),
                    os.path.join(a.out, "weights_predictor_base_hparams.yaml"))
    print("wrote", os.path.join(a.out, "clips_merging.npz"), os.path.getsize(os.path.join(a.out, "clips_merging.npz")), "bytes")


if __name__ == "__main__":
    main()
