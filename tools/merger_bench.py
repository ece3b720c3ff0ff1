"""Base-size weights predictor: ms per call and weight bytes / time of the MLP at M in {1, 8, 32, 64, 128, 256}, through ovo_gemm_fewrows (the host's
row limit lifted: fewrows_max_m) and, with OVO_MERGER_NO_FEWROWS, through ovo_gemm, alternating, every measurement in a child process under its own
`timeout`.  Each RESULT line carries `mlp_routes`, the entry that actually ran each of the six MLP layers; `--extract` times extract_clip with the
dispatch that ships.
`python tools/merger_bench.py [--out FILE] [--extract]`; `--one M ROUTE` is the child."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MS = (1, 8, 32, 64, 128, 256)


def one(m: int, route: str, extract: bool):
    if route == "gemm":
        os.environ["OVO_MERGER_NO_FEWROWS"] = "1"
    import torch
    import yaml
    from ovo_amd.entities.clips_merging import WeightsPredictorMerger, random_state_dict
    res = {"M": m, "route": route}
    if extract:
        from ovo_amd.entities.clip_generator import CLIPGenerator
        import shutil, tempfile
        d = tempfile.mkdtemp()
        shutil.copyfile(os.path.join(ROOT, "tests", "golden", "weights_predictor_base_hparams.yaml"), os.path.join(d, "hparams.yaml"))
        image = (torch.rand(3, 480, 640) * 255).cuda()
        masks = torch.zeros(32, 480, 640, dtype=torch.bool, device="cuda")
        for i in range(32):
            masks[i, 10 + 12 * i:70 + 13 * i, 15 + 17 * i:65 + 19 * i] = True
        for et in ("fixed_weights", "learned"):
            g = CLIPGenerator({"embed_type": et, "model_card": "SigLIP-384", "weights_predictor_path": d})
            for _ in range(3):
                g.extract_clip(image, masks)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                g.extract_clip(image, masks)
            torch.cuda.synchronize()
            res["extract_clip_ms_" + et] = (time.perf_counter() - t0) / 10 * 1e3
            if et == "learned":
                res["route"], res["mlp_routes"] = "shipped dispatch", g.clips_fusion_model.mlp_routes
            del g
    else:
        with open(os.path.join(ROOT, "tests", "golden", "weights_predictor_base_hparams.yaml")) as f:
            cfg = yaml.safe_load(f)["model"]
        cfg["transformer"]["n_layers"] = 0                           # the MLP alone: the encoder layers run on ovo_gemm either way
        model = WeightsPredictorMerger(cfg, random_state_dict(cfg, 0), device="cuda", fewrows_max_m=max(MS) if route == "fewrows" else 0)
        x = torch.nn.functional.normalize(torch.randn(m, 3, 1152, device="cuda"), dim=-1)
        for _ in range(5):
            model(x)
        torch.cuda.synchronize()
        reps = 40
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            model(x)
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / reps
        res.update(mlp_routes=model.mlp_routes, ms_per_call=ms, weight_bytes=model.weight_bytes(), weight_TBps=model.weight_bytes() / (ms * 1e-3) / 1e12)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2)
    ap.add_argument("--extract", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.one:
        return one(int(a.one[0]), a.one[1], a.extract)
    lines = []
    jobs = [(m, r, False) for m in MS for r in ("fewrows", "gemm", "fewrows", "gemm")] + ([(32, "fewrows", True)] if a.extract else [])
    for m, r, ex in jobs:
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--one", str(m), r] + (["--extract"] if ex else [])
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(f"M={m} {r}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
            return 1                                                  # nothing more is started on the GPU after a failure
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
