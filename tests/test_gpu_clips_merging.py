"""embed_type "learned" on the GPU: ovo_gemm_fewrows, ovo_attention_short, ovo_merge_clips, the whole WeightsPredictorMerger and CLIPGenerator.

Whole-merger error bound: ef <= 1.5 ep + 1e-4 (max abs on the unit-norm output), ep = the error of the SAME restatement with weights and the input
of every product rounded to bf16, taken on the CPU: the number format's own floor (the form of the LayerNorm-fold tests)."""
import ctypes as C
import math
import os
import shutil

import pytest
import torch

from conftest import GOLDEN
from merger_restatement import ACTS, bf16_round, forward, merge
from test_clips_merging import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
ACT_NAME = {0: None, 3: "relu", 4: "sigmoid", 6: "leaky_relu", 7: "silu"}


def _few(a, w, bias, act=0, out_dtype=torch.float32, add=None, entry="ovo_gemm_fewrows"):
    from ovo_amd import _lib as L
    out = torch.empty(a.shape[0], w.shape[0], dtype=out_dtype, device=DEV)
    L.check(getattr(L.load(), entry)(C.byref(L.gemm_desc(a, w, out, bias=bias, add=add, act=act)), L.stream()))
    return out


@pytest.mark.parametrize("k,n", [(3456, 13824), (13824, 13824), (13824, 3456), (192, 80)])
def test_gemm_fewrows_vs_fp64(k, n):
    gen = torch.Generator().manual_seed(k + n)
    w = (torch.randn(n, k, generator=gen) * k ** -0.5).to(DEV, torch.bfloat16)
    bias = torch.randn(n, generator=gen).to(DEV)
    wd = w.double()
    for m in (1, 3, 16, 17, 32, 64):
        a = torch.randn(m, k, generator=gen).to(DEV, torch.bfloat16)
        z = a.double() @ wd.T + bias.double()
        for act, name in ACT_NAME.items():
            ref = (ACTS[name](z) if name else z).float()
            out = _few(a, w, bias, act)
            again = _few(a, w, bias, act)
            assert torch.equal(out, again), (m, act)                    # fixed reduction order: bit-identical launches
            torch.testing.assert_close(out, ref, atol=3e-4, rtol=3e-4, msg=lambda s: f"M={m} act={act}: {s}")
        add = torch.randn(m, n, generator=gen).to(DEV)
        torch.testing.assert_close(_few(a, w, bias, 0, add=add), (z + add.double()).float(), atol=3e-4, rtol=3e-4)
        torch.testing.assert_close(_few(a, w, bias, 6, torch.bfloat16).float(), ACTS["leaky_relu"](z).float(), atol=2e-2, rtol=2e-2)


def test_gemm_fewrows_row_blocks_and_unsupported():
    from ovo_amd import _lib as L
    gen = torch.Generator().manual_seed(5)
    a = torch.randn(150, 256, generator=gen).to(DEV, torch.bfloat16)
    w = (torch.randn(96, 256, generator=gen) / 16).to(DEV, torch.bfloat16)
    bias = torch.randn(96, generator=gen).to(DEV)
    torch.testing.assert_close(_few(a, w, bias, 7), ACTS["silu"](a.double() @ w.double().T + bias.double()).float(), atol=3e-4, rtol=3e-4)
    # ovo_gemm takes the two activations as well (the route above the crossover and with OVO_MERGER_NO_FEWROWS)
    for act, name in ((6, "leaky_relu"), (7, "silu")):
        torch.testing.assert_close(_few(a, w, bias, act, entry="ovo_gemm"), ACTS[name](a.double() @ w.double().T + bias.double()).float(), atol=3e-4, rtol=3e-4)
    out = torch.full((4, 96), 7.0, device=DEV)
    g = L.gemm_desc(a, w, out, rows=4)
    g.K = 224                                                                                          # K % 64 != 0
    assert L.load().ovo_gemm_fewrows(C.byref(g), L.stream()) == L.E_UNSUPPORTED
    g.K, g.act = 256, 1                                                                                # GELU is not one of its activations
    assert L.load().ovo_gemm_fewrows(C.byref(g), L.stream()) == L.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                                    # nothing launched


def _att_ref(qkv, scale):
    q, k, v = (qkv[:, :, j].permute(0, 2, 1, 3).double() for j in range(3))
    o = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1) @ v
    return o.permute(0, 2, 1, 3).reshape(qkv.shape[0], qkv.shape[1], -1).float()


@pytest.mark.parametrize("b,t,h,hd", [(32, 3, 8, 144), (5, 8, 4, 64), (2, 1, 2, 8), (3, 5, 1, 1032)])
def test_attention_short(b, t, h, hd):
    from ovo_amd import _lib as L
    gen = torch.Generator().manual_seed(b * t + hd)
    qkv = torch.randn(b, t, 3, h, hd, generator=gen).to(DEV, torch.bfloat16)
    out = torch.empty(b, t, h * hd, dtype=torch.bfloat16, device=DEV)
    scale = 1.0 / math.sqrt(hd)
    L.check(L.load().ovo_attention_short(L.ptr(qkv), b, t, h, hd, scale, L.ptr(out), L.stream()))
    torch.testing.assert_close(out.float(), _att_ref(qkv, scale), atol=2e-2, rtol=1.6e-2)              # one bf16 rounding of O(1) values
    if hd == 64:                                                                                       # the MFMA attention on the same packed tensor
        o2 = torch.empty_like(out)
        a = L.attention_packed(qkv, o2, b, h, t, t, hd, scale=scale)
        L.check(L.load().ovo_attention(C.byref(a), L.stream()))
        torch.testing.assert_close(out.float(), o2.float(), atol=4e-2, rtol=3.2e-2)                    # two roundings vs one


@pytest.mark.parametrize("per_row", [0, 1])
def test_merge_clips(per_row):
    from ovo_amd import _lib as L
    gen = torch.Generator().manual_seed(11 + per_row)
    b, d = 9, 1152
    clips = torch.nn.functional.normalize(torch.randn(b, 3, d, generator=gen), dim=-1)
    logits = torch.randn(b, 3 if per_row else 3 * d, generator=gen) * 4
    logits[0] = 0.25                                                    # a row whose three logits are equal (per channel: in every channel)
    ld = 32 if per_row else 3 * d
    lg = torch.zeros(b, ld)
    lg[:, :logits.shape[1]] = logits
    out = torch.empty(b, d, device=DEV)
    lg_d, clips_d = lg.to(DEV), clips.to(DEV)
    L.check(L.load().ovo_merge_clips(L.ptr(lg_d), ld, per_row, L.ptr(clips_d), b, d, L.ptr(out), L.stream()))
    ref, _ = merge(logits, clips, 3 if per_row else 3 * d)
    torch.testing.assert_close(out.cpu(), ref, atol=2e-6, rtol=1e-5)
    torch.testing.assert_close(out[0].cpu(), torch.nn.functional.normalize(clips[0].mean(0), dim=-1), atol=2e-6, rtol=1e-5)


def _check_merger(cfg, sd, x, label, model=None):
    from ovo_amd.entities.clips_merging import WeightsPredictorMerger
    ref, w = forward(sd, cfg, x, want_weights=True)
    peak = w.max(dim=1).values.mean().item()
    floor = forward(sd, cfg, x, rnd=bf16_round)
    ep = (floor - ref).abs().max().item()
    model = model or WeightsPredictorMerger(cfg, sd, device=DEV)
    got = model(x.to(DEV)).cpu()
    ef = (got - ref).abs().max().item()
    print(f"{label}: mean largest merge weight {peak:.3f}  ep {ep:.3e}  ef {ef:.3e}  MLP layers per entry {model.mlp_routes}")
    assert peak >= 0.6, "the seeded weights leave the softmax near uniform: the test could not see an error in the logits"
    assert torch.allclose(got.norm(dim=-1), torch.ones(len(got)), atol=1e-5)
    assert ef <= 1.5 * ep + 1e-4, (ef, ep)
    return model, got


GAIN = 3.0        # every Linear of the seeded models is scaled by this (default init shrinks the activations layer by layer and the softmax collapses to 1/3)


@pytest.mark.parametrize("name", ["per_channel", "per_row"])
def test_merger_golden_configs(name):
    from ovo_amd.entities.clips_merging import random_state_dict
    cfg, sd, x, _ = load_golden()[name]
    _check_merger(cfg, sd, x, name + " (golden rows)")
    gen = torch.Generator().manual_seed(3)
    xs = torch.nn.functional.normalize(torch.randn(32, 3, cfg["transformer"]["d_model"], generator=gen), dim=-1)
    sd2 = random_state_dict(cfg, seed=1, gain=GAIN)
    _check_merger(cfg, sd2, xs, name + " (B = 32, seeded)")


def test_merger_base_size(monkeypatch):
    """B = 32 (the dispatch that ships sends it to ovo_gemm), B = 16 (all six MLP layers on ovo_gemm_fewrows: bf16 hidden rows, f32 logits) and B = 16 with
    OVO_MERGER_NO_FEWROWS (ovo_gemm again), each against the same bound."""
    import yaml
    from ovo_amd.entities.clips_merging import FEWROWS_MAX_M, random_state_dict
    with open(os.path.join(GOLDEN, "weights_predictor_base_hparams.yaml")) as f:
        cfg = yaml.safe_load(f)["model"]
    sd = random_state_dict(cfg, seed=2, gain=GAIN)
    gen = torch.Generator().manual_seed(4)
    x = torch.nn.functional.normalize(torch.randn(32, 3, 1152, generator=gen), dim=-1)
    model, _ = _check_merger(cfg, sd, x, "base size (B = 32, seeded)")
    assert model.mlp_routes == ({"fewrows": 6, "gemm": 0} if 32 <= FEWROWS_MAX_M else {"fewrows": 0, "gemm": 6})
    assert FEWROWS_MAX_M >= 16
    _, few = _check_merger(cfg, sd, x[:16], "base size (B = 16, ovo_gemm_fewrows)", model)
    assert model.mlp_routes == {"fewrows": 6, "gemm": 0}
    monkeypatch.setenv("OVO_MERGER_NO_FEWROWS", "1")
    _, plain = _check_merger(cfg, sd, x[:16], "base size (B = 16, OVO_MERGER_NO_FEWROWS)", model)
    assert model.mlp_routes == {"fewrows": 0, "gemm": 6}
    monkeypatch.delenv("OVO_MERGER_NO_FEWROWS")
    _, forced = _check_merger(cfg, sd, x, "base size (B = 32, fewrows_max_m lifted)", type(model)(cfg, sd, device=DEV, fewrows_max_m=64))
    print(f"fewrows vs ovo_gemm route, B = 16: max abs {(few - plain).abs().max().item():.3e}")


def test_clip_generator_use_half_casts_only_the_learned_merge(tmp_path):
    from ovo_amd.entities.clip_generator import CLIPGenerator
    small = {"transformer": {"d_model": 1152, "dim_feedforward": 64, "n_layers": 1}, "mlp": {"act_key": "relu", "i_dim": 3456, "h_dim": 64, "n_layers": 0, "o_dim": 3}}
    import yaml
    with open(tmp_path / "hparams.yaml", "w") as f:
        yaml.safe_dump({"model": small}, f)
    gen_ = CLIPGenerator({"embed_type": "learned", "model_card": "SigLIP-384", "weights_predictor_path": str(tmp_path), "use_half": True})
    image = (torch.rand(3, 240, 320, generator=torch.Generator().manual_seed(1)) * 255).to(DEV)
    masks = torch.zeros(3, 240, 320, dtype=torch.bool, device=DEV)
    for i in range(3):
        masks[i, 20 + 30 * i:90 + 30 * i, 40 + 50 * i:130 + 50 * i] = True
    assert gen_.extract_clip(image, masks).dtype == torch.float16
    assert gen_.extract_clip(image, masks, return_all=True).dtype == torch.float32


def test_clip_generator_learned(tmp_path):
    from ovo_amd.entities.clip_generator import CLIPGenerator
    shutil.copyfile(os.path.join(GOLDEN, "weights_predictor_base_hparams.yaml"), tmp_path / "hparams.yaml")
    gen_ = CLIPGenerator({"embed_type": "learned", "model_card": "SigLIP-384", "weights_predictor_path": str(tmp_path)})
    g = torch.Generator().manual_seed(0)
    image = (torch.rand(3, 480, 640, generator=g) * 255).to(DEV)
    masks = torch.zeros(32, 480, 640, dtype=torch.bool, device=DEV)
    for i in range(32):
        y0, x0 = 10 + 12 * i, 15 + 17 * i
        masks[i, y0:y0 + 60 + i, x0:x0 + 50 + 2 * i] = True
    out = gen_.extract_clip(image, masks)
    triple = gen_.extract_clip(image, masks, return_all=True)
    assert out.shape == (32, 1152) and triple.shape == (32, 3, 1152) and out.dtype == torch.float32
    torch.testing.assert_close(out, gen_.clips_fusion_model(triple), atol=0, rtol=0)
    assert torch.allclose(out.norm(dim=-1), torch.ones(32, device=DEV), atol=1e-5)
    assert gen_.extract_clip(image, masks[:0]).shape == (0, 1152)
