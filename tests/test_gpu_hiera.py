"""-m gpu: SAM2 image encoder (Hiera + FPN) on the GPU vs the fp32 oracle and HuggingFace golden vectors.

bf16 operands, fp32 accumulation and residual stream: errors are reported relative to the feature RMS.
"""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return ((a - b).abs().max() / b.pow(2).mean().sqrt()).item()


def _rel_rms(a: torch.Tensor, b: torch.Tensor) -> float:
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


# Measured on MI355X (profiles/r03*_pytest_gpu.txt): per card, max |error| / rms over the three FPN levels and rms(error) / rms.  The maximum
# over 1-4 M elements of a bf16-operand pipeline sits 5-6 sigma out (rms error 4-7e-3: ~2^-9 per GEMM operand through 12-48 blocks), so the
# MAX bound is a statistic of the tail, the RMS bound is the one that moves when a kernel loses precision.  Bounds = 1.5 x measured.
_HIERA_BOUNDS = {"hiera_test": (0.06, 0.012), "hiera_b+": (0.06, 0.012), "hiera_t": (0.06, 0.012), "hiera_l": (0.075, 0.015)}


def test_hiera_vs_hf_golden():
    from oracle import hiera as OH
    from ovo_amd.encoders.hiera import HieraSpec, HipHiera
    d = golden("hf_sam2_hiera")
    sd = OH.hf_sam2_to_sam2({k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w:")})
    spec = HieraSpec("hf-golden", 16, 1, tuple(d["stages"].tolist()), tuple(d["global_blocks"].tolist()),
                     tuple(d["window_spec"].tolist()), (5, 5), image_size=128, fpn_dim=32, hi_res=False)
    enc = HipHiera(spec, sd, device=DEV)
    feats = enc.forward(torch.from_numpy(d["x"]).to(DEV))
    for i, f in enumerate(feats):
        ref = torch.from_numpy(d[f"fpn{i}"]).permute(0, 2, 3, 1)
        assert f.shape == ref.shape
        r = _rel(f.cpu(), ref)
        print(f"level {i}: max err / rms = {r:.3e}")
        assert r < 0.08


@pytest.mark.parametrize("card,batch", [("hiera_test", 2), ("hiera_b+", 1), ("hiera_t", 1), ("hiera_l", 1)])
def test_hiera_vs_oracle(card, batch):
    """Every SAM2 trunk the reference can select (segment_utils.py:274: hiera_l -- its default, ovo.yaml:35 -- and hiera_t) and
    BASELINE.json's hiera_b+, at 1024^2, against the fp32 oracle; hiera_l's window spec (8, 4, 16, 8) and 48 blocks exercise window /
    un-window shapes the others do not."""
    from oracle import hiera as OH
    from ovo_amd.encoders.hiera import SPECS, HipHiera, random_state
    spec = SPECS[card]
    sd = random_state(spec, seed=5)
    enc = HipHiera(spec, sd, device=DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 3, spec.image_size, spec.image_size, generator=g)
    ref = OH.hiera_forward(sd, x, stages=spec.stages, heads=spec.heads, window_spec=spec.window_spec,
                           global_blocks=spec.global_blocks, hi_res=True)
    out = enc.forward(x.to(DEV))
    for i, (f, r) in enumerate(zip(out, ref)):
        assert f.shape == r.shape, (f.shape, r.shape)
        e, er = _rel(f.cpu(), r), _rel_rms(f.cpu(), r)
        cos = torch.nn.functional.cosine_similarity(f.cpu().flatten(), r.flatten(), dim=0).item()
        print(f"{card} level {i} {tuple(f.shape)}: max err / rms = {e:.3e}, rms err / rms = {er:.3e}, cosine = {cos:.6f}")
        b_max, b_rms = _HIERA_BOUNDS[card]
        assert e < b_max and er < b_rms and cos > 0.9999


@pytest.mark.parametrize("card", ["hiera_b+", "hiera_l"])
def test_layernorm_in_the_operand_load_vs_separate_pass(card, monkeypatch):
    """Stages 1-2 (and their FPN laterals, conv_s0 / conv_s1) take LayerNorm / the bf16 cast inside the streaming GEMM's A-operand load
    (gemm_stream.hip, F32A) instead of a k_ln_window / k_cast_pad pass: same formula, the row statistics summed in another order.  A bf16
    activation that rounds the other way re-rolls the roundings of everything downstream, so the two forwards differ by a fraction of the
    rounding noise both carry against the fp32 oracle (rms 1e-3 of the feature rms between them; 5-7e-3 each against the oracle, whose
    bounds both meet: test_hiera_vs_oracle runs the fused path) -- measured max 2.0e-2 / rms 1.1e-3 at the stage-1 level, 1.9e-2 / 3.6e-3 behind
    stage 3's sixteen blocks.  The operation itself is pinned one layer at a time in test_gemm_with_layernorm_in_the_operand_load."""
    from ovo_amd.encoders.hiera import SPECS, HipHiera, random_state
    spec = SPECS[card]
    enc = HipHiera(spec, random_state(spec, seed=5), device=DEV)
    x = torch.randn(1, 3, spec.image_size, spec.image_size, generator=torch.Generator().manual_seed(2)).to(DEV)
    fused = [t.clone() for t in enc.forward(x)]
    monkeypatch.setenv("OVO_NO_LN_FOLD", "1")
    plain = [t.clone() for t in enc.forward(x)]
    diff = 0.0
    for i, (a, b) in enumerate(zip(fused, plain)):
        e, er = _rel(a, b), _rel_rms(a, b)
        print(f"{card} level {i}: fused vs separate LayerNorm pass: max / rms = {e:.3e}, rms / rms = {er:.3e}")
        assert e < 0.05 and er < 6e-3
        diff = max(diff, e)
    assert diff > 0.0, "the fused path did not run (identical bits)"


def test_hiera_preprocess_matches_torch():
    from oracle import vit as OV
    from ovo_amd.encoders.hiera import IMAGENET_MEAN, IMAGENET_STD, SPECS, HipHiera
    enc = object.__new__(HipHiera)
    enc.spec, enc.device = SPECS["hiera_b+"], torch.device(DEV)
    img = (torch.rand(3, 480, 640, generator=torch.Generator().manual_seed(0)) * 255).to(torch.uint8)
    got = HipHiera.preprocess(enc, img.to(DEV))[0].cpu()
    ref = OV.resize_normalize(img, 1024, IMAGENET_MEAN, IMAGENET_STD, None, scale=1 / 255.0, antialias=True)
    torch.testing.assert_close(got, ref, atol=3e-5, rtol=1e-5)


@pytest.mark.parametrize("card", ["hiera_b+", "hiera_t"])
def test_flops_accounting_matches_the_launched_work(card):
    """`HieraSpec.flops_per_image()` (bench.py's gflop_per_frame / frame_frac) against the sum of 2MNK / 4BHTqTk.hd over the GEMM and
    attention launches of one real forward (the library's hipEvent profiler records the shape of every launch)."""
    import ctypes as C
    from ovo_amd import _lib as L
    from ovo_amd.encoders.hiera import SPECS, HipHiera
    spec = SPECS[card]
    enc = HipHiera(spec, None, device=DEV, seed=1)
    x = torch.zeros(1, 3, spec.image_size, spec.image_size, device=DEV)
    enc.forward(x)
    lib = L.load()
    L.check(lib.ovo_profile_start())
    enc.forward(x)
    ms, work, n = (C.c_double * 9)(), (C.c_double * 9)(), (C.c_int64 * 9)()
    L.check(lib.ovo_profile_stop(ms, work, n, 9))
    launched = work[1] + sum(work[k] for k in (0, 3, 4, 5, 6, 7, 8))            # attention + every GEMM family (tiled, ping-pong, streaming)
    model = spec.flops_per_image()
    print(f"{card}: launched {launched / 1e9:.1f} GFLOP, flops_per_image {model / 1e9:.1f} GFLOP")
    assert abs(launched - model) / model < 0.03


@pytest.mark.parametrize("E,S,B", [(112, 1024, 2), (96, 256, 3), (144, 128, 1)])
def test_patch_embed_direct_conv_vs_torch(E, S, B):
    """`ovo_hiera_patch_embed` (round 5: the 7 x 7 / stride-4 patch convolution straight from the f32 image, bias and position embedding in its
    epilogue) against torch's fp32 Conv2d on the same bf16-rounded image and weights: the products are exact in f32, only the summation order
    differs -> 1e-5 of the output scale.  Edge tiles (zero padding on all four sides) are part of every case."""
    import ctypes as C
    from ovo_amd import _lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(E + S)
    img = torch.randn(B, 3, S, S, generator=g)
    w = torch.randn(E, 3, 7, 7, generator=g) * 0.05
    bias, pos = torch.randn(E, generator=g), torch.randn((S // 4) ** 2, E, generator=g)
    wp = torch.zeros(E, 192)
    wp[:, :147] = w.reshape(E, -1)
    d_img, d_w, d_b, d_p = img.to(DEV), wp.to(torch.bfloat16).to(DEV), bias.to(DEV), pos.to(DEV)
    out = torch.empty(B, (S // 4) ** 2, E, device=DEV)
    L.check(lib.ovo_hiera_patch_embed(L.ptr(d_img), B, S, E, L.ptr(d_w), 192, L.ptr(d_b), L.ptr(d_p), L.ptr(out), L.stream()))
    ref = torch.nn.functional.conv2d(img.to(torch.bfloat16).float(), w.to(torch.bfloat16).float(), bias, stride=4, padding=3)
    ref = ref.permute(0, 2, 3, 1).reshape(B, -1, E) + pos[None]
    err = (out.cpu() - ref).abs().max().item()
    print(f"E={E} S={S} B={B}: max |err| = {err:.3e} (output rms {ref.pow(2).mean().sqrt():.2f})")
    assert err < 2e-5 * ref.abs().max().item()


def test_patch_embed_direct_equals_im2col_gemm_forward(monkeypatch):
    """The whole hiera_b+ forward with the direct patch convolution against the im2col + GEMM form (OVO_HIERA_PATCH_GEMM=1): the first layer's
    f32 sums differ in their last bit or two, which re-rolls a few bf16 roundings downstream -- inside the noise both carry against the oracle
    (measured rms difference / rms 1.4-1.8e-3 at the stage-1 level, 3.6-3.8e-3 behind stage 3's sixteen blocks; each is 5-7e-3 from the oracle)."""
    from ovo_amd.encoders.hiera import SPECS, HipHiera, random_state
    spec = SPECS["hiera_b+"]
    enc = HipHiera(spec, random_state(spec, seed=5), device=DEV)
    x = torch.randn(1, 3, spec.image_size, spec.image_size, generator=torch.Generator().manual_seed(2)).to(DEV)
    a = [f.clone() for f in enc.forward(x)]
    monkeypatch.setenv("OVO_HIERA_PATCH_GEMM", "1")
    b = [f.clone() for f in enc.forward(x)]
    for i, (u, v) in enumerate(zip(a, b)):
        er = _rel_rms(u.cpu(), v.cpu())
        print(f"level {i}: rms difference / rms = {er:.3e}")
        assert er < 8e-3


@pytest.mark.parametrize("case", ["stage1", "stage_change", "stage2"])
def test_window_attention_fused_vs_torch(case):
    """`ovo_window_attention_f32` (round 5: LayerNorm -> QKV -> window attention of a Hiera block in one launch per pair of heads, q | k | v in
    registers; "stage_change": 4 heads, queries 2 x 2 max-pooled inside the 8 x 8 window; "stage2": 224 channels, 4 heads, 4 x 4 windows) against torch
    with the kernel's rounding points (LayerNorm output, q | k | v, the softmax numerators and the output in bf16; f32 sums).  What is left is summation
    order and the rounding of values that sit on a bf16 boundary: measured max 2.5e-2 / rms 2e-4 of the output rms."""
    import math
    from ovo_amd import _lib as L
    lib = L.load()
    HD = 56
    B, H, W, C, CO, NH, ws, pool = {"stage1": (2, 256, 256, 112, 112, 2, 8, 0), "stage_change": (2, 256, 256, 112, 224, 4, 8, 1),
                                    "stage2": (2, 128, 128, 224, 224, 4, 4, 0)}[case]
    kp = 128 if C == 112 else 256
    g = torch.Generator().manual_seed(3 + len(case))
    x = (torch.randn(B, H, W, C, generator=g) * 1.5 + 0.3)
    ln_g, ln_b = 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    w = torch.randn(3 * CO, C, generator=g) * (C ** -0.5)
    bias = 0.2 * torch.randn(3 * CO, generator=g)
    w[:CO] *= math.log2(math.e) / math.sqrt(HD)                  # the q rows carry log2(e) / sqrt(head_dim)
    bias[:CO] *= math.log2(math.e) / math.sqrt(HD)
    wp = torch.zeros(3 * CO, kp)
    wp[:, :C] = w
    w16 = wp.to(torch.bfloat16)
    n_win, tk, ld = B * (H // ws) * (W // ws), ws * ws, 256
    tq = tk // 4 if pool else tk
    att = torch.full((n_win * tq, ld), 7.0, dtype=torch.bfloat16, device=DEV)
    d = [t.to(DEV) for t in (x, ln_g, ln_b, w16, bias)]
    L.check(lib.ovo_window_attention_f32(L.ptr(d[0]), B, H, W, ws, C, CO, NH, pool, L.ptr(d[1]), L.ptr(d[2]), 1e-6, L.ptr(d[3]), kp, L.ptr(d[4]), L.ptr(att),
                                         ld, L.stream()))
    out = att.float().cpu()
    assert (out[:, CO:] == 7.0).all()                            # the padding columns are not touched
    r16 = lambda t: t.to(torch.bfloat16).float()
    xn = r16(torch.nn.functional.layer_norm(x, (C,), ln_g, ln_b, 1e-6))
    xw = xn.reshape(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(n_win, tk, C)
    qkv = r16(xw @ w16[:, :C].float().T + bias).reshape(n_win, tk, 3, NH, HD)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))           # [n_win, NH, tk, HD]
    if pool:                                                     # 2 x 2 max-pool of q over the window's 8 x 8 tokens (sam2 do_pool on q)
        q = q.reshape(n_win, NH, 4, 2, 4, 2, HD).amax(dim=(3, 5)).reshape(n_win, NH, 16, HD)
    s = q @ k.transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    ref = r16((r16(p) @ v) / p.sum(-1, keepdim=True)).permute(0, 2, 1, 3).reshape(n_win * tq, CO)
    err = (out[:, :CO] - ref).abs()
    rms = ref.pow(2).mean().sqrt().item()
    print(f"{case}: max |err| / rms = {err.max().item() / rms:.3e}, rms err / rms = {err.pow(2).mean().sqrt().item() / rms:.3e}")
    # (the maximum is a handful of values whose inputs sat on a bf16 rounding boundary -- q, k, v or a softmax numerator one step apart; the rms is the
    # bound that moves when something is wrong: measured 2.0-2.2e-4)
    assert err.max().item() < 8e-2 * rms and err.pow(2).mean().sqrt().item() < 1e-3 * rms


def test_window_attention_fused_equals_three_launch_forward(monkeypatch):
    """The whole hiera_b+ forward (batch 2) with the fused attention of stage 1 and of the stage-change block against the three-launch form
    (OVO_HIERA_NO_WINATTN=1): same rounding points, other summation orders -- a fraction of the noise both carry against the oracle."""
    from ovo_amd.encoders.hiera import SPECS, HipHiera, random_state
    spec = SPECS["hiera_b+"]
    enc = HipHiera(spec, random_state(spec, seed=5), device=DEV)
    x = torch.randn(2, 3, spec.image_size, spec.image_size, generator=torch.Generator().manual_seed(2)).to(DEV)
    a = [f.clone() for f in enc.forward(x)]
    monkeypatch.setenv("OVO_HIERA_NO_WINATTN", "1")
    b = [f.clone() for f in enc.forward(x)]
    for i, (u, v) in enumerate(zip(a, b)):
        er = _rel_rms(u.cpu(), v.cpu())
        print(f"level {i}: rms difference / rms = {er:.3e}")
        assert 0 < er < 8e-3


def test_fused_hiera_kernels_are_deterministic():
    """The fused stage-1/2 kernels at the bench's full 12-frame size, launched repeatedly: every output bit-identical to the first launch (the fused
    MLP kernel once had a two-workgroup form that was not, `test_fused_mlp_stream_is_deterministic`; these kernels have no cross-wave hand-over after
    the weights are in LDS, and this test holds them to it)."""
    from ovo_amd import _lib as L
    lib = L.load()
    B = 12
    g = torch.Generator().manual_seed(11)
    for (H, C, CO, NH, ws, pool, kp) in ((256, 112, 112, 2, 8, 0, 128), (256, 112, 224, 4, 8, 1, 128), (128, 224, 224, 4, 4, 0, 256)):
        x = torch.randn(B, H, H, C, generator=g).to(DEV)
        ln_g, ln_b = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        w = torch.zeros(3 * CO, kp)
        w[:, :C] = torch.randn(3 * CO, C, generator=g) * 0.1
        w16, bias = w.to(torch.bfloat16).to(DEV), (0.1 * torch.randn(3 * CO, generator=g)).to(DEV)
        n_win, tq = B * (H // ws) ** 2, (ws * ws // 4 if pool else ws * ws)
        outs = []
        for rep in range(20):
            att = torch.zeros((n_win * tq, 256), dtype=torch.bfloat16, device=DEV)
            L.check(lib.ovo_window_attention_f32(L.ptr(x), B, H, H, ws, C, CO, NH, pool, L.ptr(ln_g), L.ptr(ln_b), 1e-6, L.ptr(w16), kp, L.ptr(bias), L.ptr(att),
                                                 256, L.stream()))
            outs.append(att)
        torch.cuda.synchronize()
        bad = sum(int(not torch.equal(outs[0], o)) for o in outs[1:])
        assert bad == 0, f"window attention ({C} -> {CO}, pool {pool}): {bad} of 19 repeats differ"
    S, E = 1024, 112
    img = torch.randn(B, 3, S, S, generator=g).to(DEV)
    wp = torch.zeros(E, 192)
    wp[:, :147] = torch.randn(E, 147, generator=g) * 0.05
    d_w, d_b, d_p = wp.to(torch.bfloat16).to(DEV), torch.randn(E, generator=g).to(DEV), torch.randn((S // 4) ** 2, E, generator=g).to(DEV)
    outs = []
    for rep in range(6):
        out = torch.empty(B, (S // 4) ** 2, E, device=DEV)
        L.check(lib.ovo_hiera_patch_embed(L.ptr(img), B, S, E, L.ptr(d_w), 192, L.ptr(d_b), L.ptr(d_p), L.ptr(out), L.stream()))
        outs.append(out)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])


@pytest.mark.parametrize("windowed", [True, False])
def test_projection_with_rowwise_layernorm_vs_torch(windowed):
    """`ovo_gemm_rowln` (round 5: Hiera stage 3's attention output projection + residual on a full-row tile, the block's norm2 taken from the accumulators):
    C against torch's f32 product of the same bf16 operands (summation order only) and ln_out against LayerNorm of the C the kernel itself wrote (the
    statistics' summation order and one bf16 rounding)."""
    import ctypes as C
    from ovo_amd import _lib as L
    lib = L.load()
    B, H, ws, N, K = 2, 64, 14, 448, 448
    g = torch.Generator().manual_seed(9)
    nw = -(-H // ws)
    M = B * nw * nw * ws * ws if windowed else B * H * H
    A = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    bias, x = torch.randn(N, generator=g) * 0.1, torch.randn(B * H * H, N, generator=g)
    ln_g, ln_b = 1.0 + 0.2 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    d_A, d_W, d_bias, d_x, d_g, d_b = (t.to(DEV) for t in (A, W, bias, x.clone(), ln_g, ln_b))
    h = torch.full((B * H * H, N), 7.0, dtype=torch.bfloat16, device=DEV)
    q = L.gemm_desc(d_A, d_W, d_x, bias=d_bias, add=d_x, ldc=N)      # (windowed: d_x holds the spatial rows, fewer than M)
    win = L.Window(B, H, H, ws, ws) if windowed else None
    L.check(lib.ovo_gemm_rowln(C.byref(q), C.byref(win) if windowed else None, L.ptr(d_g), L.ptr(d_b), 1e-6, L.ptr(h), N, L.stream()))
    prod = A.float() @ W.float().T + bias
    if windowed:                                                 # window-major product rows -> spatial rows; padding positions dropped
        prod = prod.reshape(B, nw, nw, ws, ws, N).permute(0, 1, 3, 2, 4, 5).reshape(B, nw * ws, nw * ws, N)[:, :H, :H].reshape(B * H * H, N)
    ref = x + prod
    out = d_x.cpu()
    err = (out - ref).abs().max().item()
    ln_ref = torch.nn.functional.layer_norm(out, (N,), ln_g, ln_b, 1e-6)
    e_ln = (h.float().cpu() - ln_ref).abs()
    print(f"windowed={windowed}: C max |err| {err:.2e}; LN max |err| {e_ln.max().item():.2e} (one bf16 step at |y| ~ 4 is 1.6e-2)")
    assert err < 2e-5 * ref.abs().max().item() + 1e-5
    assert (e_ln <= 2.0 ** -8 * ln_ref.abs() + 1e-4).all()


def test_forward_with_the_rowwise_layernorm_projection(monkeypatch):
    """The opt-in stage-3 form (OVO_HIERA_PROJ_LN=1: projection + residual + norm2 on the full-row tile) against the default forward: the same values
    up to the statistics' summation order."""
    from ovo_amd.encoders.hiera import SPECS, HipHiera, random_state
    spec = SPECS["hiera_b+"]
    enc = HipHiera(spec, random_state(spec, seed=5), device=DEV)
    x = torch.randn(1, 3, spec.image_size, spec.image_size, generator=torch.Generator().manual_seed(2)).to(DEV)
    a = [f.clone() for f in enc.forward(x)]
    monkeypatch.setenv("OVO_HIERA_PROJ_LN", "1")
    b = [f.clone() for f in enc.forward(x)]
    for i, (u, v) in enumerate(zip(a, b)):
        er = _rel_rms(u.cpu(), v.cpu())
        print(f"level {i}: rms difference / rms = {er:.3e}")
        assert er < 8e-3
    assert _rel_rms(a[2].cpu(), b[2].cpu()) > 0                  # (the knob took effect: stage 3 feeds level 2)
