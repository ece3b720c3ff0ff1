"""The learned crop-merging weights predictor on MI355X.

Mirror of the reference's `ovo/entities/clips_merging.py:WeightsPredictorMerger` (same constructor argument, `hparams["model"]`, same
`forward`, same state-dict key names): `n_layers` post-norm transformer encoder layers (ReLU feed-forward, LayerNorm eps 1e-5, eval mode)
over the three descriptors of a mask, an MLP on the flattened triple that predicts merge logits, softmax over the three clips, weighted
sum, L2 normalisation.

Weights are converted once to resident bf16 (biases and LayerNorm parameters f32); inputs and outputs are f32 on the device.  The
products of the MLP (one row per mask) run on `ovo_gemm_fewrows` up to `FEWROWS_MAX_M` rows and on `ovo_gemm` above, for shapes
`ovo_gemm_fewrows` does not take, and always with OVO_MERGER_NO_FEWROWS set; the encoder layers chain `ovo_gemm`, `ovo_attention_short`
and `ovo_layernorm`.  Output widths are padded with zero rows to a multiple of 32 so that every product fits the kernels' shape rules.

Offline limit, stated rather than hidden: without a state dict the module holds seeded random weights of the same architecture.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from .. import _lib as L

ACT_CODE = {"relu": 3, "sigmoid": 4, "leaky_relu": 6, "silu": 7}      # ovo_gemm_t.act; the keys of the reference's ACTIVATION_DICT
FEWROWS_MAX_M = 16           # rows per call up to which the MLP runs on ovo_gemm_fewrows: the measured crossover (a tie at 32, ovo_gemm ahead from 64)
LN_EPS = 1e-5


def _pad32(n: int) -> int:
    return (n + 31) // 32 * 32


def layer_shapes(config: Dict) -> Dict[str, List]:
    """(out, in) of every linear layer, as the reference module's state dict holds them; allocates nothing."""
    t, m = config["transformer"], config["mlp"]
    d, ff = t["d_model"], t["dim_feedforward"]
    enc = [("self_attn.in_proj", (3 * d, d)), ("self_attn.out_proj", (d, d)), ("linear1", (ff, d)), ("linear2", (d, ff))]
    mlp = [(m["h_dim"], m["i_dim"])] + [(m["h_dim"], m["h_dim"])] * m["n_layers"] + [(m["o_dim"], m["h_dim"])]
    return {"encoder_layer": enc, "n_encoder_layers": t["n_layers"], "mlp": mlp}


def random_state_dict(config: Dict, seed: int = 0, gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """Seeded weights under the reference module's key names: U(-b, b) with b = gain / sqrt(fan_in) for matrices and biases (nn.Linear's default
    at gain 1), LayerNorm at (1, 0)."""
    gen = torch.Generator().manual_seed(seed)
    sh = layer_shapes(config)
    d = config["transformer"]["d_model"]
    sd: Dict[str, torch.Tensor] = {}

    def lin(wkey, bkey, shape):
        b = gain / math.sqrt(shape[1])
        sd[wkey] = (torch.rand(shape, generator=gen) * 2 - 1) * b
        sd[bkey] = (torch.rand(shape[0], generator=gen) * 2 - 1) * b

    for i in range(sh["n_encoder_layers"]):
        p = f"att_encoder.layers.{i}."
        lin(p + "self_attn.in_proj_weight", p + "self_attn.in_proj_bias", (3 * d, d))
        lin(p + "self_attn.out_proj.weight", p + "self_attn.out_proj.bias", (d, d))
        lin(p + "linear1.weight", p + "linear1.bias", sh["encoder_layer"][2][1])
        lin(p + "linear2.weight", p + "linear2.bias", sh["encoder_layer"][3][1])
        for n in ("norm1", "norm2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = torch.ones(d), torch.zeros(d)
    for j, shape in enumerate(sh["mlp"]):
        lin(f"mlp.{2 * j}.weight", f"mlp.{2 * j}.bias", shape)
    return sd


class _Linear:
    """bf16 weight [pad32(out), k_pad] (zero rows / columns beyond the layer's own) + f32 bias, resident on the device."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, k_pad: int, device):
        n, k = weight.shape
        self.n, self.n_pad, self.k = n, _pad32(n), k_pad
        w = torch.zeros(self.n_pad, k_pad, dtype=torch.bfloat16, device=device)
        w[:n, :k] = weight.detach().to(device=device, dtype=torch.bfloat16)
        b = torch.zeros(self.n_pad, dtype=torch.float32, device=device)
        b[:n] = bias.detach().to(device=device, dtype=torch.float32)
        self.w, self.b = w, b


def _gemm(a: torch.Tensor, lin: _Linear, out_dtype: torch.dtype, act: int = 0, add: Optional[torch.Tensor] = None, fewrows: bool = False,
          routes: Optional[Dict[str, int]] = None) -> torch.Tensor:
    """One linear layer; `routes` counts the entry that actually ran it (ovo_gemm_fewrows declines with OVO_E_UNSUPPORTED, nothing launched)."""
    out = torch.empty(a.shape[0], lin.n_pad, dtype=out_dtype, device=a.device)
    g = L.gemm_desc(a, lin.w, out, bias=lin.b, add=add, act=act)
    lib = L.load()
    if fewrows:
        rc = lib.ovo_gemm_fewrows(L.C.byref(g), L.stream())
        if rc != L.E_UNSUPPORTED:
            L.check(rc)
            if routes is not None:
                routes["fewrows"] += 1
            return out
    L.check(lib.ovo_gemm(L.C.byref(g), L.stream()))
    if routes is not None:
        routes["gemm"] += 1
    return out


class WeightsPredictorMerger:
    def __init__(self, config: Dict, state_dict: Optional[Dict[str, torch.Tensor]] = None, device: Optional[str] = "cuda", seed: int = 0,
                 fewrows_max_m: int = FEWROWS_MAX_M):
        """`config` = hparams["model"].  device=None builds the shape description only (`layer_shapes`), allocating nothing.
        `fewrows_max_m`: rows per call up to which the MLP is offered to ovo_gemm_fewrows (tools/merger_bench.py raises it to measure the kernel at every M);
        `mlp_routes` counts, for the last call of `logits`, the MLP layers each entry actually ran."""
        self.config = config
        t, m = config["transformer"], config["mlp"]
        self.d, self.nhead, self.ff, self.n_layers = t["d_model"], t.get("nhead", 8), t["dim_feedforward"], t["n_layers"]
        self.act = ACT_CODE[m.get("act_key", "leaky_relu")]
        self.o_dim = m["o_dim"]
        if self.d % self.nhead or (self.d // self.nhead) % 8 or self.d % 32:
            raise ValueError("d_model must be a multiple of 32 and of 8 * nhead")
        if m["i_dim"] != 3 * self.d or self.o_dim not in (3, 3 * self.d):
            raise ValueError("mlp.i_dim must be 3 * d_model and mlp.o_dim 3 or 3 * d_model")
        self.layer_shapes = layer_shapes(config)
        self.device = device
        self.fewrows_max_m = fewrows_max_m
        self.mlp_routes = {"fewrows": 0, "gemm": 0}
        self.layers: List[Dict] = []
        self.mlp: List[_Linear] = []
        if device is not None:
            self.load_state_dict(state_dict if state_dict is not None else random_state_dict(config, seed))

    def eval(self):
        return self

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        dev, d = self.device, self.d
        f32 = lambda k: sd[k].detach().to(device=dev, dtype=torch.float32).contiguous()
        self.layers = []
        for i in range(self.n_layers):
            p = f"att_encoder.layers.{i}."
            lin1 = _Linear(sd[p + "linear1.weight"], sd[p + "linear1.bias"], d, dev)
            self.layers.append({
                "qkv": _Linear(sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"], d, dev),
                "out": _Linear(sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], d, dev),
                "fc1": lin1, "fc2": _Linear(sd[p + "linear2.weight"], sd[p + "linear2.bias"], lin1.n_pad, dev),
                "n1": (f32(p + "norm1.weight"), f32(p + "norm1.bias")), "n2": (f32(p + "norm2.weight"), f32(p + "norm2.bias"))})
        self.mlp, k = [], 3 * d
        for j in range(len(self.layer_shapes["mlp"])):
            self.mlp.append(_Linear(sd[f"mlp.{2 * j}.weight"], sd[f"mlp.{2 * j}.bias"], k, dev))
            k = self.mlp[-1].n_pad

    def weight_bytes(self) -> int:
        return sum(l.w.numel() * 2 for l in self.mlp)

    def _ln(self, x: torch.Tensor, gb) -> torch.Tensor:
        y = torch.empty_like(x)
        L.check(L.load().ovo_layernorm(L.ptr(x), x.shape[1], x.shape[0], x.shape[1], L.ptr(gb[0]), L.ptr(gb[1]), LN_EPS, L.ptr(y), x.shape[1], 0, L.stream()))
        return y

    @staticmethod
    def _bf16(x: torch.Tensor) -> torch.Tensor:
        y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        L.check(L.load().ovo_cast_f32(L.ptr(x), x.numel(), L.ptr(y), 2, L.stream()))
        return y

    @torch.no_grad()
    def logits(self, input_clips: torch.Tensor) -> torch.Tensor:
        """f32 [B, pad32(o_dim)]: the MLP's output (columns >= o_dim are padding)."""
        b, d, lib = input_clips.shape[0], self.d, L.load()
        x = L.dev(input_clips.float().contiguous(), torch.float32, "input_clips").reshape(3 * b, d)
        for ly in self.layers:
            qkv = _gemm(self._bf16(x), ly["qkv"], torch.bfloat16)
            att = torch.empty(3 * b, d, dtype=torch.bfloat16, device=x.device)
            L.check(lib.ovo_attention_short(L.ptr(qkv), b, 3, self.nhead, d // self.nhead, 1.0 / math.sqrt(d // self.nhead), L.ptr(att), L.stream()))
            x = self._ln(_gemm(att, ly["out"], torch.float32, add=x), ly["n1"])
            h = _gemm(self._bf16(x), ly["fc1"], torch.bfloat16, act=3)
            x = self._ln(_gemm(h, ly["fc2"], torch.float32, add=x), ly["n2"])
        few = b <= self.fewrows_max_m     # OVO_MERGER_NO_FEWROWS (read by the library) turns every such call into ovo_gemm
        h = self._bf16(x).reshape(b, 3 * d)
        self.mlp_routes = {"fewrows": 0, "gemm": 0}
        for j, lin in enumerate(self.mlp):
            last = j == len(self.mlp) - 1
            h = _gemm(h, lin, torch.float32 if last else torch.bfloat16, act=0 if last else self.act, fewrows=few, routes=self.mlp_routes)
        return h

    @torch.no_grad()
    def forward(self, input_clips: torch.Tensor) -> torch.Tensor:
        """input_clips [B, 3, d_model] on the device -> merged, unit-norm f32 [B, d_model] (clips_merging.py:39-56)."""
        b, n_clips, d = input_clips.shape
        if n_clips != 3 or d != self.d:
            raise ValueError(f"input_clips must be [B, 3, {self.d}]")
        out = torch.empty(b, d, dtype=torch.float32, device=input_clips.device)
        if b == 0:
            return out
        clips = L.dev(input_clips.float().contiguous(), torch.float32, "input_clips")
        lg = self.logits(clips)
        L.check(L.load().ovo_merge_clips(L.ptr(lg), lg.shape[1], 1 if self.o_dim == 3 else 0, L.ptr(clips), b, d, L.ptr(out), L.stream()))
        return out

    __call__ = forward
