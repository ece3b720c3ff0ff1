"""WeightsPredictorMerger.forward restated from the published formulas in explicit tensor ops (no nn.Module): post-norm transformer encoder
layers (multi-head self-attention over the three clips, ReLU feed-forward, LayerNorm eps 1e-5, no dropout), the MLP on the flattened triple,
softmax over the clips, weighted sum, L2 normalisation.  `rnd` is applied to every weight matrix and to the input of every product (the
linear layers and the attention's q, k, v): identity = the fp32 restatement; a bf16 round trip = the number format's own floor."""
import math

import torch

ACTS = {"relu": torch.relu, "sigmoid": torch.sigmoid, "leaky_relu": lambda v: torch.where(v > 0, v, 0.01 * v), "silu": lambda v: v * torch.sigmoid(v)}


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def merge(logits, clips, o_dim):
    b, n, d = clips.shape
    w = torch.softmax(logits.reshape(b, n, d), dim=1) if o_dim != 3 else torch.softmax(logits, dim=-1)[..., None]
    y = (clips * w).sum(1)
    return y / y.norm(dim=-1, keepdim=True).clamp_min(1e-12), w


def forward(sd, config, clips, rnd=lambda t: t, want_weights=False):
    t, m = config["transformer"], config["mlp"]
    d, nh = t["d_model"], t.get("nhead", 8)
    hd = d // nh
    lin = lambda x, w, b: rnd(x) @ rnd(sd[w]).T + sd[b]
    bsz = clips.shape[0]
    x = clips
    for i in range(t["n_layers"]):
        p = f"att_encoder.layers.{i}."
        qkv = rnd(lin(x, p + "self_attn.in_proj_weight", p + "self_attn.in_proj_bias")).reshape(bsz, 3, 3, nh, hd)      # [B, T, (q k v), H, hd]
        q, k, v = (qkv[:, :, j].permute(0, 2, 1, 3) for j in range(3))                                               # [B, H, T, hd]
        att = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1) @ v
        att = att.permute(0, 2, 1, 3).reshape(bsz, 3, d)
        x = layer_norm(x + lin(att, p + "self_attn.out_proj.weight", p + "self_attn.out_proj.bias"), sd[p + "norm1.weight"], sd[p + "norm1.bias"])
        h = torch.relu(lin(x, p + "linear1.weight", p + "linear1.bias"))
        x = layer_norm(x + lin(h, p + "linear2.weight", p + "linear2.bias"), sd[p + "norm2.weight"], sd[p + "norm2.bias"])
    h = x.reshape(bsz, 3 * d)
    n_lin = m["n_layers"] + 2
    for j in range(n_lin):
        h = lin(h, f"mlp.{2 * j}.weight", f"mlp.{2 * j}.bias")
        if j < n_lin - 1:
            h = ACTS[m.get("act_key", "leaky_relu")](h)
    y, w = merge(h, clips, m["o_dim"])
    return (y, w) if want_weights else y
