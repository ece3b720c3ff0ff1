"""SAM2 prompt encoder (point prompts) + mask decoder on MI355X.

The reference reaches this through the un-vendored `sam2` package: `SAM2AutomaticMaskGenerator.generate` prompts the
decoder with a regular grid of foreground clicks (segment_utils.py:291-308, mask_generator.py:113).  Here every prompt of
the grid is decoded in ONE batch: the token side ([P*8, 256]) and the image side ([P*4096, 256]) of the two-way
transformer are plain row-major matrices, all products run on `ovo_gemm` / `ovo_attention`, and the passes between them
(residual, LayerNorm, "+ positional code", casts, the two transposed convolutions, the hyper-network product) are the
three kernels of csrc/samdec.hip.  State-dict names follow the sam2 repository, like `oracle/sam2_decoder.py`.

What is shared between prompts is computed once: the keys of the first layer (identical for every prompt until the first
image->token update) are projected for a single prompt and broadcast through a zero batch stride; the point tokens of a
fixed prompt grid and the dense positional code are constants of the generator, built at set-up.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from .. import _lib as L

import os
# The per-prompt keys [P * S, C] between the two-way layers are kept in bf16 only: the tensor every product reads is bf16 anyway, and reading it
# back as the residual instead of a second f32 copy saves 1.6 GB of traffic per layer at 256 prompts.  The reference runs the decoder under bf16
# autocast (mask_generator.py:46,112: every nn.Linear output is bf16 there); measured against the fp32 oracle the mask-logit error is unchanged
# (max err / rms 4.1e-2 -> 4.0e-2, tests/test_gpu_sam_decoder.py).  OVO_SAM_RES16=0 keeps the f32 residual stream.
RES16 = os.environ.get("OVO_SAM_RES16", "1") == "1"
PE = "sam_prompt_encoder."
MD = "sam_mask_decoder."


@dataclass(frozen=True)
class SamDecoderSpec:
    name: str
    hidden: int = 256
    heads: int = 8
    mlp_dim: int = 2048
    depth: int = 2
    n_mask_tokens: int = 4
    embed_size: int = 64            # side of the image embedding grid
    image_size: int = 1024          # side of the model input the prompts are expressed in
    iou_hidden: int = 256


SPECS: Dict[str, SamDecoderSpec] = {
    "sam2": SamDecoderSpec("sam2"),
    "sam2_small": SamDecoderSpec("sam2_small", mlp_dim=512, embed_size=16, image_size=256),      # real widths, 256^2 input
    "sam2_test": SamDecoderSpec("sam2_test", hidden=128, heads=4, mlp_dim=256, embed_size=16, image_size=256, iou_hidden=128),
}


def random_state(spec: SamDecoderSpec, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded random weights with the sam2 repository's parameter names (there are no checkpoints offline)."""
    g = torch.Generator().manual_seed(seed)
    c, ci = spec.hidden, spec.hidden // 2
    sd: Dict[str, torch.Tensor] = {}

    def lin(name, out, inp):
        sd[name + ".weight"] = torch.randn(out, inp, generator=g) * inp ** -0.5
        sd[name + ".bias"] = torch.randn(out, generator=g) * 0.05

    def norm(name, n):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn(n, generator=g)
        sd[name + ".bias"] = 0.1 * torch.randn(n, generator=g)

    def attn(name, inner):
        for p, (o, i) in (("q_proj", (inner, c)), ("k_proj", (inner, c)), ("v_proj", (inner, c)), ("out_proj", (c, inner))):
            lin(f"{name}.{p}", o, i)

    sd[PE + "pe_layer.positional_encoding_gaussian_matrix"] = torch.randn(2, c // 2, generator=g)
    for i in range(4):
        sd[PE + f"point_embeddings.{i}.weight"] = torch.randn(1, c, generator=g) * 0.5
    sd[PE + "not_a_point_embed.weight"] = torch.randn(1, c, generator=g) * 0.5
    sd[PE + "no_mask_embed.weight"] = torch.randn(1, c, generator=g) * 0.5
    sd["no_mem_embed"] = torch.randn(1, 1, c, generator=g) * 0.1
    for n in ("obj_score_token", "iou_token"):
        sd[MD + n + ".weight"] = torch.randn(1, c, generator=g) * 0.5
    sd[MD + "mask_tokens.weight"] = torch.randn(spec.n_mask_tokens, c, generator=g) * 0.5
    t = MD + "transformer."
    for i in range(spec.depth):
        b = t + f"layers.{i}."
        attn(b + "self_attn", c)
        attn(b + "cross_attn_token_to_image", ci)
        attn(b + "cross_attn_image_to_token", ci)
        lin(b + "mlp.layers.0", spec.mlp_dim, c)
        lin(b + "mlp.layers.1", c, spec.mlp_dim)
        for k in range(1, 5):
            norm(b + f"norm{k}", c)
    attn(t + "final_attn_token_to_image", ci)
    norm(t + "norm_final_attn", c)
    sd[MD + "output_upscaling.0.weight"] = torch.randn(c, c // 4, 2, 2, generator=g) * c ** -0.5
    sd[MD + "output_upscaling.0.bias"] = torch.randn(c // 4, generator=g) * 0.05
    norm(MD + "output_upscaling.1", c // 4)
    sd[MD + "output_upscaling.3.weight"] = torch.randn(c // 4, c // 8, 2, 2, generator=g) * (c // 4) ** -0.5
    sd[MD + "output_upscaling.3.bias"] = torch.randn(c // 8, generator=g) * 0.05
    for i in range(spec.n_mask_tokens):
        m = MD + f"output_hypernetworks_mlps.{i}."
        lin(m + "layers.0", c, c); lin(m + "layers.1", c, c); lin(m + "layers.2", c // 8, c)
    lin(MD + "iou_prediction_head.layers.0", spec.iou_hidden, c)
    lin(MD + "iou_prediction_head.layers.1", spec.iou_hidden, spec.iou_hidden)
    lin(MD + "iou_prediction_head.layers.2", spec.n_mask_tokens, spec.iou_hidden)
    lin(MD + "pred_obj_score_head.layers.0", c, c); lin(MD + "pred_obj_score_head.layers.1", c, c); lin(MD + "pred_obj_score_head.layers.2", 1, c)
    return sd


def fourier_pe(coords01: torch.Tensor, gauss: torch.Tensor) -> torch.Tensor:
    """[..., 2] (x, y) in [0, 1] -> [sin | cos](2 pi (2c - 1) G): SAM's random-Fourier positional code (set-up time only)."""
    c = 2.0 * math.pi * ((2.0 * coords01 - 1.0) @ gauss)
    return torch.cat([torch.sin(c), torch.cos(c)], dim=-1)


def point_grid(n_per_side: int) -> torch.Tensor:
    """The regular prompt grid of the automatic mask generator, in [0, 1]^2 (x, y), row-major -> [n*n, 2]."""
    off = 1.0 / (2 * n_per_side)
    t = torch.linspace(off, 1.0 - off, n_per_side, dtype=torch.float64)
    yy, xx = torch.meshgrid(t, t, indexing="ij")
    return torch.stack([xx, yy], dim=-1).reshape(-1, 2)


class _Tokens(NamedTuple):
    """The token side of one forward, [P * T, C] each: the f32 residual stream, its bf16 copy, the bf16 copy with the prompts' positional code (the
    tokens as given) added, and where the self-attention leaves its output.  Every step overwrites them in place."""
    q: torch.Tensor
    q16: torch.Tensor
    qpe16: torch.Tensor
    attn_out: torch.Tensor


class _KeyUpdate(NamedTuple):
    """Operands of one image -> token key update, keys' = LayerNorm(residual[row % res_rows] + out-projection); its bf16 outputs are the stream's
    `k16` / `kpe16`."""
    res: Optional[torch.Tensor]         # the residual operand in f32 ...
    res16: Optional[torch.Tensor]       # ... or in bf16
    res_rows: int                       # S: the shared keys, broadcast to every prompt; P * S: per-prompt rows
    y32: Optional[torch.Tensor]         # f32 output; None when nothing reads it later
    broadcast: bool                     # `res` is the shared [S, C] keys, not the [P * S, C] stream the output continues


class _ImageKeys:
    """The image-side key stream through the two-way layers.  It starts as one [S, C] matrix shared by every prompt (`keys` f32, `k16` bf16, `kpe16`
    bf16 with the positional code added) and becomes [P * S, C] rows per prompt at the first image -> token update.  From there on it is either bf16
    only (`bf16_only`: an update reads the previous `k16` as its residual and writes a fresh one) or carries the f32 `keys` beside `k16`, updated in
    place.  `k16` / `kpe16` are what the next product reads; `kpe16` is None once the prompts have diverged: (keys + pe) is never formed per prompt,
    see `_upload_fused_image_projections`."""

    def __init__(self, keys0: torch.Tensor, k16: torch.Tensor, kpe16: torch.Tensor, prompts: int, bf16_only: bool):
        self.shared = True
        self.keys: Optional[torch.Tensor] = keys0
        self.k16, self.kpe16 = k16, kpe16
        self.bf16_only = bf16_only
        self.P, (self.S, self.c) = prompts, keys0.shape

    def begin_update(self, last: bool) -> _KeyUpdate:
        """What the next key update takes as residual and writes in f32; re-binds `k16` / `kpe16` to what it writes in bf16.
        last: no layer follows, so the f32 residual stream is not read after this update."""
        S, c, rows, dev = self.S, self.c, self.P * self.S, self.k16.device
        if self.shared:                                           # the prompts diverge here: materialise per-prompt keys
            res, res16, res_rows = self.keys, None, S
            self.keys = None if last or self.bf16_only else torch.empty((rows, c), dtype=torch.float32, device=dev)
            self.k16 = torch.empty((rows, c), dtype=torch.bfloat16, device=dev)
            self.kpe16 = None
        elif self.bf16_only:                                      # the previous bf16 keys are the residual, the new ones go to a buffer of their own
            res, res16, res_rows = None, self.k16, rows
            self.k16 = torch.empty((rows, c), dtype=torch.bfloat16, device=dev)
        else:                                                     # the f32 stream, updated in place
            res, res16, res_rows = self.keys, None, rows
        update = _KeyUpdate(res, res16, res_rows, None if last else self.keys, self.shared)
        self.shared = False
        return update


class HipSamDecoder:
    def __init__(self, spec: SamDecoderSpec, state: Optional[Dict[str, torch.Tensor]] = None, device="cuda", seed: int = 0):
        self.spec, self.device = spec, torch.device(device)
        self.sd = state if state is not None else random_state(spec, seed)
        self.w: Dict[str, torch.Tensor] = {}
        self.q_prescaled = L.q_prescale_enabled()
        self.res16 = RES16                                        # OVO_SAM_RES16, taken once at construction like q_prescaled
        self.force_unfused = False                                # tests: take the unfused key update (and with it the f32 key stream) at any width
        c, H = spec.hidden, spec.heads
        self.c, self.ci, self.H, self.S = c, c // 2, H, spec.embed_size * spec.embed_size     # the cross attentions work at the inner width C / 2
        self.hd_s, self.hd_c = c // H, c // 2 // H                # head dims: token self-attention, cross attentions
        self._upload_weights()
        self._upload_constants()
        self._upload_fused_image_projections()
        self.tokens0: Optional[torch.Tensor] = None
        self.tok16: Optional[torch.Tensor] = None
        self.P = 0

    # ------------------------------------------------------------------ weights (set-up)
    def _up(self, name: str, t: torch.Tensor, dtype) -> None:
        self.w[name] = t.to(self.device, dtype).contiguous()

    def _lin(self, name: str) -> None:
        self._up(name + ".w", self.sd[name + ".weight"], torch.bfloat16)
        self._up(name + ".b", self.sd[name + ".bias"].float(), torch.float32)

    def _norm(self, name: str, key: Optional[str] = None) -> None:
        key = name if key is None else key
        self._up(key + ".g", self.sd[name + ".weight"].float(), torch.float32)
        self._up(key + ".b", self.sd[name + ".bias"].float(), torch.float32)

    def _upload_weights(self) -> None:
        """The state dict's matrices (bf16) with their biases and norms (f32) under the state dict's names; q | k of the token self-attention as one."""
        sd, spec, c = self.sd, self.spec, self.c
        t = MD + "transformer."
        projections = ("q_proj", "k_proj", "v_proj", "out_proj")
        for i in range(spec.depth):
            b = t + f"layers.{i}."
            sa = b + "self_attn."
            qkw, qkb = torch.cat([sd[sa + "q_proj.weight"], sd[sa + "k_proj.weight"]]), torch.cat([sd[sa + "q_proj.bias"], sd[sa + "k_proj.bias"]])
            if self.q_prescaled:                                  # token self-attention (ovo_attention): log2 e / sqrt(hd) into the q rows, in f32
                qkw, qkb = L.fold_q_scale(qkw, qkb, c, self.hd_s)
            self._up(sa + "qk.w", qkw, torch.bfloat16)
            self._up(sa + "qk.b", qkb.float(), torch.float32)
            self._lin(sa + "v_proj"); self._lin(sa + "out_proj")
            for a in ("cross_attn_token_to_image.", "cross_attn_image_to_token."):
                for p in projections:
                    self._lin(b + a + p)
            self._lin(b + "mlp.layers.0"); self._lin(b + "mlp.layers.1")
            for k in range(1, 5):
                self._norm(b + f"norm{k}")
        for p in projections:
            self._lin(t + "final_attn_token_to_image." + p)
        self._norm(t + "norm_final_attn")
        for i, key in ((0, "up1"), (3, "up2")):                   # ConvTranspose2d [Cin, Cout, 2, 2] -> GEMM weight [(dy, dx, co), Cin]
            wt = sd[MD + f"output_upscaling.{i}.weight"]
            self._up(key + ".w", wt.permute(2, 3, 1, 0).reshape(4 * wt.shape[1], wt.shape[0]), torch.bfloat16)
            self._up(key + ".b", sd[MD + f"output_upscaling.{i}.bias"].float(), torch.float32)
        self._norm(MD + "output_upscaling.1", "up_ln")
        for i in range(spec.n_mask_tokens):
            for j in range(3):
                self._lin(MD + f"output_hypernetworks_mlps.{i}.layers.{j}")
        for j in range(3):
            self._lin(MD + f"iou_prediction_head.layers.{j}")

    def _upload_constants(self) -> None:
        """Constants of the generator: the positional code of the embedding grid and the dense "no mask" embedding."""
        sd, c, s = self.sd, self.c, self.spec.embed_size
        self._gauss = sd[PE + "pe_layer.positional_encoding_gaussian_matrix"].double()
        tt = (torch.arange(s, dtype=torch.float64) + 0.5) / s
        yy, xx = torch.meshgrid(tt, tt, indexing="ij")
        self._up("key_pe", fourier_pe(torch.stack([xx, yy], dim=-1), self._gauss).reshape(s * s, c).float(), torch.float32)
        dense = sd[PE + "no_mask_embed.weight"].reshape(1, c).float()
        if "no_mem_embed" in sd:                                  # SAM2ImagePredictor adds it to the lowest-resolution feature
            dense = dense + sd["no_mem_embed"].reshape(1, c).float()
        self._up("dense", dense, torch.float32)

    def _upload_fused_image_projections(self) -> None:
        """Image-side projections once the prompts have diverged (layers >= 1 and the final attention): K | V (| Q of the image -> token
        attention) read the same keys, so they are ONE product over them; the positional code enters as its own projection, a per-pixel
        constant added in the epilogue (ovo_gemm_periodic): k_proj(keys + pe) = keys . Wk^T + (pe . Wk^T)[pixel]."""
        sd = self.sd
        pe64 = self.w["key_pe"].double().cpu()

        def fuse(name, parts):                                     # parts: (projection, adds the positional code?)
            ws = [sd[pn + ".weight"] for pn, _ in parts]
            self._up(name + ".w", torch.cat(ws), torch.bfloat16)
            self._up(name + ".b", torch.cat([sd[pn + ".bias"] for pn, _ in parts]).float(), torch.float32)
            cols = [pe64 @ w.to(torch.bfloat16).double().T if with_pe else torch.zeros(pe64.shape[0], w.shape[0], dtype=torch.float64)
                    for w, (_, with_pe) in zip(ws, parts)]
            self._up(name + ".add", torch.cat(cols, dim=1).float(), torch.float32)

        t = MD + "transformer."
        for i in range(1, self.spec.depth):
            b = t + f"layers.{i}."
            fuse(b + "kvq", [(b + "cross_attn_token_to_image.k_proj", True), (b + "cross_attn_token_to_image.v_proj", False),
                             (b + "cross_attn_image_to_token.q_proj", True)])
        fuse(t + "final_kv", [(t + "final_attn_token_to_image.k_proj", True), (t + "final_attn_token_to_image.v_proj", False)])

    # ------------------------------------------------------------------ prompts (set-up)
    def set_points(self, points_xy: torch.Tensor, labels: Optional[torch.Tensor] = None) -> None:
        """points [P, 2] (x, y) in pixels of the image_size^2 model input, one click per prompt; labels [P] (default 1).
        Builds the constant token matrix [P, 8, C] = (obj, iou, 4 mask tokens, click, "not a point" padding)."""
        sd, spec = self.sd, self.spec
        pts = points_xy.double().cpu()
        p = pts.shape[0]
        lab = torch.ones(p, dtype=torch.long) if labels is None else labels.long().cpu()
        pe = fourier_pe((pts + 0.5) / float(spec.image_size), self._gauss).float()
        emb = torch.stack([sd[PE + f"point_embeddings.{i}.weight"][0] for i in (0, 1)]).float()
        click = pe + emb[lab]
        out_tok = torch.cat([sd[MD + "obj_score_token.weight"], sd[MD + "iou_token.weight"], sd[MD + "mask_tokens.weight"]], 0).float()
        pad = sd[PE + "not_a_point_embed.weight"].float()
        tokens = torch.cat([out_tok[None].expand(p, -1, -1), click[:, None], pad[None].expand(p, -1, -1)], dim=1)
        self.tokens0 = tokens.reshape(-1, spec.hidden).to(self.device).contiguous()
        self.tok16 = self.tokens0.to(torch.bfloat16)
        self.P, self.T = p, tokens.shape[1]

    def set_point_grid(self, n_per_side: int) -> torch.Tensor:
        pts = point_grid(n_per_side) * self.spec.image_size
        self.set_points(pts)
        return pts

    # ------------------------------------------------------------------ launches
    def _gemm(self, a: torch.Tensor, wname: str, out_dtype, act: int = 0, add: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None, rows: Optional[int] = None, lda: Optional[int] = None, ldc: Optional[int] = None,
              a_off: int = 0, c_off: int = 0, bias: bool = True, add_rows: int = 0) -> torch.Tensor:
        w = self.w[wname + ".w"]
        if out is None:
            out = torch.empty((a.shape[0] if rows is None else rows, w.shape[0]), dtype=out_dtype, device=a.device)
        g = L.gemm_desc(a, w, out, bias=self.w[wname + ".b"] if bias else None, add=add, act=act, rows=rows, lda=lda, a_off=a_off, ldc=ldc, c_off=c_off)
        if add_rows:                                              # add[m % add_rows]: a per-pixel constant shared by every prompt
            L.check(L.load().ovo_gemm_periodic(C.byref(g), add_rows, L.stream()))
        else:
            L.check(L.load().ovo_gemm(C.byref(g), L.stream()))
        return out

    @staticmethod
    def _attn(q, k, v, o, B, H, Tq, Tk, hd, qs, ks, vs, os_, prescaled=False):
        """q/k/v/o: (tensor, element offset); *s: (batch, head, token) strides in elements.  prescaled: q already carries
        log2(e) / sqrt(hd) (folded into its projection at load time) -> scale 0 = no factor inside the kernel."""
        a = L.Attention()
        a.q, a.k, a.v, a.o = (t.data_ptr() + off * t.element_size() for t, off in (q, k, v, o))
        a.q_sb, a.q_sh, a.q_st = qs
        a.k_sb, a.k_sh, a.k_st = ks
        a.v_sb, a.v_sh, a.v_st = vs
        a.o_sb, a.o_sh, a.o_st = os_
        a.B, a.H, a.Tq, a.Tk, a.hd, a.scale = B, H, Tq, Tk, hd, (0.0 if prescaled else hd ** -0.5)
        L.check(L.load().ovo_attention(C.byref(a), L.stream()))

    def _rows(self, x, R, Cc, *, base=None, base_rows=0, norm=None, eps=1e-5, pe=None, pe_rows=0, y=None, y16=None, ype16=None):
        g = self.w[norm + ".g"] if norm else None
        b = self.w[norm + ".b"] if norm else None
        L.check(L.load().ovo_row_epilogue(L.ptr(x), R, Cc, L.ptr(base), base_rows, L.ptr(g), L.ptr(b), eps, L.ptr(pe), pe_rows,
                                          L.ptr(y), L.ptr(y16), L.ptr(ype16), L.stream()))

    # ------------------------------------------------------------------ fused entry points (samfuse.hip), each with the chain it replaces
    @staticmethod
    def _unsupported(rc: int) -> bool:
        """True when a fused entry point answered OVO_E_UNSUPPORTED -- it has no instantiation for the shape, the caller runs the unfused chain;
        any other failure raises."""
        if rc == L.E_UNSUPPORTED:
            return True
        L.check(rc)
        return False

    def _image_proj(self, a16: torch.Tensor, wname: str, groups) -> torch.Tensor:
        """bf16 [rows, N] = a16 . W^T + bias + add[row % S] for the fused image-side projection `wname` (see `_upload_fused_image_projections`),
        computed as one LDS-resident-weight stream per column group (`groups`: widths summing to N; ovo_sam_linear) or, for widths that entry
        point has no instantiation for, as one tiled GEMM with the periodic add."""
        w, bias, add = self.w[wname + ".w"], self.w[wname + ".b"], self.w[wname + ".add"]
        n, k = w.shape
        rows, S = a16.shape[0], add.shape[0]
        out = torch.empty((rows, n), dtype=torch.bfloat16, device=a16.device)
        lib, lo = L.load(), 0
        for width in groups:
            rc = lib.ovo_sam_linear(L.ptr(a16), C.c_void_p(w.data_ptr() + 2 * lo * k), C.c_void_p(bias.data_ptr() + 4 * lo),
                                    C.c_void_p(add.data_ptr() + 4 * lo), S, n, C.c_void_p(out.data_ptr() + 2 * lo), n, rows, width, k, L.stream())
            if self._unsupported(rc):
                return self._gemm(a16, wname, torch.bfloat16, add=add, add_rows=S, out=out)
            lo += width
        return out

    def _t2i_attention(self, tq: torch.Tensor, k, v, kv_sb: int, kv_st: int, o: torch.Tensor) -> None:
        """o [P * T, ci] = attention of every prompt's T token queries `tq` over its S image keys.  k / v: (tensor, element offset), rows `kv_st`
        elements apart, prompts `kv_sb` apart (0: one set of keys shared by all).  The dedicated kernel exists for head dim 16."""
        P, S, T, H, ci, hd = self.P, self.S, self.T, self.H, self.ci, self.hd_c
        rc = L.E_UNSUPPORTED
        if hd == 16:
            kptr, vptr = (C.c_void_p(t.data_ptr() + off * 2) for t, off in (k, v))
            rc = L.load().ovo_sam_t2i_attention(L.ptr(tq), kptr, vptr, kv_sb, kv_st, L.ptr(o), P, S, T, H, hd ** -0.5, L.stream())
        if self._unsupported(rc):
            self._attn((tq, 0), k, v, (o, 0), P, H, T, S, hd, (T * ci, hd, ci), (kv_sb, hd, kv_st), (kv_sb, hd, kv_st), (T * ci, hd, ci))

    def _update_keys(self, b: str, oi: torch.Tensor, keys: _ImageKeys, last: bool) -> None:
        """The image -> token attention's out-projection + residual + norm4 (+ the bf16 copies the next products read): one fused launch; widths
        it does not cover run the product and the row pass separately, over the f32 stream (the bf16-only stream exists at covered widths only)."""
        P, S, c, w, key_pe = self.P, self.S, self.c, self.w, self.w["key_pe"]
        a = b + "cross_attn_image_to_token."
        u = keys.begin_update(last)
        rc = L.E_UNSUPPORTED if self.force_unfused else \
            L.load().ovo_sam_proj_ln(L.ptr(oi), L.ptr(w[a + "out_proj.w"]), L.ptr(w[a + "out_proj.b"]), L.ptr(u.res), L.ptr(u.res16), u.res_rows,
                                     L.ptr(w[b + "norm4.g"]), L.ptr(w[b + "norm4.b"]), 1e-5, L.ptr(key_pe), S, L.ptr(u.y32), L.ptr(keys.k16),
                                     L.ptr(keys.kpe16), P * S, c, self.ci, L.stream())
        if not self._unsupported(rc):
            return
        if u.broadcast:
            x = self._gemm(oi, a + "out_proj", torch.float32)
            self._rows(x, P * S, c, base=u.res, base_rows=u.res_rows, norm=b + "norm4", pe=key_pe, pe_rows=S, y=u.y32, y16=keys.k16, ype16=keys.kpe16)
        else:
            self._gemm(oi, a + "out_proj", torch.float32, add=u.res, out=u.res)
            self._rows(u.res, P * S, c, norm=b + "norm4", pe=key_pe, pe_rows=S, y=u.y32, y16=keys.k16, ype16=keys.kpe16)

    def _up1_ln(self, k16: torch.Tensor, f1: torch.Tensor) -> torch.Tensor:
        """bf16 [P * 4S, C/4]: the first transposed convolution as a skinny product fused with what follows it (+ feat_s1, LayerNorm2d, GELU)."""
        P, s, c, w = self.P, self.spec.embed_size, self.c, self.w
        up1 = torch.empty((P * 4 * self.S, c // 4), dtype=torch.bfloat16, device=self.device)
        lib = L.load()
        rc = lib.ovo_sam_up1_ln(L.ptr(k16), L.ptr(w["up1.w"]), L.ptr(w["up1.b"]), L.ptr(f1), L.ptr(w["up_ln.g"]), L.ptr(w["up_ln.b"]), 1e-6,
                                P, s, c // 4, c, L.ptr(up1), L.stream())
        if self._unsupported(rc):
            g1 = self._gemm(k16, "up1", torch.bfloat16, bias=False)                       # [P*S, 4 * c/4]
            L.check(lib.ovo_sam_upscale_ln(L.ptr(g1), L.ptr(w["up1.b"]), L.ptr(f1), L.ptr(w["up_ln.g"]), L.ptr(w["up_ln.b"]), 1e-6,
                                           P, s, c // 4, L.ptr(up1), L.stream()))
        return up1

    def _up2_masks(self, up1: torch.Tensor, f0: torch.Tensor, hyper: torch.Tensor, first: int) -> torch.Tensor:
        """f32 [P, n - first, 4s, 4s]: the second transposed convolution fused with what follows it (+ feat_s0, GELU, the product with the hyper-network
        rows `first` .. n - 1 of `hyper` [P, n, C/8])."""
        P, s, c, w, n = self.P, self.spec.embed_size, self.c, self.w, hyper.shape[1]
        masks = torch.empty((P, n - first, 4 * s, 4 * s), dtype=torch.float32, device=self.device)
        lib = L.load()
        rc = lib.ovo_sam_up2_masks(L.ptr(up1), L.ptr(w["up2.w"]), L.ptr(w["up2.b"]), L.ptr(f0), L.ptr(hyper), n, first, P, 2 * s, c // 8, c // 4,
                                   L.ptr(masks), L.stream())
        if self._unsupported(rc):
            g2 = self._gemm(up1, "up2", torch.bfloat16, bias=False)                       # [P*4S, 4 * c/8]
            L.check(lib.ovo_sam_upscale_masks(L.ptr(g2), L.ptr(w["up2.b"]), L.ptr(f0), L.ptr(hyper), n, first, P, 2 * s, c // 8, L.ptr(masks),
                                              L.stream()))
        return masks

    # ------------------------------------------------------------------ steps of the forward
    def _layer0_keys(self, emb: torch.Tensor) -> _ImageKeys:
        """keys = image embedding + dense "no mask" embedding, in f32, bf16 and bf16 with the positional code: shared by every prompt."""
        S, c, dev = self.S, self.c, self.device
        keys0 = torch.empty((S, c), dtype=torch.float32, device=dev)
        k16 = torch.empty((S, c), dtype=torch.bfloat16, device=dev)
        kpe16 = torch.empty((S, c), dtype=torch.bfloat16, device=dev)
        self._rows(emb, S, c, base=self.w["dense"], base_rows=1, pe=self.w["key_pe"], pe_rows=S, y=keys0, y16=k16, ype16=kpe16)
        # the per-prompt keys live as bf16 only where the fused out-projection + norm kernel exists (hidden 256 / 128, samfuse.hip); at any
        # other width the unfused chain needs the f32 stream as its residual operand (`force_unfused`: tests)
        bf16_only = self.res16 and c in (256, 128) and not self.force_unfused
        return _ImageKeys(keys0, k16, kpe16, self.P, bf16_only)

    def _token_buffers(self) -> _Tokens:
        R, c, dev = self.P * self.T, self.c, self.device
        q = torch.empty((R, c), dtype=torch.float32, device=dev)
        q16 = torch.empty((R, c), dtype=torch.bfloat16, device=dev)
        qpe16 = torch.empty((R, c), dtype=torch.bfloat16, device=dev)
        attn_out = torch.empty((R, c), dtype=torch.bfloat16, device=dev)
        return _Tokens(q, q16, qpe16, attn_out)

    def _per_prompt_proj(self, keys: _ImageKeys, wname: str, groups) -> Optional[torch.Tensor]:
        """The fused image-side projection `wname` of the per-prompt keys, bf16 [P * S, sum(groups)]; None while the keys are shared (layer 0): each
        attention then projects the one [S, C] matrix itself."""
        return None if keys.shared else self._image_proj(keys.k16, wname, groups)

    def _self_attention(self, b: str, tok: _Tokens, first: bool) -> None:
        """Self attention on the tokens + norm1 (first layer: the tokens as given are the input, no positional code, no residual)."""
        P, T, c, H, hd = self.P, self.T, self.c, self.H, self.hd_s
        qk = self._gemm(self.tok16 if first else tok.qpe16, b + "self_attn.qk", torch.bfloat16)          # [R, 2c]
        v = self._gemm(self.tok16 if first else tok.q16, b + "self_attn.v_proj", torch.bfloat16)         # [R, c]
        self._attn((qk, 0), (qk, c), (v, 0), (tok.attn_out, 0), P, H, T, T, hd, (T * 2 * c, hd, 2 * c), (T * 2 * c, hd, 2 * c),
                   (T * c, hd, c), (T * c, hd, c), prescaled=self.q_prescaled)
        self._gemm(tok.attn_out, b + "self_attn.out_proj", torch.float32, add=None if first else tok.q, out=tok.q)
        self._rows(tok.q, P * T, c, norm=b + "norm1", pe=self.tokens0, pe_rows=P * T, y=tok.q, y16=tok.q16, ype16=tok.qpe16)

    def _token_to_image(self, pre: str, norm: str, tok: _Tokens, keys: _ImageKeys, kv: Optional[torch.Tensor]) -> None:
        """The tokens attend to the image + `norm`.  kv: the fused per-prompt projection bf16 [P*S, n * ci] (K | V | ...), or None while the keys are
        shared (layer 0)."""
        S, c, ci, R = self.S, self.c, self.ci, self.P * self.T
        tq = self._gemm(tok.qpe16, pre + "q_proj", torch.bfloat16)                        # [R, ci]
        if kv is None:
            K = self._gemm(keys.kpe16, pre + "k_proj", torch.bfloat16)                    # [S, ci]
            V = self._gemm(keys.k16, pre + "v_proj", torch.bfloat16)
            k, v, kv_sb, kv_st = (K, 0), (V, 0), 0, ci
        else:
            k, v, kv_sb, kv_st = (kv, 0), (kv, ci), S * kv.shape[1], kv.shape[1]
        o = torch.empty((R, ci), dtype=torch.bfloat16, device=self.device)
        self._t2i_attention(tq, k, v, kv_sb, kv_st, o)
        self._gemm(o, pre + "out_proj", torch.float32, add=tok.q, out=tok.q)
        self._rows(tok.q, R, c, norm=norm, y=tok.q, y16=tok.q16)

    def _mlp(self, b: str, tok: _Tokens) -> None:
        R, c = self.P * self.T, self.c
        h = self._gemm(tok.q16, b + "mlp.layers.0", torch.bfloat16, act=3)
        self._gemm(h, b + "mlp.layers.1", torch.float32, add=tok.q, out=tok.q)
        self._rows(tok.q, R, c, norm=b + "norm3", pe=self.tokens0, pe_rows=R, y=tok.q, y16=tok.q16, ype16=tok.qpe16)

    def _image_to_token(self, a: str, tok: _Tokens, keys: _ImageKeys, kvq: Optional[torch.Tensor]) -> torch.Tensor:
        """bf16 [P * S, ci]: the image attends to the tokens (before its out-projection: `_update_keys`).  kvq: K | V | Q of the per-prompt keys in one
        matrix, or None while the keys are shared."""
        P, S, T, H, ci, hd = self.P, self.S, self.T, self.H, self.ci, self.hd_c
        kt = self._gemm(tok.qpe16, a + "k_proj", torch.bfloat16)                          # [R, ci]
        vt = self._gemm(tok.q16, a + "v_proj", torch.bfloat16)
        if kvq is None:
            qi, q_off, q_sb, q_st = self._gemm(keys.kpe16, a + "q_proj", torch.bfloat16), 0, 0, ci       # [S, ci]
        else:
            qi, q_off, q_sb, q_st = kvq, 2 * ci, S * 3 * ci, 3 * ci
        oi = torch.empty((P * S, ci), dtype=torch.bfloat16, device=self.device)
        if hd == 16 and T <= 16 and 256 % H == 0:                 # S queries x 8 keys: the dedicated HBM-bound kernel
            L.check(L.load().ovo_sam_i2t_attention(C.c_void_p(qi.data_ptr() + 2 * q_off), q_sb, q_st, L.ptr(kt), L.ptr(vt), L.ptr(oi), P, S, T, H,
                                                   hd ** -0.5, L.stream()))
        else:
            self._attn((qi, q_off), (kt, 0), (vt, 0), (oi, 0), P, H, S, T, hd, (q_sb, hd, q_st), (T * ci, hd, ci), (T * ci, hd, ci), (S * ci, hd, ci))
        return oi

    def _heads(self, q16: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(predicted IoU f32 [P, nm], hyper-network rows f32 [P, nm, C/8]) straight from strided token rows: token 1 and tokens 2 .. 2 + nm."""
        P, T, c, nm = self.P, self.T, self.c, self.spec.n_mask_tokens
        bf, f32 = torch.bfloat16, torch.float32
        x = self._gemm(q16, MD + "iou_prediction_head.layers.0", bf, act=3, rows=P, lda=T * c, a_off=1 * c)
        x = self._gemm(x, MD + "iou_prediction_head.layers.1", bf, act=3)
        iou = self._gemm(x, MD + "iou_prediction_head.layers.2", f32, act=4)
        hyper = torch.empty((P, nm, c // 8), dtype=f32, device=self.device)
        for m in range(nm):
            pre = MD + f"output_hypernetworks_mlps.{m}."
            x = self._gemm(q16, pre + "layers.0", bf, act=3, rows=P, lda=T * c, a_off=(2 + m) * c)
            x = self._gemm(x, pre + "layers.1", bf, act=3)
            self._gemm(x, pre + "layers.2", f32, out=hyper, ldc=nm * (c // 8), c_off=m * (c // 8))
        return iou, hyper

    # ------------------------------------------------------------------ forward
    def forward(self, image_embed: torch.Tensor, feat_s1: torch.Tensor, feat_s0: torch.Tensor, multimask: bool = True
                ) -> Tuple[torch.Tensor, torch.Tensor]:
        """image_embed f32 [s, s, C] (NHWC, as HipHiera emits it), feat_s1 f32 [2s, 2s, C/4], feat_s0 f32 [4s, 4s, C/8]
        -> (mask logits f32 [P, 3 | 4, 4s, 4s], predicted IoU f32 [P, 3 | 4]) for the prompts of set_points()."""
        if self.tokens0 is None:
            raise L.OvoHipError("set_points() / set_point_grid() first")
        spec, S, c, ci = self.spec, self.S, self.c, self.ci
        emb = L.dev(image_embed.reshape(S, c), torch.float32, "image_embed")
        f1 = L.dev(feat_s1.reshape(4 * S, c // 4), torch.float32, "feat_s1")
        f0 = L.dev(feat_s0.reshape(16 * S, c // 8), torch.float32, "feat_s0")
        t = MD + "transformer."

        keys = self._layer0_keys(emb)
        tok = self._token_buffers()
        for i in range(spec.depth):
            b = t + f"layers.{i}."
            # K | V of the token -> image attention and Q of the image -> token attention in one product over the per-prompt keys
            kvq = self._per_prompt_proj(keys, b + "kvq", (2 * ci, ci))                    # [P*S, 3 ci]
            self._self_attention(b, tok, first=i == 0)
            self._token_to_image(b + "cross_attn_token_to_image.", b + "norm2", tok, keys, kvq)
            self._mlp(b, tok)
            oi = self._image_to_token(b + "cross_attn_image_to_token.", tok, keys, kvq)
            self._update_keys(b, oi, keys, last=i == spec.depth - 1)
        kv = self._per_prompt_proj(keys, t + "final_kv", (2 * ci,))                       # [P*S, 2 ci]
        self._token_to_image(t + "final_attn_token_to_image.", t + "norm_final_attn", tok, keys, kv)

        iou, hyper = self._heads(tok.q16)
        # multimask: mask tokens 1 .. nm - 1 are the outputs; otherwise token 0 alone, and only its hyper-network row is handed on
        first, n = (1, spec.n_mask_tokens) if multimask else (0, 1)
        up1 = self._up1_ln(keys.k16, f1)
        masks = self._up2_masks(up1, f0, hyper[:, :n].contiguous(), first)
        return masks, iou[:, first:n]

