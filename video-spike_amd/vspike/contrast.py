"""ContrastViT plugin — drop-in for the reference's `src/model/vit_mae/vit_mae.py:26-44`
(NAME2MODEL['ContrastViT'], the model `src/pretrain.py --model c` selects).

The reference wraps HF `ViTMAEModel` at mask_ratio 0 and projects the CLS token:

    x[g, 0] = cls + table[0];  x[g, 1 + p] = Conv2d_{k=s=patch}(image g)[p] + table[1 + p]
    for i in range(L): x = pre-LN block_i(x)                      # q, k, v biases; the block VideoMAE runs
    h = LayerNorm(x[:, 0]);  z_raw = h @ proj.weight.T + proj.bias;  z = z_raw / |z_raw|
    return {'z': z, 'temp': 1 / exp(temperature)}

with `table` the fixed 2-D sin-cos table (row 0 zeros).  Two things of HF's forward are left out, both
without effect on `z`, the loss or any gradient: the random shuffle of the patch
tokens (attention is permutation-equivariant and only the CLS row is read) and the key bias (it shifts
every logit of a query row equally; its gradient is zero, it is accepted on load and exported as zeros).

Everything of the blocks is the VideoMAE plugin's (this class subclasses it: the flat-buffer layout,
the activation arena, the block executor structs, the bf16 shadows, the blocks' backward — with the
weight-gradient products in order on the main stream, never on the side stream: see set_side_stream).  New here: vs_cls_embed_fwd / _bwd around the generic im2col + GEMM patch product,
vs_embed_head_fwd / _bwd on the CLS row, and the state-dict names of the reference's module.
"""
from __future__ import annotations

import dataclasses
import math
import re
import types
import weakref
from typing import Optional

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import ops
from .layout import BackboneCfg, FlatLayout, _layer_hf_items, _layer_shapes, modern_name
from .memory import Arena
from .vit import _DTYPES, VideoMAE, _FwdState, _cfg_get, _dev_key


@dataclasses.dataclass(frozen=True)
class ContrastCfg(BackboneCfg):
    """Geometry of the 2-D encoder: one frame, no tubelet, and a CLS token in front of the patches."""
    image_size: int = 144
    num_channels: int = 1
    num_frames: int = 1
    tubelet_size: int = 1

    @property
    def num_patches(self) -> int:
        g = self.image_size // self.patch_size
        return g * g

    @property
    def num_tokens(self) -> int:
        return self.num_patches + 1


def sincos_2d_table(dim: int, grid: int) -> np.ndarray:
    """HF ViTMAE's fixed position table (`get_2d_sincos_pos_embed(dim, grid, add_cls_token=True)`): float64
    angles, row 0 zeros, patch (h, w) -> [sin(w o) | cos(w o) | sin(h o) | cos(h o)], o_k = 10000^(-k / (dim/4))."""
    if dim % 4:
        raise ValueError("the 2-D sin-cos table needs hidden_size % 4 == 0")
    q = dim // 4
    omega = 1.0 / 10000.0 ** (np.arange(q, dtype=np.float64) / q)
    hh, ww = np.meshgrid(np.arange(grid, dtype=np.float64), np.arange(grid, dtype=np.float64), indexing="ij")
    eh, ew = np.outer(hh.reshape(-1), omega), np.outer(ww.reshape(-1), omega)
    t = np.concatenate([np.sin(ew), np.cos(ew), np.sin(eh), np.cos(eh)], axis=1)
    return np.concatenate([np.zeros((1, dim)), t], axis=0)


class ContrastLayout:
    """encoder flat: patch_w, patch_b, cls, per layer LAYER_KEYS, lnf_g, lnf_b; head flat: proj_w, proj_b."""

    def __init__(self, cfg: ContrastCfg, embed: int):
        self.cfg, self.embed = cfg, embed
        D, F = cfg.hidden_size, cfg.intermediate_size
        e = FlatLayout()
        e.add("patch_w", (D, cfg.patch_dim))
        e.add("patch_b", (D,))
        e.add("cls", (D,))
        self.layer_ranges = []
        for i in range(cfg.num_hidden_layers):
            lo = e.numel
            for k, shape in _layer_shapes(D, F):
                e.add(f"{i}.{k}", shape)
            self.layer_ranges.append((lo, e.numel))
        self.final_range = (e.numel, 0)
        e.add("lnf_g", (D,))
        e.add("lnf_b", (D,))
        self.final_range = (self.final_range[0], e.numel)
        self.enc = e
        h = FlatLayout()
        h.add("proj_w", (embed, D))
        h.add("proj_b", (embed,))
        self.head = h

    def hf_items(self):
        """(name, which_flat, slot, row_slice) under the reference module's names (HF ViTMAEModel as `vit`)."""
        D = self.cfg.hidden_size
        yield "vit.embeddings.cls_token", "enc", "cls", None
        yield "vit.embeddings.patch_embeddings.projection.weight", "enc", "patch_w", None
        yield "vit.embeddings.patch_embeddings.projection.bias", "enc", "patch_b", None
        for i in range(self.cfg.num_hidden_layers):
            for name, which, slot, rows in _layer_hf_items(f"vit.encoder.layer.{i}.", "enc", i, D):
                yield modern_name(name), which, slot, rows      # ViTMAE spells the biases query.bias / value.bias
        yield "vit.layernorm.weight", "enc", "lnf_g", None
        yield "vit.layernorm.bias", "enc", "lnf_b", None
        yield "proj.weight", "head", "proj_w", None
        yield "proj.bias", "head", "proj_b", None


# transformers 5.x spellings of a block's parameters -> the reference's (4.38)
_V5 = (("attention.q_proj.", "attention.attention.query."), ("attention.k_proj.", "attention.attention.key."),
       ("attention.v_proj.", "attention.attention.value."), ("attention.o_proj.", "attention.output.dense."),
       ("mlp.fc1.", "intermediate.dense."), ("mlp.fc2.", "output.dense."))


def _reference_name(key: str) -> str:
    m = re.match(r"vit\.layers\.(\d+)\.(.*)$", key)
    if not m:
        return key
    rest = m.group(2)
    for new, old in _V5:
        if rest.startswith(new):
            rest = old + rest[len(new):]
            break
    return f"vit.encoder.layer.{m.group(1)}.{rest}"


def _v5_name(key: str) -> str:
    m = re.match(r"vit\.encoder\.layer\.(\d+)\.(.*)$", key)
    if not m:
        return key
    rest = m.group(2)
    for new, old in _V5:
        if rest.startswith(old):
            rest = new + rest[len(old):]
            break
    return f"vit.layers.{m.group(1)}.{rest}"


class ContrastViT(VideoMAE):
    # the flat parameter buffers whose gradients the data-parallel sink owns (vspike.dp.GradExchange);
    # `temperature` is reduced with the non-sink parameters in GradExchange.finish()
    SUNK_BUFFERS = ("enc_flat", "head_flat")

    def __init__(self, config):
        nn.Module.__init__(self)
        names = {f.name for f in dataclasses.fields(ContrastCfg)} - {"num_frames", "tubelet_size"}
        kw = {}
        for k in names:
            v = _cfg_get(config, k, None)
            if v is not None:
                kw[k] = float(v) if k == "layer_norm_eps" else int(v)
        cfg = self.backbone = ContrastCfg(**kw)
        self.embed_size = int(_cfg_get(config, "embed_size", 0) or 0)
        self.fix_temp = bool(_cfg_get(config, "fix_temp", True))
        cdt = str(_cfg_get(config, "compute_dtype", "fp32")).lower()
        if cdt in ("fp8", "mxfp8"):
            raise ValueError("ContrastViT: compute_dtype fp8 is not supported (fp32 | bf16)")
        if cdt not in _DTYPES:
            raise ValueError(f"ContrastViT: unknown compute_dtype {cdt!r}")
        self.compute_dtype = _DTYPES[cdt]
        self.fp8 = False
        self.freeze_encoder = False          # everything trains (src/trainer/contrast.py:124-127)
        if cfg.hidden_size != 64 * cfg.num_attention_heads:
            raise ValueError("this build supports head dim 64 (hidden_size = 64 * num_attention_heads)")
        for k in ("hidden_dropout_prob", "attention_probs_dropout_prob"):
            if float(_cfg_get(config, k, 0.0) or 0.0) != 0.0:
                raise ValueError(f"ContrastViT: {k} must be 0 (the kernels have no dropout)")
        if str(_cfg_get(config, "hidden_act", "gelu")).lower() != "gelu":
            raise ValueError("ContrastViT: hidden_act must be gelu")
        if not bool(_cfg_get(config, "qkv_bias", True)):
            raise ValueError("ContrastViT: qkv_bias must be true (the block executor always carries the biases)")
        if not 1 <= self.embed_size <= 256:
            raise ValueError("ContrastViT: embed_size must be in 1..256")
        if cfg.image_size <= 0 or cfg.patch_size <= 0 or cfg.image_size % cfg.patch_size:
            raise ValueError("ContrastViT: image_size must be a positive multiple of patch_size (vs_patch_im2col)")
        if cfg.patch_dim % 8 or cfg.intermediate_size % 8:
            raise ValueError("ContrastViT: num_channels * patch_size^2 and intermediate_size must be multiples of 8")
        # mask_ratio (forced to 0 by the reference, vit_mae.py:31) and the decoder_* keys are not read; the
        # reference trainer's transform() sets and restores `model.config.mask_ratio` (contrast.py:177-202)
        self.config = types.SimpleNamespace(mask_ratio=0.0)
        self.layout = ContrastLayout(cfg, self.embed_size)
        self.enc_flat = nn.Parameter(torch.zeros(self.layout.enc.numel))
        self.head_flat = nn.Parameter(torch.zeros(self.layout.head.numel))
        # tau = 1 / exp(temperature) (vit_mae.py:34,43).  Apart from the flat buffers: under fix_temp the
        # reference's gets no gradient and AdamW skips it, so it must not sit in a weight-decayed buffer
        self.temperature = nn.Parameter(torch.zeros(()), requires_grad=not self.fix_temp)
        self.grad_sink = None
        self._pos_cache = {}
        # the blocks' weight-gradient products run in order on the main stream (no side stream): see set_side_stream
        self.__dict__["_side"] = False
        self.reset_parameters()

    # ---------------------------------------------------------------------------------------
    # parameters
    # ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def reset_parameters(self, generator: Optional[torch.Generator] = None):
        """HF ViTMAE's init: N(0, 0.02) Linear weights and CLS token, zero biases, LayerNorm (1, 0), the
        patch projection xavier-uniform as a Linear; nn.Linear's default for `proj`."""
        enc, head, lay = self.enc_flat, self.head_flat, self.layout
        enc.zero_()
        for name, slot in lay.enc.slots.items():
            v = lay.enc.view(enc, name)
            if name.endswith(("ln1_g", "ln2_g", "lnf_g")):
                v.fill_(1.0)
            elif name == "patch_w":
                bound = math.sqrt(6.0 / (slot.shape[0] + slot.shape[1]))
                v.uniform_(-bound, bound, generator=generator)
            elif name == "cls" or len(slot.shape) == 2:
                v.normal_(0.0, 0.02, generator=generator)
        head.zero_()
        bound = 1.0 / math.sqrt(self.backbone.hidden_size)
        lay.head.view(head, "proj_w").uniform_(-bound, bound, generator=generator)
        lay.head.view(head, "proj_b").uniform_(-bound, bound, generator=generator)
        self.temperature.zero_()

    def __getstate__(self):
        st = super().__getstate__()
        st.pop("_live", None)
        return st

    # VideoMAE is subclassed for its block machinery only (arena planning, _layer_struct, the bf16 shadows, the
    # caches, _blocks_backward).  What it has for its own 3-D patch embedding and regression head cannot work on
    # this layout, so it is closed off here instead of failing somewhere inside.
    def _not_for_this_plugin(self, *args, **kwargs):
        raise NotImplementedError("VideoMAE's video preprocessing, tubelet patch embedding and regression head do "
                                  "not exist in ContrastViT")

    preprocess = raw_frame_indices = _apply_fn = _encoder_forward = _encoder_backward = _not_for_this_plugin

    def set_side_stream(self, enabled: bool) -> None:
        """This plugin runs the blocks' dW products in order on the main stream only.  With them on the block
        executor's side stream the bf16 backward was not bitwise reproducible at the 82-token geometry (about 1
        backward in 100 differed), so that path is not offered here until the cause is found."""
        if enabled:
            raise ValueError("ContrastViT runs its weight-gradient products in order; the side stream is not "
                             "available for this plugin (DESIGN.md section 7)")
        self.__dict__["_side"] = False
        self._caches()[2].clear()

    def _table64(self) -> np.ndarray:
        cfg = self.backbone
        return sincos_2d_table(cfg.hidden_size, cfg.image_size // cfg.patch_size)

    def _pos_table(self, device):
        """The fixed 2-D sin-cos table [P + 1, D] (computed once in f64, cached per device; not a parameter)."""
        key = _dev_key(device)
        if key not in self._pos_cache:
            self._pos_cache[key] = torch.from_numpy(self._table64().astype(np.float32)).to(device)
        return self._pos_cache[key]

    def _slot_shape(self, slot: str):
        cfg = self.backbone
        if slot == "patch_w":
            return (cfg.hidden_size, cfg.num_channels, cfg.patch_size, cfg.patch_size)
        if slot == "cls":
            return (1, 1, cfg.hidden_size)
        return None

    def reference_state_dict(self, modern_names: bool = False):
        """Parameters under the reference plugin's names (`vit.*` = HF ViTMAEModel of the pinned
        transformers 4.38, `proj.*`, `temperature`); with `modern_names` the block names of
        transformers 5.x (`vit.layers.{i}.attention.q_proj`, `mlp.fc1`, ..).  `key.bias` is exported as
        zeros and `position_embeddings` as the fixed table."""
        cfg, D = self.backbone, self.backbone.hidden_size
        out = {}
        for name, which, slot, rows in self.layout.hf_items():
            t = self._flat_layout(which).view(self._flat(which).detach(), slot)
            shape = self._slot_shape(slot)
            t = (t if rows is None else t[rows]).clone()
            out[name] = t.view(shape) if shape else t
        for i in range(cfg.num_hidden_layers):
            out[f"vit.encoder.layer.{i}.attention.attention.key.bias"] = torch.zeros(D)
        out["vit.embeddings.position_embeddings"] = torch.from_numpy(self._table64().astype(np.float32))[None]
        out["temperature"] = self.temperature.detach().clone()
        if modern_names:
            out = {_v5_name(k): v for k, v in out.items()}
        return out

    @torch.no_grad()
    def load_reference_state_dict(self, sd, strict: bool = True):
        """Load a reference `ContrastViT` state_dict (either spelling of the block names).  Any `key.bias`
        is accepted and ignored; a `position_embeddings` that differs from the fixed table by more than
        1e-6 is refused (the plugin has no learned table)."""
        sd = {_reference_name(k): v for k, v in sd.items()}
        seen = set()
        for name, which, slot, rows in self.layout.hf_items():
            if name not in sd:
                if strict:
                    raise KeyError(f"missing {name}")
                continue
            dst = self._flat_layout(which).view(self._flat(which), slot)
            dst = dst[rows] if rows is not None else dst
            dst.copy_(torch.as_tensor(sd[name]).to(dst.device, torch.float32).reshape(dst.shape))
            seen.add(name)
        for k, v in sd.items():
            if k.endswith("attention.attention.key.bias"):
                seen.add(k)
            elif k == "vit.embeddings.position_embeddings":
                t = torch.as_tensor(v).to("cpu", torch.float64).reshape(-1, self.backbone.hidden_size)
                ref = torch.from_numpy(self._table64())
                if t.shape != ref.shape or (t - ref).abs().max().item() > 1e-6:
                    raise ValueError("vit.embeddings.position_embeddings is not the fixed 2-D sin-cos table "
                                     "(the plugin computes the table; a learned one cannot be loaded)")
                seen.add(k)
            elif k == "temperature":
                self.temperature.copy_(torch.as_tensor(v).to(self.temperature.device, torch.float32).reshape(()))
                seen.add(k)
        if strict:
            if "temperature" not in seen:
                raise KeyError("missing temperature")
            extra = set(sd) - seen
            if extra:
                raise KeyError(f"unexpected keys: {sorted(extra)[:5]}")
        self.invalidate_lp()

    # ---------------------------------------------------------------------------------------
    # forward
    # ---------------------------------------------------------------------------------------
    def forward(self, inputs: torch.Tensor):
        cfg = self.backbone
        if inputs.dim() != 4 or tuple(inputs.shape[1:]) != (cfg.num_channels, cfg.image_size, cfg.image_size):
            raise ValueError(f"ContrastViT expects (G, {cfg.num_channels}, {cfg.image_size}, {cfg.image_size})")
        L.require_device(inputs)
        pixels = inputs.detach().to(torch.float32).contiguous()
        z = _ContrastFn.apply(pixels, self.enc_flat, self.head_flat, self)
        return {"z": z, "temp": torch.exp(-self.temperature)}

    def _fwd_buffers(self, G: int, dev, save_encoder: bool):
        """VideoMAE._fwd_buffers for this model: the compact patch rows, the blocks' buffers and what the
        head saves (same caching rules: a forward whose buffers a live autograd state still holds gets a
        private set, so the reference trainer's three forwards before one backward work)."""
        fwd_cache, _, _ = self._caches()
        enc32, head32 = self.enc_flat.detach(), self.head_flat.detach()
        sig = (enc32.data_ptr(), head32.data_ptr())
        key = (G, _dev_key(dev), save_encoder, self.compute_dtype)
        ent = fwd_cache.get(key)
        if ent is not None and ent["sig"] == sig and (ent["owner"] is None or ent["owner"]() is None):
            return ent
        cfg, dt = self.backbone, self.compute_dtype
        P, D, E = cfg.num_patches, cfg.hidden_size, self.embed_size
        ar = Arena()
        fused = self._plan_encoder(ar, G, save_encoder)  # cols, x0, the blocks' activations, X{j}
        # the fused tubelet-gather patch kernels are VideoMAE's (tubelet 2): this model always runs im2col + GEMM
        assert not fused and cfg.tubelet_size == 1, "ContrastViT: the patch embedding must take the im2col path"
        ar.add("patches", (G * P, D), torch.float32)
        for name, shape in (("hh", (G, D)), ("hmean", (G,)), ("hrstd", (G,)), ("hnrm", (G,)), ("z_raw", (G, E))):
            ar.add(name, shape, torch.float32)
        act = ar.allocate(dev)
        enc_lp = self._lp_shadows(dev)["enc"][0] if dt != torch.float32 else enc32
        structs, x = self._encoder_structs(act, G, save_encoder, enc_lp, enc32)
        new = {"act": act, "structs": structs, "enc_lp": enc_lp, "x_final": x, "sig": sig, "owner": None}
        if ent is None or ent["sig"] != sig:
            fwd_cache[key] = new
        return new

    def _run_forward(self, pixels, save_encoder: bool):
        cfg = self.backbone
        G, dev = pixels.shape[0], pixels.device
        P, N, D = cfg.num_patches, cfg.num_tokens, cfg.hidden_size
        le, lh = self.layout.enc, self.layout.head
        enc32, head32 = self.enc_flat.detach(), self.head_flat.detach()
        if save_encoder and self.grad_sink is not None:
            live = self.__dict__.setdefault("_live", [])
            live[:] = [r for r in live if r() is not None]
            if live:
                raise RuntimeError("ContrastViT: a second forward before the first one's backward while a gradient "
                                   "sink (vspike.dp.GradExchange) is attached; the sink reduces one backward per "
                                   "step — use ContrastTrainer.step (one fused 3n forward)")
        ent = self._fwd_buffers(G, dev, save_encoder)
        act, enc_lp = ent["act"], ent["enc_lp"]
        self._refresh_lp(dev)
        table = self._pos_table(dev)
        cols = act["cols"][: G * P]
        # the patch product is the generic path: im2col (one frame, no tubelet) + GEMM with the bias and the
        # table's patch rows in its epilogue, into a compact [G*P, D] tensor
        ops.patch_im2col(pixels.view(G, 1, cfg.num_channels, cfg.image_size, cfg.image_size), cols, 1, cfg.patch_size)
        ops.linear(cols, le.view(enc_lp, "patch_w"), act["patches"], bias=le.view(enc32, "patch_b"),
                   epilogue=L.EPI_POS, pos=table[1:], pos_rows=P)
        ops.cls_embed_fwd(act["patches"], le.view(enc32, "cls"), table, act["x0"].view(G, N, D))
        for s in ent["structs"]:
            ops.vit_layer_fwd(s)
        z = torch.empty(G, self.embed_size, dtype=torch.float32, device=dev)      # handed to the caller
        ops.embed_head_fwd(ent["x_final"], N * D, le.view(enc32, "lnf_g"), le.view(enc32, "lnf_b"), cfg.layer_norm_eps,
                           lh.view(head32, "proj_w"), lh.view(head32, "proj_b"), act["hh"], act["hmean"], act["hrstd"],
                           act["z_raw"], act["hnrm"], z)
        state = _FwdState(act=act, structs=ent["structs"], enc_lp=enc_lp, x_final=ent["x_final"], B=G)
        ent["owner"] = weakref.ref(state)
        if save_encoder and self.grad_sink is not None:
            self.__dict__["_live"].append(weakref.ref(state))
        return z, state

    # ---------------------------------------------------------------------------------------
    # backward
    # ---------------------------------------------------------------------------------------
    def _bwd_scratch(self, G: int, dev):
        cfg, dt = self.backbone, self.compute_dtype
        P, N, D, F, H, E = (cfg.num_patches, cfg.num_tokens, cfg.hidden_size, cfg.intermediate_size,
                            cfg.num_attention_heads, self.embed_size)
        M = G * N
        lp = dt != torch.float32
        _, bwd_cache, _ = self._caches()
        bkey = (G, _dev_key(dev), dt)
        g = bwd_cache.get(bkey)
        if g is None:
            ar = Arena()
            for k, shape, d in (("d_a", (M, F), dt), ("d_h", (M, D), torch.float32), ("dy", (M, D), torch.float32),
                                ("d_o", (M, D), dt), ("d_qkv", (M, 3 * D), dt), ("dxA", (M, D), torch.float32),
                                ("dxB", (M, D), torch.float32), ("d_patch", (G * P, D), dt)):
                ar.add(k, shape, d)
            if lp:
                for k in ("dy_lp", "dxA_lp", "dxB_lp"):
                    ar.add(k, (M, D), dt)
            ar.add("attn_ws", (ops.attn_bwd_workspace_bytes(G, N, H) // 4 + 64,), torch.float32)
            pws = ops.splitk_workspace_bytes(dt, D, cfg.patch_dim, G * P)
            if pws:
                ar.add("patch_ws", (pws // 4 + 64,), torch.float32)
            ar.add("ln_ws", (ops.layernorm_bwd_workspace_bytes(M, D) // 4 + 64,), torch.float32)
            gws = max(ops.splitk_workspace_bytes(dt, m, n, M) for m, n in ((D, F), (F, D), (D, D), (3 * D, D)))
            ar.add("gemm_ws", (gws // 4 + 64,), torch.float32)
            ar.add("head_ws", (ops.embed_head_bwd_workspace_bytes(G, D, E) // 4 + 64,), torch.float32)
            g = ar.allocate(dev)
            bwd_cache[bkey] = g
        return g, bkey

    def _run_backward(self, st, dz):
        cfg = self.backbone
        G = st["B"]
        P, N, D = cfg.num_patches, cfg.num_tokens, cfg.hidden_size
        lay, le, lh = self.layout, self.layout.enc, self.layout.head
        act, dev = st["act"], dz.device
        lp = self.compute_dtype != torch.float32
        enc32, head32 = self.enc_flat.detach(), self.head_flat.detach()
        dz = dz.to(torch.float32).contiguous()
        g, bkey = self._bwd_scratch(G, dev)
        g_head, g_enc = self._grad_buffer(self.head_flat), self._grad_buffer(self.enc_flat)
        Ge = lambda n: le.view(g_enc, n)  # noqa: E731
        # head: normalise', projection', final LayerNorm' into the CLS rows of the last block's dx_out (and
        # its bf16 copy); the other rows get their zeros in the same pass
        ops.embed_head_bwd(dz, st["x_final"], N * D, act["hh"], act["hmean"], act["hrstd"], act["z_raw"], act["hnrm"],
                           le.view(enc32, "lnf_g"), lh.view(head32, "proj_w"), g["dxA"].view(G, N, D),
                           dx_lp=g["dxA_lp"] if lp else None, dw=lh.view(g_head, "proj_w"), db=lh.view(g_head, "proj_b"),
                           dgamma=Ge("lnf_g"), dbeta=Ge("lnf_b"), workspace=g["head_ws"])
        self._ready(self.head_flat, 0, self.head_flat.numel())
        self._ready(self.enc_flat, *lay.final_range)
        dx, _ = self._blocks_backward(st, g, bkey, g_enc)
        # CLS token and patch embedding: d_cls = sum of the CLS rows; dW = d_patch^T cols, db = its column sums
        ops.cls_embed_bwd(dx.view(G, N, D), Ge("cls"), g["d_patch"])
        ops.linear_dw(g["d_patch"], act["cols"][: G * P], Ge("patch_w"), db=Ge("patch_b"), workspace=g.get("patch_ws"))
        self._ready(self.enc_flat, 0, lay.layer_ranges[0][0] if lay.layer_ranges else lay.final_range[0])
        return g_enc, g_head


class _ContrastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pixels, enc_flat, head_flat, mod):
        want = bool(ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        z, st = mod._run_forward(pixels, save_encoder=want)
        ctx.mod, ctx.st = mod, (st if want else None)
        return z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dz):
        mod, st = ctx.mod, ctx.st
        g_enc, g_head = mod._run_backward(st, dz)
        ctx.st = None
        sink = mod.grad_sink
        if sink is not None and hasattr(sink, "end_backward"):
            sink.end_backward()
        if sink is not None and not getattr(sink, "return_grads", False):
            return None, None, None, None      # the sink owns .grad (all-reduced in place)
        return None, g_enc, g_head, None
