"""MAE plugin — drop-in for the reference's `src/model/vit_mae/vit_mae.py:45-94` (NAME2MODEL['MAE'], the model
`src/pretrain.py --model m` selects): HF `ViTMAEForPreTraining` plus the normalised CLS latent.

    patches[g, p] = Conv2d_{k=s=patch}(image g)[p] + table[1 + p]
    shuffle = argsort(noise); restore = argsort(shuffle); keep = shuffle[:, :Lk], Lk = int(P (1 - mask_ratio))
    x[g, 0] = cls + table[0];  x[g, 1 + j] = patches[g, keep[g, j]];  latent = LayerNorm(encoder blocks(x))
    z = latent[:, 0] / |latent[:, 0]|                       # vit_mae.py:54: no projection
    e = decoder_embed(latent);  xd = unshuffle(e, mask_token, restore) + tabd
    logits = decoder_pred(LayerNorm_d(decoder blocks(xd)))[:, 1:]
    recon_loss = sum_masked mean_k (logits - patchify(pixels))^2 / #masked
    return {'z': z, 'recon_loss': recon_loss}

The encoder keeps head dim 64 (vs_attn_fwd / _bwd); the decoder is `decoder_hidden_size = 32 *
decoder_num_attention_heads` wide and runs vs_attn32_fwd / _bwd through the same block executor.  Both position
tables are the fixed 2-D sin-cos table.  The index plumbing (two argsorts of `noise`) stays in torch; everything else
is libvspike: im2col + GEMM, vs_mae_embed_*, the block executor, LayerNorm, vs_mae_dec_assemble_*, vs_mae_recon_loss.

`z` is returned WITHOUT a gradient path: the reference's step for this model uses `recon_loss` only (`loss_fn_`'s first
branch, contrast.py:100-107), so nothing ever differentiates z.  Its one division per image is a torch expression on
the (G, D) CLS rows.  Left out relative to HF: norm_pix_loss, dropout, interpolate_pos_encoding,
learned tables, the key biases (no effect on any output).  Weight-gradient products run in order on the main stream
(set_side_stream(True) raises, for the reason ContrastViT gives); data parallel is not built (a GradExchange raises).
The activation buffers of a forward are allocated per call (no cached arena yet).
"""
from __future__ import annotations

import math
import types
from typing import Optional

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import ops
from .contrast import _V5, sincos_2d_table
from .layout import LAYER_KEYS, FlatLayout, _layer_hf_items, _layer_shapes, modern_name
from .vit import _DTYPES, _cfg_get, _dev_key

_ACT = ("h1", "mean1", "rstd1", "qkv", "attn_o", "lse", "y", "h2", "mean2", "rstd2", "a_pre", "a_act")
_PRE = "vit_mae."


class _Stack:
    """L pre-LN blocks of one width over the block executor: parameter slots `{i}.<LAYER_KEYS>` of one flat layout."""

    def __init__(self, lay: FlatLayout, layers: int, D: int, H: int, F: int, eps: float):
        self.lay, self.layers, self.D, self.H, self.F, self.eps = lay, layers, D, H, F, eps
        self.head_dim = D // H

    def forward(self, x, G: int, N: int, dt, w_lp, w32):
        """Runs the blocks on x [G*N, D] f32; returns (the last block's output, the structs, the saved buffers)."""
        M, D, F, H = G * N, self.D, self.F, self.H
        dev, f32 = x.device, torch.float32
        structs, keep = [], [x]
        for i in range(self.layers):
            act = {k: torch.empty(shape, dtype=d, device=dev) for k, shape, d in (
                ("h1", (M, D), dt), ("mean1", (M,), f32), ("rstd1", (M,), f32), ("qkv", (M, 3 * D), dt),
                ("attn_o", (M, D), dt), ("lse", (G, H, N), f32), ("y", (M, D), f32), ("h2", (M, D), dt),
                ("mean2", (M,), f32), ("rstd2", (M,), f32), ("a_pre", (M, F), dt), ("a_act", (M, F), dt),
                ("x_out", (M, D), f32))}
            s = L.VitLayer()
            s.dtype, s.heads = L.dtype_code(dt), H
            s.batch, s.tokens, s.hidden, s.mlp = G, N, D, F
            s.ln_eps, s.attn_scale = self.eps, 1.0 / math.sqrt(self.head_dim)
            for k in LAYER_KEYS:
                setattr(s, k, self.lay.view(w_lp if k.startswith("w_") else w32, f"{i}.{k}").data_ptr())
            s.x_in, s.x_out = x.data_ptr(), act["x_out"].data_ptr()
            for k in _ACT:
                setattr(s, k, act[k].data_ptr())
            ops.vit_layer_fwd(s)
            structs.append(s)
            keep.append(act)
            x = act["x_out"]
        return x, structs, keep

    def backward(self, structs, dx, dx_lp, G: int, N: int, dt, g_flat):
        """The blocks in reverse from dx [G*N, D] f32 (and its `dt` copy in bf16 mode); weight gradients accumulate
        into g_flat.  Returns the gradient of the first block's input (f32)."""
        M, D, F, H = G * N, self.D, self.F, self.H
        dev, f32, lp = dx.device, torch.float32, dt != torch.float32
        E = lambda shape, d: torch.empty(shape, dtype=d, device=dev)  # noqa: E731
        attn_ws = ops.attn32_bwd_workspace_bytes(G, N, H) if self.head_dim == 32 else ops.attn_bwd_workspace_bytes(G, N, H)
        gws = max(ops.splitk_workspace_bytes(dt, m, n, M) for m, n in ((D, F), (F, D), (D, D), (3 * D, D)))
        sc = {"d_a": E((M, F), dt), "d_h": E((M, D), f32), "dy": E((M, D), f32), "d_o": E((M, D), dt),
              "d_qkv": E((M, 3 * D), dt), "attn_ws": E((attn_ws // 4 + 64,), f32),
              "ln_ws": E((ops.layernorm_bwd_workspace_bytes(M, D) // 4 + 64,), f32), "gemm_ws": E((gws // 4 + 64,), f32),
              "dy_lp": E((M, D), dt) if lp else None}
        for i in reversed(range(self.layers)):
            nxt, nxt_lp = E((M, D), f32), (E((M, D), dt) if lp else None)
            gs = L.VitLayerGrad()
            for k in LAYER_KEYS:
                setattr(gs, k, self.lay.view(g_flat, f"{i}.{k}").data_ptr())
            gs.dx_out, gs.dx_out_lp = dx.data_ptr(), (dx_lp.data_ptr() if lp else None)
            gs.dx_in, gs.dx_in_lp = nxt.data_ptr(), (nxt_lp.data_ptr() if lp else None)
            for k in ("d_a", "d_h", "dy", "d_o", "d_qkv", "attn_ws", "ln_ws", "gemm_ws"):
                setattr(gs, k, sc[k].data_ptr())
            gs.dy_lp = sc["dy_lp"].data_ptr() if lp else None
            gs.gemm_ws_bytes, gs.flags, gs.chain = sc["gemm_ws"].numel() * 4, 0, None    # in order, main stream
            ops.vit_layer_bwd(structs[i], gs)
            dx, dx_lp = nxt, nxt_lp
        return dx


def _both_spellings(key: str, to_v5: bool) -> str:
    """A block parameter's name in the other transformers spelling (4.38 <-> 5.x); other names unchanged."""
    a, b = (".vit.encoder.layer.", ".vit.layers.")
    key = key.replace(a, b) if to_v5 else key.replace(b, a)
    for new, old in _V5:
        src, dst = ("." + old, "." + new) if to_v5 else ("." + new, "." + old)
        if src in key and "layer" in key:
            return key.replace(src, dst)
    return key


class MAE(nn.Module):
    def __init__(self, config):
        super().__init__()
        g = lambda k, d=None: _cfg_get(config, k, d)  # noqa: E731
        self.image_size, self.patch_size = int(g("image_size", 224)), int(g("patch_size", 16))
        self.num_channels = int(g("num_channels", 3))
        D, H = int(g("hidden_size", 768)), int(g("num_attention_heads", 12))
        Dd, Hd = int(g("decoder_hidden_size", 512)), int(g("decoder_num_attention_heads", 16))
        self.eps = float(g("layer_norm_eps", 1e-12))
        cdt = str(g("compute_dtype", "fp32")).lower()
        if cdt in ("fp8", "mxfp8"):
            raise ValueError("MAE: compute_dtype fp8 is not supported (fp32 | bf16)")
        if cdt not in _DTYPES:
            raise ValueError(f"MAE: unknown compute_dtype {cdt!r}")
        self.compute_dtype = _DTYPES[cdt]
        if D != 64 * H:
            raise ValueError("MAE: the encoder needs head dim 64 (hidden_size = 64 * num_attention_heads)")
        if Dd != 32 * Hd:
            raise ValueError("MAE: the decoder needs head dim 32 (decoder_hidden_size = 32 * decoder_num_attention_heads)")
        if bool(g("norm_pix_loss", False)):
            raise ValueError("MAE: norm_pix_loss is not built (the reference sets it false)")
        for k in ("hidden_dropout_prob", "attention_probs_dropout_prob"):
            if float(g(k, 0.0) or 0.0) != 0.0:
                raise ValueError(f"MAE: {k} must be 0 (the kernels have no dropout)")
        if str(g("hidden_act", "gelu")).lower() != "gelu" or not bool(g("qkv_bias", True)):
            raise ValueError("MAE: hidden_act must be gelu and qkv_bias true")
        if self.image_size <= 0 or self.image_size % self.patch_size:
            raise ValueError("MAE: image_size must be a positive multiple of patch_size")
        self.grid = self.image_size // self.patch_size
        self.num_patches = self.grid * self.grid
        if self.num_patches + 1 > 256:
            raise ValueError("MAE: the decoder's head-dim-32 attention takes at most 256 tokens (vs_attn32)")
        self.patch_dim = self.num_channels * self.patch_size ** 2
        F, Fd = int(g("intermediate_size", 3072)), int(g("decoder_intermediate_size", 2048))
        Le, Ld = int(g("num_hidden_layers", 12)), int(g("decoder_num_hidden_layers", 8))
        if self.patch_dim % 8 or F % 8 or Fd % 8 or D % 8 or Dd % 8:
            raise ValueError("MAE: widths and num_channels * patch_size^2 must be multiples of 8")
        self.hidden_size, self.decoder_hidden_size = D, Dd
        # live: read on every call; the reference trainer sets it to 0 around transform (contrast.py:177-202)
        self.config = types.SimpleNamespace(mask_ratio=float(g("mask_ratio", 0.75)))
        e = FlatLayout()
        e.add("patch_w", (D, self.patch_dim)); e.add("patch_b", (D,)); e.add("cls", (D,))
        for i in range(Le):
            for k, shape in _layer_shapes(D, F):
                e.add(f"{i}.{k}", shape)
        e.add("lnf_g", (D,)); e.add("lnf_b", (D,))
        d = FlatLayout()
        d.add("embed_w", (Dd, D)); d.add("embed_b", (Dd,)); d.add("mask_token", (Dd,))
        for i in range(Ld):
            for k, shape in _layer_shapes(Dd, Fd):
                d.add(f"{i}.{k}", shape)
        d.add("norm_g", (Dd,)); d.add("norm_b", (Dd,))
        d.add("pred_w", (self.patch_dim, Dd)); d.add("pred_b", (self.patch_dim,))
        self.layout = types.SimpleNamespace(enc=e, dec=d)
        self.enc_stack = _Stack(e, Le, D, H, F, self.eps)
        self.dec_stack = _Stack(d, Ld, Dd, Hd, Fd, self.eps)
        self.enc_flat = nn.Parameter(torch.zeros(e.numel))
        self.dec_flat = nn.Parameter(torch.zeros(d.numel))
        self.__dict__["_tables"] = {}
        self.reset_parameters()

    # ---------------------------------------------------------------------------------------------------
    # parameters
    # ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def reset_parameters(self, generator: Optional[torch.Generator] = None):
        """HF ViTMAE's init: N(0, 0.02) Linear weights, CLS token and mask token, zero biases, LayerNorm (1, 0), the
        patch projection xavier-uniform as a Linear."""
        for flat, lay in ((self.enc_flat, self.layout.enc), (self.dec_flat, self.layout.dec)):
            flat.zero_()
            for name, slot in lay.slots.items():
                v = lay.view(flat, name)
                if name.endswith(("ln1_g", "ln2_g", "lnf_g", "norm_g")):
                    v.fill_(1.0)
                elif name == "patch_w":
                    bound = math.sqrt(6.0 / (slot.shape[0] + slot.shape[1]))
                    v.uniform_(-bound, bound, generator=generator)
                elif name in ("cls", "mask_token") or len(slot.shape) == 2:
                    v.normal_(0.0, 0.02, generator=generator)

    @property
    def grad_sink(self):
        return None

    @grad_sink.setter
    def grad_sink(self, sink):
        if sink is not None:
            raise NotImplementedError("MAE: data parallel is not built for this plugin (no GradExchange)")

    def set_side_stream(self, enabled: bool) -> None:
        if enabled:
            raise ValueError("MAE runs its weight-gradient products in order; the side stream is not available for "
                             "this plugin (DESIGN.md section 7)")

    def hf_items(self):
        """(reference name, which flat, slot, row slice, shape under that name)."""
        D, Dd, C, p = self.hidden_size, self.decoder_hidden_size, self.num_channels, self.patch_size
        yield _PRE + "vit.embeddings.cls_token", "enc", "cls", None, (1, 1, D)
        yield _PRE + "vit.embeddings.patch_embeddings.projection.weight", "enc", "patch_w", None, (D, C, p, p)
        yield _PRE + "vit.embeddings.patch_embeddings.projection.bias", "enc", "patch_b", None, None
        for i in range(self.enc_stack.layers):
            for name, which, slot, rows in _layer_hf_items(f"{_PRE}vit.encoder.layer.{i}.", "enc", i, D):
                yield modern_name(name), which, slot, rows, None
        yield _PRE + "vit.layernorm.weight", "enc", "lnf_g", None, None
        yield _PRE + "vit.layernorm.bias", "enc", "lnf_b", None, None
        yield _PRE + "decoder.decoder_embed.weight", "dec", "embed_w", None, None
        yield _PRE + "decoder.decoder_embed.bias", "dec", "embed_b", None, None
        yield _PRE + "decoder.mask_token", "dec", "mask_token", None, (1, 1, Dd)
        for i in range(self.dec_stack.layers):
            for name, which, slot, rows in _layer_hf_items(f"{_PRE}decoder.decoder_layers.{i}.", "dec", i, Dd):
                yield modern_name(name), which, slot, rows, None
        yield _PRE + "decoder.decoder_norm.weight", "dec", "norm_g", None, None
        yield _PRE + "decoder.decoder_norm.bias", "dec", "norm_b", None, None
        yield _PRE + "decoder.decoder_pred.weight", "dec", "pred_w", None, None
        yield _PRE + "decoder.decoder_pred.bias", "dec", "pred_b", None, None

    def _flat(self, which):
        return (self.enc_flat, self.layout.enc) if which == "enc" else (self.dec_flat, self.layout.dec)

    def _table64(self, dim):
        return sincos_2d_table(dim, self.grid)

    def reference_state_dict(self, modern_names: bool = False):
        """Parameters under the reference module's names (`vit_mae.vit.*`, `vit_mae.decoder.*`; transformers 4.38 block
        names, or 5.x with `modern_names`).  `key.bias` is exported as zeros, the two tables as the fixed table."""
        out = {}
        for name, which, slot, rows, shape in self.hf_items():
            flat, lay = self._flat(which)
            t = lay.view(flat.detach(), slot)
            t = (t if rows is None else t[rows]).clone()
            out[name] = t.view(shape) if shape else t
        for stack, pfx, D in ((self.enc_stack, "vit.encoder.layer.", self.hidden_size),
                              (self.dec_stack, "decoder.decoder_layers.", self.decoder_hidden_size)):
            for i in range(stack.layers):
                out[f"{_PRE}{pfx}{i}.attention.attention.key.bias"] = torch.zeros(D)
        out[_PRE + "vit.embeddings.position_embeddings"] = torch.from_numpy(
            self._table64(self.hidden_size).astype(np.float32))[None]
        out[_PRE + "decoder.decoder_pos_embed"] = torch.from_numpy(
            self._table64(self.decoder_hidden_size).astype(np.float32))[None]
        if modern_names:
            out = {_both_spellings(k, True): v for k, v in out.items()}
        return out

    @torch.no_grad()
    def load_reference_state_dict(self, sd, strict: bool = True):
        """Load a reference `MAE` state_dict (either spelling).  Any `key.bias` is accepted and ignored; a position
        table that differs from the fixed one by more than 1e-6 is refused."""
        sd = {_both_spellings(k, False): v for k, v in sd.items()}
        seen = set()
        for name, which, slot, rows, _ in self.hf_items():
            if name not in sd:
                if strict:
                    raise KeyError(f"missing {name}")
                continue
            flat, lay = self._flat(which)
            dst = lay.view(flat, slot)
            dst = dst[rows] if rows is not None else dst
            dst.copy_(torch.as_tensor(sd[name]).to(dst.device, torch.float32).reshape(dst.shape))
            seen.add(name)
        tables = {_PRE + "vit.embeddings.position_embeddings": self.hidden_size,
                  _PRE + "decoder.decoder_pos_embed": self.decoder_hidden_size}
        for k, v in sd.items():
            if k.endswith("attention.attention.key.bias"):
                seen.add(k)
            elif k in tables:
                t = torch.as_tensor(v).to("cpu", torch.float64).reshape(-1, tables[k])
                ref = torch.from_numpy(self._table64(tables[k]))
                if t.shape != ref.shape or (t - ref).abs().max().item() > 1e-6:
                    raise ValueError(f"{k} is not the fixed 2-D sin-cos table (a learned one cannot be loaded)")
                seen.add(k)
        if strict and set(sd) - seen:
            raise KeyError(f"unexpected keys: {sorted(set(sd) - seen)[:5]}")

    # ---------------------------------------------------------------------------------------------------
    # forward / backward
    # ---------------------------------------------------------------------------------------------------
    def _table(self, dim, dev):
        key = (dim, _dev_key(dev))
        if key not in self._tables:
            self._tables[key] = torch.from_numpy(self._table64(dim).astype(np.float32)).to(dev)
        return self._tables[key]

    def forward(self, x: torch.Tensor, noise: Optional[torch.Tensor] = None):
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.num_channels, self.image_size, self.image_size):
            raise ValueError(f"MAE expects (G, {self.num_channels}, {self.image_size}, {self.image_size})")
        L.require_device(x)
        pixels = x.detach().to(torch.float32).contiguous()
        G, P = pixels.shape[0], self.num_patches
        keep_n = int(P * (1 - float(self.config.mask_ratio)))
        if keep_n >= P:            # mask_ratio 0: every patch in natural order, no decoder; HF's loss is 0 / 0
            with torch.no_grad():
                z = self._run_forward(pixels, None, None, P, False)[0]
            return {"z": z, "recon_loss": torch.full((), float("nan"), device=x.device)}
        if keep_n < 1:
            raise ValueError("MAE: mask_ratio leaves no patch")
        if noise is None:
            noise = torch.rand(G, P, device=x.device)
        if tuple(noise.shape) != (G, P):
            raise ValueError(f"MAE: noise must be ({G}, {P})")
        shuffle = torch.argsort(noise.to(x.device), dim=1)
        restore = torch.argsort(shuffle, dim=1).to(torch.int32).contiguous()
        keep = shuffle[:, :keep_n].to(torch.int32).contiguous()
        z, loss = _MAEFn.apply(pixels, keep, restore, self.enc_flat, self.dec_flat, self)
        return {"z": z, "recon_loss": loss}

    def _weights(self, dev):
        enc32, dec32 = self.enc_flat.detach(), self.dec_flat.detach()
        if self.compute_dtype == torch.float32:
            return enc32, dec32, enc32, dec32
        enc_lp = torch.empty(enc32.numel(), dtype=self.compute_dtype, device=dev)
        dec_lp = torch.empty(dec32.numel(), dtype=self.compute_dtype, device=dev)
        ops.cast(enc32, enc_lp)
        ops.cast(dec32, dec_lp)
        return enc32, dec32, enc_lp, dec_lp

    def _run_forward(self, pixels, keep, restore, Lk: int, train: bool):
        G, dev, dt, f32 = pixels.shape[0], pixels.device, self.compute_dtype, torch.float32
        P, D, Dd, K = self.num_patches, self.hidden_size, self.decoder_hidden_size, self.patch_dim
        le, ld = self.layout.enc, self.layout.dec
        enc32, dec32, enc_lp, dec_lp = self._weights(dev)
        E = lambda shape, d: torch.empty(shape, dtype=d, device=dev)  # noqa: E731
        table = self._table(D, dev)
        cols, patches = E((G * P, K), dt), E((G * P, D), f32)
        ops.patch_im2col(pixels.view(G, 1, self.num_channels, self.image_size, self.image_size), cols, 1, self.patch_size)
        ops.linear(cols, le.view(enc_lp, "patch_w"), patches, bias=le.view(enc32, "patch_b"), epilogue=L.EPI_POS,
                   pos=table[1:], pos_rows=P)
        Ne = Lk + 1
        x0 = E((G, Ne, D), f32)
        if keep is None:
            ops.cls_embed_fwd(patches, le.view(enc32, "cls"), table, x0)
        else:
            ops.mae_embed_fwd(patches, keep, le.view(enc32, "cls"), table, x0)
        xe, e_structs, e_keep = self.enc_stack.forward(x0.view(G * Ne, D), G, Ne, dt, enc_lp, enc32)
        latent, lmean, lrstd = E((G * Ne, D), dt), E((G * Ne,), f32), E((G * Ne,), f32)
        ops.layernorm_fwd(xe, le.view(enc32, "lnf_g"), le.view(enc32, "lnf_b"), self.eps, latent, lmean, lrstd)
        h = latent.view(G, Ne, D)[:, 0].to(f32)
        z = h / h.norm(dim=-1, keepdim=True)
        if keep is None:
            return z, None, None
        e = E((G, Ne, Dd), f32)
        ops.linear(latent, ld.view(dec_lp, "embed_w"), e.view(G * Ne, Dd), bias=ld.view(dec32, "embed_b"))
        Nd = P + 1
        xd0 = E((G, Nd, Dd), f32)
        ops.mae_dec_assemble_fwd(e, restore, ld.view(dec32, "mask_token"), self._table(Dd, dev), xd0)
        xd, d_structs, d_keep = self.dec_stack.forward(xd0.view(G * Nd, Dd), G, Nd, dt, dec_lp, dec32)
        hd, dmean, drstd = E((G * Nd, Dd), dt), E((G * Nd,), f32), E((G * Nd,), f32)
        ops.layernorm_fwd(xd, ld.view(dec32, "norm_g"), ld.view(dec32, "norm_b"), self.eps, hd, dmean, drstd)
        pred = E((G, Nd, K), f32)
        ops.linear(hd, ld.view(dec_lp, "pred_w"), pred.view(G * Nd, K), bias=ld.view(dec32, "pred_b"))
        loss, d_pred = E((1,), f32), E((G, Nd, K), dt)
        ws = E((ops.mae_recon_loss_workspace_bytes(G, P) // 4 + 4,), f32)
        ops.mae_recon_loss(pred, pixels, restore, Lk, self.patch_size, loss, d_pred, ws)
        st = None
        if train:
            st = dict(G=G, Lk=Lk, cols=cols, keep=keep, restore=restore, e_structs=e_structs, e_keep=e_keep, xe=xe,
                      latent=latent, lmean=lmean, lrstd=lrstd, d_structs=d_structs, d_keep=d_keep, xd=xd, hd=hd,
                      dmean=dmean, drstd=drstd, d_pred=d_pred, enc_lp=enc_lp, dec_lp=dec_lp, x0=x0, xd0=xd0)
        return z, loss.view(()), st

    def _run_backward(self, st, dloss):
        G, Lk, dt, f32 = st["G"], st["Lk"], self.compute_dtype, torch.float32
        P, D, Dd, K = self.num_patches, self.hidden_size, self.decoder_hidden_size, self.patch_dim
        le, ld = self.layout.enc, self.layout.dec
        enc32, dec32 = self.enc_flat.detach(), self.dec_flat.detach()
        dev, lp = enc32.device, dt != torch.float32
        Ne, Nd = Lk + 1, P + 1
        g_enc, g_dec = torch.zeros_like(enc32), torch.zeros_like(dec32)
        Ge, Gd = (lambda n: le.view(g_enc, n)), (lambda n: ld.view(g_dec, n))  # noqa: E731
        E = lambda shape, d: torch.empty(shape, dtype=d, device=dev)  # noqa: E731
        # decoder_pred and decoder_norm
        d_pred = st["d_pred"].view(G * Nd, K)
        ops.linear_dw(d_pred, st["hd"], Gd("pred_w"), db=Gd("pred_b"))
        d_hd = E((G * Nd, Dd), f32)
        ops.linear_dx(d_pred, ld.view(st["dec_lp"], "pred_w"), d_hd)
        dxd, dxd_lp = E((G * Nd, Dd), f32), (E((G * Nd, Dd), dt) if lp else None)
        ops.layernorm_bwd(d_hd, st["xd"], st["dmean"], st["drstd"], ld.view(dec32, "norm_g"), dxd, Gd("norm_g"),
                          Gd("norm_b"), dx_lp=dxd_lp)
        dxd0 = self.dec_stack.backward(st["d_structs"], dxd, dxd_lp, G, Nd, dt, g_dec)
        # decoder assembly and decoder_embed
        d_e = E((G, Ne, Dd), dt)
        ws = E((ops.mae_dec_assemble_bwd_workspace_bytes(G, Dd) // 4 + 4,), f32)
        ops.mae_dec_assemble_bwd(dxd0.view(G, Nd, Dd), st["keep"], st["restore"], d_e, Gd("mask_token"), ws)
        d_e2 = d_e.view(G * Ne, Dd)
        ops.linear_dw(d_e2, st["latent"], Gd("embed_w"), db=Gd("embed_b"))
        d_lat = E((G * Ne, D), f32)
        ops.linear_dx(d_e2, ld.view(st["dec_lp"], "embed_w"), d_lat)
        # the encoder's final LayerNorm, its blocks, the masked gather and the patch projection
        dxe, dxe_lp = E((G * Ne, D), f32), (E((G * Ne, D), dt) if lp else None)
        ops.layernorm_bwd(d_lat, st["xe"], st["lmean"], st["lrstd"], le.view(enc32, "lnf_g"), dxe, Ge("lnf_g"),
                          Ge("lnf_b"), dx_lp=dxe_lp)
        dx0 = self.enc_stack.backward(st["e_structs"], dxe, dxe_lp, G, Ne, dt, g_enc)
        d_patch = E((G * P, D), dt)
        ops.mae_embed_bwd(dx0.view(G, Ne, D), st["restore"], Ge("cls"), d_patch)
        ops.linear_dw(d_patch, st["cols"], Ge("patch_w"), db=Ge("patch_b"))
        # the loss kernel wrote d(loss)/d(pred); every product above is linear in it
        g_enc.mul_(dloss)
        g_dec.mul_(dloss)
        return g_enc, g_dec


class _MAEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pixels, keep, restore, enc_flat, dec_flat, mod):
        want = bool(ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        z, loss, st = mod._run_forward(pixels, keep, restore, keep.shape[1], want)
        ctx.mod, ctx.st = mod, st
        ctx.mark_non_differentiable(z)
        return z, loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dz, dloss):
        g_enc, g_dec = ctx.mod._run_backward(ctx.st, dloss.to(torch.float32))
        ctx.st = None
        return None, None, None, g_enc, g_dec, None
