"""VideoMAETemporal plugin — BASELINE C5's "ViT + temporal transformer" (NAME2MODEL['VideoMAETemporal']).

The reference has no code for this stage, so the model is defined here and in
DESIGN.md section 7, and checked against a CPU restatement (tests/temporal_ref.py); parity with any
reference output is unpinned, like the R3D encoder's.  With X (B, T'*S, D) the VideoMAE encoder's
output (T' = num_frames / tubelet_size time steps of S = (image_size / patch_size)^2 tokens, t-major):

    P[b, t] = mean_s X[b, t*S + s] + sinusoid_table(T', D)[t]        # vs_token_pool_fwd, no parameter
    for j in range(L_t): P = VideoMAELayer_j(P)                       # the encoder's pre-LN block, T' tokens
    z = P.flatten(1) @ enc_w.T + enc_b;  r = z @ dec_w.T + dec_b      # head over T'*D instead of T'*S*D

Config: the VideoMAE plugin's keys plus `temporal: {num_layers: L_t, intermediate_size: F_t}` (F_t
defaults to the backbone's intermediate_size; L_t = 0 is a pooled head only).

Everything of the encoder is the VideoMAE plugin's (this class subclasses it: same flat encoder
buffer, names, kernels and backward sequencing).  The temporal blocks live in a third flat f32 buffer
`temp_flat` (always trainable: `freeze_encoder` freezes `enc_flat` only) and run through the same
block executor with batch = B, tokens = T'.  Under `compute_dtype: fp8` they run in bf16: B*T' rows are
too few to repay the operand quantisation, and the MX-FP8 workspace is sized for the encoder.
The backward is hand-sequenced: head, temporal blocks in reverse on the main stream, then (trainable
encoder only) vs_token_pool_bwd writes the gradient of the encoder output straight into the last
encoder block's dx_out / dx_out_lp pair and the VideoMAE encoder backward follows.
"""
from __future__ import annotations

import math
import weakref
from typing import Optional

import torch
from torch import nn

from . import _lib as L
from . import ops
from .layout import LAYER_KEYS, TemporalLayout
from .memory import Arena
from .vit import VideoMAE, _FwdState, _cfg_get, _dev_key

_ACT_KEYS = ("h1", "mean1", "rstd1", "qkv", "attn_o", "lse", "y", "h2", "mean2", "rstd2", "a_pre", "a_act")


class VideoMAETemporal(VideoMAE):
    # the flat parameter buffers whose gradients the data-parallel sink owns (vspike.dp.GradExchange)
    SUNK_BUFFERS = ("enc_flat", "temp_flat", "head_flat")

    def __init__(self, config):
        super().__init__(config)
        self.temp_flat = nn.Parameter(torch.zeros(self.layout.temp.numel))
        self._reset_temporal()

    def _make_layout(self, config, enc_out: int, out_dim: int):
        cfg = self.backbone
        t = _cfg_get(config, "temporal", None) or {}
        layers = int(_cfg_get(t, "num_layers", 0) or 0)
        mlp = int(_cfg_get(t, "intermediate_size", None) or cfg.intermediate_size)
        if layers < 0 or mlp <= 0 or mlp % 8:
            raise ValueError("temporal.num_layers must be >= 0 and temporal.intermediate_size a positive multiple of 8")
        if cfg.hidden_size % 64:
            raise ValueError("the token pool needs hidden_size % 64 == 0")
        return TemporalLayout(cfg, enc_out, out_dim, layers, mlp)

    # ---------------------------------------------------------------------------------------
    # parameters
    # ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def _reset_temporal(self, generator: Optional[torch.Generator] = None):
        """The encoder's block init (HF `_init_weights`): N(0, 0.02) weights, zero biases, LayerNorm (1, 0)."""
        lay, t = self.layout.temp, self.temp_flat
        t.zero_()
        for name, slot in lay.slots.items():
            v = lay.view(t, name)
            if name.endswith(("ln1_g", "ln2_g")):
                v.fill_(1.0)
            elif len(slot.shape) == 2:
                v.normal_(0.0, 0.02, generator=generator)

    @torch.no_grad()
    def reset_parameters(self, generator: Optional[torch.Generator] = None):
        super().reset_parameters(generator)
        if "temp_flat" in self._parameters:     # not yet while VideoMAE.__init__ runs
            self._reset_temporal(generator)

    def _flat(self, which):
        return self.temp_flat if which == "temp" else super()._flat(which)

    def _flat_layout(self, which):
        return self.layout.temp if which == "temp" else super()._flat_layout(which)

    def _flat_params(self):
        return (("enc", self.enc_flat), ("temp", self.temp_flat), ("head", self.head_flat))

    @torch.no_grad()
    def load_reference_state_dict(self, sd, strict: bool = True):
        """As VideoMAE's.  With strict=False a checkpoint of the plain VideoMAE plugin (its
        `encoder.weight` spans all T'*S tokens) or of the bare videomae-base encoder fills the encoder
        slots only: the other model's head is not loaded, temporal blocks and head stay as they are."""
        if not strict:
            w = sd.get("encoder.weight")
            if w is not None and torch.as_tensor(w).numel() != self.layout.head.slots["enc_w"].numel:
                sd = {k: v for k, v in sd.items() if not k.startswith(("encoder.", "decoder."))}
        super().load_reference_state_dict(sd, strict)

    # ---------------------------------------------------------------------------------------
    # forward
    # ---------------------------------------------------------------------------------------
    def _apply_fn(self, pixels):
        return _TemporalFn.apply(pixels, self.enc_flat, self.temp_flat, self.head_flat, self)

    def _time_table(self, device):
        key = ("time", _dev_key(device))
        if key not in self._pos_cache:
            self._pos_cache[key] = ops.sinusoid_table(self.layout.time_steps, self.backbone.hidden_size, device)
        return self._pos_cache[key]

    def _temp_struct(self, j, B, x_in, x_out, act, pfx, w_lp, w32):
        cfg, lay = self.backbone, self.layout
        s = L.VitLayer()
        s.dtype = L.dtype_code(self.compute_dtype)     # bf16 under fp8 too (module docstring)
        s.heads = cfg.num_attention_heads
        s.batch, s.tokens, s.hidden, s.mlp = B, lay.time_steps, cfg.hidden_size, lay.temporal_mlp
        s.ln_eps = cfg.layer_norm_eps
        s.attn_scale = 1.0 / math.sqrt(64.0)
        for k in LAYER_KEYS:
            setattr(s, k, lay.temp.view(w_lp if k.startswith("w_") else w32, f"{j}.{k}").data_ptr())
        s.x_in, s.x_out = x_in.data_ptr(), x_out.data_ptr()
        for k in _ACT_KEYS:
            setattr(s, k, act[pfx + k].data_ptr())
        return s

    def _fwd_buffers(self, B: int, dev, save_encoder: bool):
        """VideoMAE._fwd_buffers with the temporal stage's buffers and the T'*D head in place of the
        T'*S*D one (same caching rules)."""
        fwd_cache, _, _ = self._caches()
        enc32, temp32, head32 = self.enc_flat.detach(), self.temp_flat.detach(), self.head_flat.detach()
        sig = (enc32.data_ptr(), temp32.data_ptr(), head32.data_ptr())
        key = (B, _dev_key(dev), save_encoder, self.compute_dtype)
        ent = fwd_cache.get(key)
        if ent is not None and ent["sig"] == sig and (ent["owner"] is None or ent["owner"]() is None):
            return ent
        cfg, lay, dt = self.backbone, self.layout, self.compute_dtype
        D, H, T, Ft, Lt = cfg.hidden_size, cfg.num_attention_heads, lay.time_steps, lay.temporal_mlp, lay.temporal_layers
        Mt = B * T
        lp = dt != torch.float32
        ar = Arena()
        fused = self._plan_encoder(ar, B, save_encoder)
        ar.add("P0", (Mt, D), torch.float32)
        for j in range(Lt):
            for name, shape, d in (("h1", (Mt, D), dt), ("mean1", (Mt,), torch.float32), ("rstd1", (Mt,), torch.float32),
                                   ("qkv", (Mt, 3 * D), dt), ("attn_o", (Mt, D), dt), ("lse", (B, H, T), torch.float32),
                                   ("y", (Mt, D), torch.float32), ("h2", (Mt, D), dt), ("mean2", (Mt,), torch.float32),
                                   ("rstd2", (Mt,), torch.float32), ("a_pre", (Mt, Ft), dt), ("a_act", (Mt, Ft), dt)):
                ar.add(f"T{j}.{name}", shape, d)
            ar.add(f"P{j + 1}", (Mt, D), torch.float32)
        if lp:
            ar.add("p_lp", (B, T * D), dt)
        ar.add("z", (B, lay.enc_out), torch.float32)
        hws = ops.splitk_workspace_bytes(dt, B, lay.enc_out, T * D)
        if hws:
            ar.add("head_ws", (hws // 4 + 4,), torch.float32)
        act = ar.allocate(dev)
        if lp:
            sh = self._lp_shadows(dev)
            enc_lp, temp_lp, head_lp = sh["enc"][0], sh["temp"][0], sh["head"][0]
        else:
            enc_lp, temp_lp, head_lp = enc32, temp32, head32
        structs, x = self._encoder_structs(act, B, save_encoder, enc_lp, enc32)
        tstructs = [self._temp_struct(j, B, act[f"P{j}"], act[f"P{j + 1}"], act, f"T{j}.", temp_lp, temp32)
                    for j in range(Lt)]
        p_final = act[f"P{Lt}"]
        new = {"act": act, "structs": structs, "tstructs": tstructs, "enc_lp": enc_lp, "head_lp": head_lp,
               "x_final": x, "fused": fused, "p_flat_lp": act["p_lp"] if lp else p_final.view(B, T * D),
               "p_final": p_final, "head_ws": act.get("head_ws"), "sig": sig, "owner": None}
        if ent is None or ent["sig"] != sig:
            fwd_cache[key] = new
        return new

    def _run_forward(self, pixels, save_encoder: bool):
        cfg, lay, dt = self.backbone, self.layout, self.compute_dtype
        B, dev = pixels.shape[0], pixels.device
        D, T = cfg.hidden_size, lay.time_steps
        head32, lh = self.head_flat.detach(), lay.head
        ent = self._fwd_buffers(B, dev, save_encoder)
        act, head_lp = ent["act"], ent["head_lp"]
        self._refresh_lp(dev)
        self._encoder_forward(ent, pixels)
        # one token per time step (+ the T'-row sinusoid table): reads the encoder output once
        ops.token_pool_fwd(ent["x_final"], cfg.num_tokens // T, act["P0"], pos=self._time_table(dev))
        for s in ent["tstructs"]:
            ops.vit_layer_fwd(s)
        p_flat_lp = ent["p_flat_lp"]
        if dt != torch.float32:
            ops.cast(ent["p_final"].view(B, T * D), p_flat_lp)
        z = act["z"]
        r = torch.empty(B, lay.out_dim, dtype=torch.float32, device=dev)   # handed to the caller
        z.zero_()
        ops.gemm(p_flat_lp, lh.view(head_lp, "enc_w"), z, M=B, N=lay.enc_out, K=T * D, a_kcontig=True, b_kcontig=True,
                 lda=T * D, ldb=T * D, ldc=lay.enc_out, epilogue=L.EPI_ATOMIC | L.EPI_BIAS,
                 bias=lh.view(head32, "enc_b"), workspace=ent["head_ws"])
        ops.linear(z, lh.view(head32, "dec_w"), r, bias=lh.view(head32, "dec_b"))
        # a frozen encoder keeps no per-layer encoder activations, and its pixels are not read again
        keep_px = save_encoder and "cols" not in act
        state = _FwdState(act=act, structs=ent["structs"], tstructs=ent["tstructs"], enc_lp=ent["enc_lp"],
                          head_lp=head_lp, x_flat_lp=p_flat_lp, x_final=ent["x_final"], B=B,
                          pixels=pixels if keep_px else None, pixels_version=pixels._version)
        ent["owner"] = weakref.ref(state)
        return r.view(B, 100, -1), state

    # ---------------------------------------------------------------------------------------
    # backward
    # ---------------------------------------------------------------------------------------
    def _temp_scratch(self, B: int, dev):
        """Scratch of the head's and the temporal blocks' backward (B*T' rows: small), one set per shape."""
        cfg, lay, dt = self.backbone, self.layout, self.compute_dtype
        D, H, T, Ft = cfg.hidden_size, cfg.num_attention_heads, lay.time_steps, lay.temporal_mlp
        Mt = B * T
        lp = dt != torch.float32
        _, bwd_cache, _ = self._caches()
        tkey = ("temporal", B, _dev_key(dev), dt)
        g = bwd_cache.get(tkey)
        if g is None:
            ar = Arena()
            for k, shape, d in (("d_a", (Mt, Ft), dt), ("d_h", (Mt, D), torch.float32), ("dy", (Mt, D), torch.float32),
                                ("d_o", (Mt, D), dt), ("d_qkv", (Mt, 3 * D), dt), ("dpA", (Mt, D), torch.float32),
                                ("dpB", (Mt, D), torch.float32), ("dz", (B, lay.enc_out), torch.float32)):
                ar.add(k, shape, d)
            if lp:
                for k in ("dy_lp", "dpA_lp", "dpB_lp"):
                    ar.add(k, (Mt, D), dt)
                ar.add("dz_lp", (B, lay.enc_out), dt)
            ar.add("attn_ws", (ops.attn_bwd_workspace_bytes(B, T, H) // 4 + 64,), torch.float32)
            ar.add("dz_ws", (max(ops.splitk_workspace_bytes(torch.float32, B, lay.enc_out, lay.out_dim), 16) // 4 + 64,),
                   torch.float32)
            ar.add("ln_ws", (ops.layernorm_bwd_workspace_bytes(Mt, D) // 4 + 64,), torch.float32)
            gws = max(ops.splitk_workspace_bytes(dt, m, n, Mt) for m, n in ((D, Ft), (Ft, D), (D, D), (3 * D, D)))
            ar.add("gemm_ws", (gws // 4 + 64,), torch.float32)
            g = ar.allocate(dev)
            bwd_cache[tkey] = g
        return g, tkey

    def _temp_grad_structs(self, g, tkey, g_temp):
        lay = self.layout
        lp = self.compute_dtype != torch.float32
        gs_cache = self._caches()[2]
        gkey = (tkey, g_temp.data_ptr())
        grads = gs_cache.get(gkey)
        if grads is None:
            if len(gs_cache) > 8:
                gs_cache.clear()
            grads = {}
            cur = "dpA"
            for j in reversed(range(lay.temporal_layers)):
                gs = L.VitLayerGrad()
                for k in LAYER_KEYS:
                    setattr(gs, k, lay.temp.view(g_temp, f"{j}.{k}").data_ptr())
                nxt = "dpB" if cur == "dpA" else "dpA"
                gs.dx_out, gs.dx_out_lp = g[cur].data_ptr(), (g[cur + "_lp"].data_ptr() if lp else None)
                gs.dx_in, gs.dx_in_lp = g[nxt].data_ptr(), (g[nxt + "_lp"].data_ptr() if lp else None)
                gs.d_a, gs.d_h, gs.dy = g["d_a"].data_ptr(), g["d_h"].data_ptr(), g["dy"].data_ptr()
                gs.dy_lp = g["dy_lp"].data_ptr() if lp else None
                gs.d_o, gs.d_qkv, gs.attn_ws = g["d_o"].data_ptr(), g["d_qkv"].data_ptr(), g["attn_ws"].data_ptr()
                gs.ln_ws = g["ln_ws"].data_ptr()
                # every product in order on the main stream: B*T' rows leave nothing to overlap
                gs.chain, gs.flags = None, 0
                gs.gemm_ws, gs.gemm_ws_bytes = g["gemm_ws"].data_ptr(), g["gemm_ws"].numel() * 4
                grads[j] = (gs, nxt)
                cur = nxt
            gs_cache[gkey] = grads
        return grads

    def _run_backward(self, st, d_logrates, want_enc: bool, want_temp: bool, want_head: bool):
        cfg, lay, dt = self.backbone, self.layout, self.compute_dtype
        B = st["B"]
        D, T = cfg.hidden_size, lay.time_steps
        lh = lay.head
        act = st["act"]
        dev = d_logrates.device
        head32 = self.head_flat.detach()
        dr = d_logrates.reshape(B, lay.out_dim).to(torch.float32).contiguous()
        lp = dt != torch.float32
        g, tkey = self._temp_scratch(B, dev)

        # ---- head (as VideoMAE's, K = T'*D)
        g_head = self._grad_buffer(self.head_flat) if want_head else None
        Gh = lambda n: lh.view(g_head, n)  # noqa: E731
        z, dz = act["z"], g["dz"]
        dz.zero_()
        ops.linear_dx(dr, lh.view(head32, "dec_w"), dz, accumulate=True, workspace=g["dz_ws"])
        if lp:
            dz_lp = g["dz_lp"]
            ops.cast(dz, dz_lp)
        else:
            dz_lp = dz
        if want_head:
            ops.linear_dw(dr, z, Gh("dec_w"), db=Gh("dec_b"))
            ops.colsum(dz, Gh("enc_b"))
            ops.linear_dw(dz_lp, st["x_flat_lp"], Gh("enc_w"), accumulate=False)
            self._ready(self.head_flat, 0, self.head_flat.numel())
        if not (want_enc or want_temp):
            return None, None, g_head

        # ---- temporal blocks in reverse (their gradients go to the sink before the encoder's)
        cur = "dpA"
        ops.linear_dx(dz_lp, lh.view(st["head_lp"], "enc_w"), g[cur].view(B, T * D))
        if lp and lay.temporal_layers:
            ops.cast(g[cur], g[cur + "_lp"])
        # gradients of frozen temporal blocks are computed into a throw-away buffer (dX needs the pass)
        g_temp = self._grad_buffer(self.temp_flat) if want_temp else torch.zeros_like(self.temp_flat)
        grads = self._temp_grad_structs(g, tkey, g_temp)
        for j in reversed(range(lay.temporal_layers)):
            gs, cur = grads[j]
            ops.vit_layer_bwd(st["tstructs"][j], gs)
            if want_temp:
                self._ready(self.temp_flat, *lay.temp_ranges[j])
        if not want_temp:
            g_temp = None
        if not want_enc:      # frozen encoder: no pool backward
            return None, g_temp, g_head

        # ---- pool backward straight into the last encoder block's dx_out / dx_out_lp, then the encoder
        ge, bkey = self._bwd_scratch(B, dev)
        g_enc = self._grad_buffer(self.enc_flat)
        ops.token_pool_bwd(g[cur], cfg.num_tokens // T, ge["dxA"], ge["dxA_lp"] if lp else None)
        self._encoder_backward(st, ge, bkey, g_enc)
        return g_enc, g_temp, g_head


class _TemporalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pixels, enc_flat, temp_flat, head_flat, mod):
        want = tuple(bool(ctx.needs_input_grad[i]) for i in (1, 2, 3))
        if mod.temp_flat.numel() == 0:          # temporal.num_layers 0: an empty buffer has no gradient
            want = (want[0], False, want[2])
        out, st = mod._run_forward(pixels, save_encoder=want[0])
        ctx.want = want
        ctx.mod, ctx.st = mod, (st if any(want) else None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        mod, st = ctx.mod, ctx.st
        if st is not None and st.get("pixels") is not None and st["pixels"]._version != st["pixels_version"]:
            # as VideoMAE: the cols-free patch dW gathers the caller's pixels again in the backward
            raise RuntimeError("VideoMAETemporal backward: the input pixels were modified in place after the forward "
                               "(the patch-embedding weight gradient reads them again); pass a tensor that "
                               "stays unchanged until backward, or a copy")
        g_enc, g_temp, g_head = mod._run_backward(st, grad, *ctx.want)
        ctx.st = None
        sink = mod.grad_sink
        if sink is not None and hasattr(sink, "end_backward"):
            sink.end_backward()
        if sink is not None and not getattr(sink, "return_grads", False):
            return None, None, None, None, None      # the sink owns .grad (all-reduced in place)
        return None, g_enc, g_temp, g_head, None
