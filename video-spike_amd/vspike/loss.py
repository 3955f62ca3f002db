"""Spike-count regression losses, each fused with its gradient.

* Poisson (the reference's only training loss): `torch.nn.PoissonNLLLoss(reduction="none",
  log_input=True)` (src/train.py:59) followed by `.mean()` (src/trainer/base.py:142).  One pass
  computes exp(x) - y*x, a deterministic two-stage mean, and stashes d/dx = (exp(x) - y)/n for the
  backward (no second pass over x in the common upstream-gradient-is-1 case).
* MSE (BASELINE north_star: "Poisson/MSE spike-count regression head"): `torch.nn.MSELoss()`
  semantics, mean((x - y)^2), d/dx = 2 (x - y)/n.  The reference has no MSE training loss; it
  computes mse only as an eval metric (src/utils/utils.py:169-171).  Selected by the train config
  key `training.loss: mse` (default `poisson`), see `make_criterion`.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib as L
from . import ops


class _FusedMeanLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, kind):
        x = pred.detach().to(torch.float32).contiguous()
        y = target.detach().to(torch.float32).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        (ops.poisson_nll if kind == "poisson" else ops.mse_loss)(x, y, loss, dx=dx, grad_scale=1.0)
        ctx.save_for_backward(dx)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        # scale by the upstream gradient on device (no host sync)
        return dx * g.to(dx.dtype), None, None


def _check(pred, target):
    L.require_device(pred, target)
    if pred.shape != target.shape:
        raise ValueError(f"shape mismatch {tuple(pred.shape)} vs {tuple(target.shape)}")


def poisson_nll_mean(log_rate: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """mean(exp(log_rate) - target * log_rate) on the GPU (HIP), differentiable in log_rate."""
    _check(log_rate, target)
    return _FusedMeanLoss.apply(log_rate, target, "poisson")


def mse_mean(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """mean((pred - target)^2) on the GPU (HIP), differentiable in pred (torch.nn.MSELoss())."""
    _check(pred, target)
    return _FusedMeanLoss.apply(pred, target, "mse")


class PoissonNLLMeanLoss(nn.Module):
    """criterion(outputs, ap) -> scalar; equals PoissonNLLLoss(log_input=True)(...).mean()."""

    def forward(self, log_rate, target):
        return poisson_nll_mean(log_rate, target)


class MSEMeanLoss(nn.Module):
    """criterion(outputs, ap) -> scalar; equals torch.nn.MSELoss()(outputs, ap)."""

    def forward(self, pred, target):
        return mse_mean(pred, target)


class _InfoNCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ref, pos, neg, log_inv_tau):
        r, p, q = (t.detach().to(torch.float32).contiguous() for t in (ref, pos, neg))
        dev = r.device
        out = torch.empty(3, dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad
        dr = torch.empty_like(r) if need[0] else None
        dp = torch.empty_like(p) if need[1] else None
        dq = torch.empty_like(q) if need[2] else None
        lt = log_inv_tau.detach().to(torch.float32).reshape(1).contiguous() if log_inv_tau is not None else None
        dt = torch.empty(1, dtype=torch.float32, device=dev) if lt is not None and need[3] else None
        ops.info_nce(r, p, q, out, log_inv_tau=lt, d_ref=dr, d_pos=dp, d_neg=dq, grad_scale=1.0, d_log_inv_tau=dt)
        ctx.grads = (dr, dp, dq, dt)
        ctx.tau_shape = log_inv_tau.shape if log_inv_tau is not None else None
        loss, pos_loss, neg_loss = out.unbind(0)
        ctx.mark_non_differentiable(pos_loss, neg_loss)      # reported parts (they carry the detached shift c)
        return loss, pos_loss, neg_loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _gp, _gn):
        dr, dp, dq, dt = ctx.grads
        ctx.grads = None
        g = g.to(torch.float32)                               # scaled on the device (no host sync)
        return (dr * g if dr is not None else None, dp * g if dp is not None else None,
                dq * g if dq is not None else None, (dt * g).reshape(ctx.tau_shape) if dt is not None else None)


class InfoNCE(nn.Module):
    """The reference's contrastive criterion (`loss_fn_` -> `info_nce`, src/utils/loss_utils.py:3-21, 409-431)
    on vs_info_nce: `criterion(ref, pos, neg) -> {'loss', 'pos_loss', 'neg_loss'}`, with ref / pos / neg the
    ContrastViT plugin's output dicts ({'z', 'temp'}) or bare [n, E] embeddings.  fix_temp (default, as
    src/pretrain.py uses it): tau = 1; otherwise tau = ref['temp'] and its gradient reaches `temperature`.
    pos_loss and neg_loss are reported values (not differentiable); each rank uses its own negatives."""

    def __init__(self, fix_temp: bool = True):
        super().__init__()
        self.fix_temp = bool(fix_temp)

    def forward(self, ref, pos, neg):
        temp = None
        if isinstance(ref, dict):
            temp = None if self.fix_temp else ref.get("temp")
            ref, pos, neg = ref["z"], pos["z"], neg["z"]
        L.require_device(ref, pos, neg)
        if ref.dim() != 2 or pos.shape != ref.shape or neg.dim() != 2 or neg.shape[1] != ref.shape[1]:
            raise ValueError("InfoNCE: ref / pos [n, E] and neg [m, E]")
        # 1/tau = exp(log_inv_tau); temp = 1/exp(temperature), so this is the plugin's `temperature`
        log_inv_tau = -torch.log(temp) if temp is not None else None
        loss, pos_loss, neg_loss = _InfoNCEFn.apply(ref, pos, neg, log_inv_tau)
        return {"loss": loss, "pos_loss": pos_loss, "neg_loss": neg_loss}


LOSSES = {"poisson": poisson_nll_mean, "mse": mse_mean}


def make_criterion(config=None):
    """The training criterion named by `config.training.loss` (default "poisson", the reference's
    src/train.py:59).  With "mse" the model's outputs are regressed on the counts directly."""
    name = "poisson"
    if config is not None:
        try:
            name = str((config["training"] or {}).get("loss", "poisson") or "poisson").lower()
        except (KeyError, TypeError, AttributeError):
            name = "poisson"
    if name not in LOSSES:
        raise ValueError(f"training.loss must be one of {sorted(LOSSES)}, got {name!r}")
    return LOSSES[name]
