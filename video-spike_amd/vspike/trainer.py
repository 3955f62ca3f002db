"""The training step of `src/trainer/base.py:144-159`, re-stated for the HIP path.

    outputs = model(inputs); loss = criterion(outputs, ap); loss.backward()
    [all-reduce of gradients]; optimizer.step(); lr_scheduler.step(); optimizer.zero_grad()

Differences by design: the loss stays on the device (the reference's per-step `loss.item()`,
base.py:154, is a host sync — `train_epoch` here collects device scalars and syncs once per
epoch), and the data-parallel exchange is vspike.dp.GradExchange instead of DDP hooks.
"""
from __future__ import annotations

from typing import Iterable, List, Optional

import torch

from .dp import GradExchange
from .loss import make_criterion
from .metrics import eval_session
from .optim import FusedAdamW


def input_modalities(config) -> List[str]:
    """`src/trainer/base.py:8-14`."""
    mods = config["data"]["modalities"]
    return [m for m in mods if mods[m]["input"]]


def model_inputs(config, batch):
    """`src/trainer/base.py:61-70`: Linear -> cat of flattened input modalities, else video."""
    if config["model"]["model_class"] == "Linear":
        return torch.cat([batch[m].flatten(1) for m in input_modalities(config)], dim=-1)
    return batch["video"]


def build_optimizer(model, config, total_steps: int, world: int = 1):
    """`src/train.py:44-57`: AdamW(lr, wd, eps) + OneCycleLR(max_lr=lr, pct_start, div_factor)."""
    o = config["optimizer"]
    opt = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=float(o["lr"]),
                     weight_decay=float(o["wd"]), eps=float(o["eps"]), grad_scale=1.0 / world)
    sched = torch.optim.lr_scheduler.OneCycleLR(optimizer=opt, total_steps=max(1, total_steps), max_lr=float(o["lr"]),
                                                pct_start=float(o["warmup_pct"]),
                                                div_factor=float(o["div_factor"]))
    return opt, sched


class ContrastTrainer:
    """The contrastive pretraining step of `src/trainer/contrast.py:80-122` for the ContrastViT plugin:

        ref, pos, neg = model(ref), model(pos), model(neg); loss = criterion(ref, pos, neg)['loss']
        loss.backward(); optimizer.step()                      # no scheduler in the reference

    `step` runs it fused: the three (n, C, H, W) batches go through ONE 3n forward, one vs_info_nce and
    one backward.  No op couples images before the loss, so the result is the three-call form's
    (`step_three_calls`, kept for comparison and for callers that drive the model themselves)."""

    def __init__(self, model, optimizer, lr_scheduler=None, criterion=None, exchange: Optional[GradExchange] = None):
        from .loss import InfoNCE
        self.model, self.optimizer, self.lr_scheduler, self.exchange = model, optimizer, lr_scheduler, exchange
        self.criterion = criterion if criterion is not None else InfoNCE(fix_temp=getattr(model, "fix_temp", True))

    def _finish(self, res):
        if self.exchange is not None:
            self.exchange.finish()
        self.optimizer.step()
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()
        self.optimizer.zero_grad(set_to_none=True)
        return {k: v.detach() for k, v in res.items()}

    def step(self, ref, pos, neg) -> dict:
        n = ref.shape[0]
        if pos.shape != ref.shape or neg.shape[1:] != ref.shape[1:]:
            raise ValueError("ContrastTrainer.step: ref / pos (n, C, H, W) and neg (m, C, H, W)")
        out = self.model(torch.cat([ref, pos, neg], dim=0))
        z, temp = out["z"], out["temp"]
        res = self.criterion({"z": z[:n], "temp": temp}, {"z": z[n:2 * n], "temp": temp}, {"z": z[2 * n:], "temp": temp})
        res["loss"].backward()
        return self._finish(res)

    def step_fused(self, frames, n: int) -> dict:
        """`step` on the views already side by side: frames (2n + m, C, H, W) = [ref | pos | neg], as
        vspike.data.ContrastFrames.fused(batch) hands them over (one buffer, filled by one launch), so the
        `torch.cat` of `step` and its copy of every frame are skipped.  Same forward, loss and update as
        step(frames[:n], frames[n:2n], frames[2n:])."""
        if frames.dim() != 4 or not 0 < 2 * n < frames.shape[0]:
            raise ValueError("ContrastTrainer.step_fused: frames (2n + m, C, H, W) with m >= 1")
        out = self.model(frames)
        z, temp = out["z"], out["temp"]
        res = self.criterion({"z": z[:n], "temp": temp}, {"z": z[n:2 * n], "temp": temp}, {"z": z[2 * n:], "temp": temp})
        res["loss"].backward()
        return self._finish(res)

    def step_three_calls(self, ref, pos, neg) -> dict:
        """The reference trainer's literal form: three forwards alive before one backward.  Refused while a
        data-parallel gradient sink is attached (the sink reduces one backward per step)."""
        res = self.criterion(self.model(ref), self.model(pos), self.model(neg))
        res["loss"].backward()
        return self._finish(res)

    def step_recon(self, ref) -> dict:
        """The reference's step for the `MAE` model (contrast.py:100-107 with `loss_fn_`'s first branch): one forward
        of `ref`, loss = recon_loss, backward, update.  Returns {'loss'} detached."""
        res = {"loss": self.model(ref)["recon_loss"]}
        res["loss"].backward()
        return self._finish(res)

    @torch.no_grad()
    def transform(self, batches: Iterable) -> torch.Tensor:
        """`src/trainer/contrast.py:165-206`: the stacked embeddings z of every batch (tensors, or dicts
        with the images under 'ref'), in order, with `model.config.mask_ratio` set to 0 for the pass
        (contrast.py:177-202).  The mask ratio and the model's train / eval mode are restored afterwards."""
        was_training = self.model.training
        conf = getattr(self.model, "config", None)
        ratio = getattr(conf, "mask_ratio", None)
        self.model.eval()
        if ratio is not None:
            conf.mask_ratio = 0
        try:
            zs = [self.model(b["ref"] if isinstance(b, dict) else b)["z"] for b in batches]
        finally:
            self.model.train(was_training)
            if ratio is not None:
                conf.mask_ratio = ratio
        return torch.cat(zs, dim=0)

    @torch.no_grad()
    def validate(self, train_batches: Iterable, val_batches: Iterable, idx=None, eid: str = "session") -> dict:
        """`src/trainer/contrast.py:129-162`: embed every frame of the train and validation trials in eval mode,
        fit the reduced-rank regression from the embeddings to the binned spikes and score the held-out trials
        (vspike.rrr.train_rrr); returns {'val_bps': nanmean of the per-neuron bits per spike}, the number the
        reference keeps its best checkpoint by.  Batches are dicts with the frames under 'ref' ((F, C, H, W),
        or 5-D with a leading 1, contrast.py:188-189) and the spikes (trials, T, N) under 'neural'.
        idx: the T frames regressed on; default the reference's draw from numpy's global generator,
        sort(choice(F - 1, T, replace=False)) (at F = 120, T = 100 its `choice(119, 100)`, last frame never used).
        The embeddings stay on the device between the transform and the fit."""
        import numpy as np
        from .rrr import train_rrr, train_rrr_wide
        X, y = [], []
        for batches in (train_batches, val_batches):
            batches = list(batches)
            frames = [b["ref"].squeeze(0) if b["ref"].dim() == 5 else b["ref"] for b in batches]
            z = self.transform(frames)
            neural = torch.cat([b["neural"] for b in batches], dim=0).to(z.device)
            X.append(z.view(neural.shape[0], -1, z.shape[-1]))
            y.append(neural)
        F, T = X[0].shape[1], y[0].shape[1]
        if idx is None:
            idx = np.sort(np.random.choice(F - 1, T, replace=False))
        sel = torch.as_tensor(np.asarray(idx), dtype=torch.long, device=X[0].device)
        if sel.numel() != T:
            raise ValueError(f"ContrastTrainer.validate: {sel.numel()} frame indices for {T} time bins")
        data = {eid: {"X": [x[:, sel, :] for x in X], "y": y, "setup": {}}}
        # an embedding wider than train_rrr's 32 features (MAE's hidden_size-wide z) goes through one RRRGD session
        res = (train_rrr_wide if X[0].shape[-1] > 32 else train_rrr)(data)
        return {"val_bps": float(np.nanmean(res[eid]["bps"]))}


    def fit(self, loader, train_loader, val_loader, max_steps: int = 1000, path: Optional[str] = None,
            eid: str = "session") -> dict:
        """`src/trainer/contrast.py:35-59`: passes over the pretrain `loader` until `max_steps` steps are taken,
        `validate(train_loader, val_loader)` after every pass, the one `max_steps` cuts short included; the best
        val_bps is kept and, with `path`, the model's `reference_state_dict()` is saved there on every improvement
        (the reference's best_model.pth; a NaN val_bps never improves, as there).  A loader with `fused` (vspike.data.
        ContrastFrames) feeds step_fused, any other iterable of {'ref', 'pos', 'neg'} feeds step.
        Returns {'steps': the per-step loss dicts (device tensors: nothing is read back per step), 'val_bps': one per
        pass, 'best_val_bps', 'best_pass'}.  No wandb, no progress bar."""
        steps, vals, best, best_pass = [], [], -float("inf"), None
        from .mae import MAE
        fused = getattr(loader, "fused", None)
        recon = isinstance(self.model, MAE)
        self.model.train()
        while len(steps) < max_steps:
            before = len(steps)
            for batch in loader:
                if recon:       # the loader still drew pos and neg: numpy's generator stands where the reference's does
                    steps.append(self.step_recon(batch["ref"]))
                elif fused is not None:
                    steps.append(self.step_fused(fused(batch), batch["ref"].shape[0]))
                else:
                    steps.append(self.step(batch["ref"], batch["pos"], batch["neg"]))
                if len(steps) >= max_steps:
                    break
            if len(steps) == before:
                raise ValueError("ContrastTrainer.fit: the pretrain loader gave no batch")
            val = self.validate(train_loader, val_loader, eid=eid)["val_bps"]
            vals.append(val)
            if val > best:
                best, best_pass = val, len(vals) - 1
                if path is not None:
                    torch.save(self.model.reference_state_dict(), path)
        return {"steps": steps, "val_bps": vals, "best_val_bps": best, "best_pass": best_pass}

    @torch.no_grad()
    def load_best(self, path: str) -> bool:
        """The reference's `transform(use_best=True)` (contrast.py:170-173, 70-78): load the weights `fit` saved at
        `path`; False, and the model as it is, when there is no such file."""
        import os
        if not os.path.exists(path):
            return False
        self.model.load_reference_state_dict(torch.load(path, map_location="cpu"))
        return True


class Trainer:
    def __init__(self, model, optimizer, lr_scheduler=None, config=None, criterion=None,
                 exchange: Optional[GradExchange] = None):
        """criterion: default = the config's `training.loss` (make_criterion: "poisson", the
        reference's PoissonNLL of src/train.py:59, or "mse")."""
        self.model, self.optimizer, self.lr_scheduler = model, optimizer, lr_scheduler
        self.config, self.exchange = config, exchange
        self.criterion = criterion if criterion is not None else make_criterion(config)

    def step(self, inputs, target) -> torch.Tensor:
        outputs = self.model(inputs)
        loss = self.criterion(outputs, target)
        loss.backward()
        if self.exchange is not None:
            self.exchange.finish()
        self.optimizer.step()
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()
        self.optimizer.zero_grad(set_to_none=True)
        return loss.detach()

    def train_epoch(self, batches: Iterable) -> float:
        self.model.train()
        losses = [self.step(model_inputs(self.config, b) if self.config else b["video"], b["ap"]) for b in batches]
        return float(torch.stack(losses).mean().item()) if losses else float("nan")

    @torch.no_grad()
    def eval_epoch(self, batches: Iterable, metrics=("bps", "rsquared")) -> dict:
        """`src/trainer/base.py:161-206`: per batch the loss; per session (`batch['eid'][0]`) the
        concatenated gt / log-rate outputs go through `metrics_list` (exp fused, on the device).
        Returns the reference's `eval_res` dict: eval_loss and eval_<metric>, each rounded to 5
        places as base.py:198,203 does."""
        import numpy as np
        self.model.eval()
        losses, sessions = [], {}
        for b in batches:
            out = self.model(model_inputs(self.config, b) if self.config else b["video"])
            losses.append(self.criterion(out, b["ap"]))
            eid = b["eid"][0] if "eid" in b else "session"
            s = sessions.setdefault(eid, {"gt": [], "preds": []})
            s["gt"].append(b["ap"])
            s["preds"].append(out)
        res = {k: [] for k in metrics}
        for s in sessions.values():
            r = eval_session(torch.cat(s["gt"], 0), torch.cat(s["preds"], 0), metrics)
            for k, v in r.items():
                res[k].append(v)
        out = {"eval_loss": round(float(np.mean([float(x) for x in losses])), 5) if losses else float("nan")}
        out.update({f"eval_{k}": round(float(np.mean(v)), 5) for k, v in res.items()})
        return out
