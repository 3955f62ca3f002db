"""The behaviour inputs of the RRR baseline, from the video and its dense optical-flow field.

The reference makes them in two places, both on the host and frame by frame:

  * `get_optic_flow` (src/utils/ibl_data_utils.py:1103-1243) turns one trial's video and Farneback flow into the
    per-frame scalars: motion energy, the percentile-clipped mean flow, the medians of |flow|.  `flow_features` is
    that function without the cv2 calls, the drawing and the plots, for all trials at once.
  * `get_rrr_data` (src/utils/utils.py:226-304) turns loader batches into the (K, F, C) array that
    create_eid_data.py saves.  `get_rrr_data` here is the same for batches given as dicts of tensors, and
    `behaviour_rrr_data` wraps two splits into the dict `vspike.rrr.train_rrr_baseline` takes.

The reductions over the field (medians, percentiles, clipped means, motion energy) are HIP kernels
(csrc/flow_features.hip); what is left acts on K x F values and is plain torch.  The flow itself is an input:
Farneback's algorithm is not built here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import VsError
from .rrr import INPUT_MODS

# create_eid_data.py:41-60: the command-line name -> the loader key get_rrr_data is called with
LOADER_KEY = {"me": "whisker-motion-energy", "of": "whisker-of", "of-2d": "whisker-of-video",
              "of-2d-v": "whisker-of-video", "ws": "wheel-speed"}


def _f32_sub(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a - b rounded once to float32: formed in float64 (exact or not, 53 >= 2 * 24 + 2 bits make the second
    rounding harmless), so the result is numpy's whatever the device's float32 arithmetic does."""
    return (a.double() - b.double()).float()


def _f32_div(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return (a.double() / b.double()).float()


def _minmax_append(x: torch.Tensor) -> torch.Tensor:
    """(x - min) / (max - min) over the frames of each trial, then the last value once more
    (ibl_data_utils.py:1113, 1139-1147), with numpy's float32 roundings.  x (K, F - 1, ...) -> (K, F, ...).
    A trial whose series is constant has max - min = 0 and becomes 0 / 0 = NaN throughout, as in the reference;
    a NaN in the series makes the whole trial NaN (np.min / np.max propagate it)."""
    lo, hi = x.amin(dim=1, keepdim=True), x.amax(dim=1, keepdim=True)
    y = _f32_div(_f32_sub(x, lo), _f32_sub(hi, lo))
    return torch.cat([y, y[:, -1:]], dim=1)


def flow_features(video: torch.Tensor, flow: torch.Tensor) -> dict:
    """get_optic_flow for K trials at once.  video (K, F, H, W) uint8 or float32 and flow (K, F - 1, H, W, 2)
    float32, dense, on the device; the video stays in its dtype and neither is converted or copied.  Returns
      'me'        (K, F) float32: mean_{h,w} |video[f + 1] - video[f]|,
      'of'        (K, F) float32: the reference's clip_vec_field, the mean over (h, w, 2) of |flow| clipped per
                  component to np.percentile(|flow[..., c]|, 10 / 90) of the whole trial,
      'of-2d'     (K, F, 2) float32: np.median over (h, w) of |flow[..., c]|,
      'of-video'  flow itself,
    each series min-max normalised over its trial with its last value appended once.  The medians and percentiles
    are numpy's bit for bit; 'me' and 'of' are float64 sums rounded once (the reference sums in float32).
    A trial whose series is constant gives the reference's 0 / 0 = NaN for that series (see _minmax_append)."""
    if not torch.is_tensor(video) or not torch.is_tensor(flow):
        raise VsError("flow_features: video and flow are tensors on the device")
    if video.dim() != 4 or video.dtype not in (torch.uint8, torch.float32):
        raise VsError("flow_features: video (K, F, H, W) uint8 or float32")
    if flow.dim() != 5 or flow.dtype != torch.float32 or flow.shape[4] != 2:
        raise VsError("flow_features: flow (K, F - 1, H, W, 2) float32")
    K, F, H, W = video.shape
    if F < 2 or tuple(flow.shape) != (K, F - 1, H, W, 2):
        raise VsError(f"flow_features: a video of {F} frames of {H} x {W} needs a flow field ({K}, {F - 1}, {H}, {W}, 2), "
                      f"got {tuple(flow.shape)}")
    if not video.is_contiguous() or not flow.is_contiguous() or video.device != flow.device:
        raise VsError("flow_features: video and flow must be dense and on one device (they are read in place)")
    ops.require_device(video, flow)
    me = ops.motion_energy(video)
    med = ops.flow_median2(flow, absolute=True)
    bounds = ops.flow_quantiles(flow, (10, 90))
    of = ops.flow_clip_mean(flow, bounds)
    return {"me": _minmax_append(me), "of": _minmax_append(of), "of-2d": _minmax_append(med), "of-video": flow}


def _np_dtype(t: torch.Tensor):
    return torch.empty(0, dtype=t.dtype).numpy().dtype


def _np_cat(parts, dim):
    """np.concatenate's result: the parts promoted by numpy's rules (float32 with int64 gives float64, where
    torch.cat would give float32)."""
    want = np.result_type(*[_np_dtype(p) for p in parts])
    dt = torch.from_numpy(np.empty(0, dtype=want)).dtype
    return torch.cat([p.to(dt) for p in parts], dim=dim)


def _frame_medians(flow: torch.Tensor, device) -> torch.Tensor:
    """np.median over (h, w) of each SIGNED component of flow (B, F - 1, H, W, 2): (B, F - 1, 2) float32."""
    if flow.dim() != 5 or flow.shape[4] != 2 or flow.dtype != torch.float32:
        raise VsError("get_rrr_data: 'whisker-of-video' is a (B, F - 1, H, W, 2) float32 flow field")
    return ops.flow_median2(flow.to(device).contiguous(), absolute=False)


def _per_trial(batch, key, T, device):
    """block / choice (B, 1) repeated over the T frames: (B, T, 1) (utils.py:252-254)."""
    return batch[key].to(device).repeat_interleave(T, dim=1).unsqueeze(2)


def get_rrr_data(batches, input_mod: str, device=None):
    """src/utils/utils.py:226-304 for `batches`, an iterable of dicts of tensors (a loader's batches).  Returns
    (X, y, timestamps) as tensors on `device` (default: the device the first batch's spikes are on if that is a
    GPU, else "cuda"), concatenated over the batches:
      'whisker-of-video'  X (K, F - 1, 2): the per-frame medians of the signed flow components (no abs),
      'all'               [whisker-motion-energy, wheel-speed, choice, block],
      'other'             [wheel-speed, choice, block],
      'of-all'            [median x, median y, wheel-speed, choice, block], the last flow frame's medians repeated
                          once so that the flow has as many frames as the wheel speed,
      anything else       batch[input_mod] as it is ('whisker-video' and 'wheel-speed' among them).
    choice and block are (B, 1) per trial and are repeated over the frames.  Parts of different dtypes are promoted
    as np.concatenate promotes them.  Raises VsError when a batch has no 'timestamp' (the reference asserts).
    Three values, as utils.py's function returns them (use_cebra.py, which unpacks two, is not reproduced)."""
    if not isinstance(input_mod, str):
        raise VsError("get_rrr_data: input_mod is a loader key (a string)")
    X, y, stamps = [], [], []
    for n, batch in enumerate(batches):
        if not isinstance(batch, dict):
            raise VsError(f"get_rrr_data: batch {n} is not a dict of tensors")
        if "timestamp" not in batch:
            raise VsError(f"get_rrr_data: timestamp is not in batch {n}")
        need = {"whisker-of-video": ("whisker-of-video",), "all": ("block", "choice", "wheel-speed",
                                                                    "whisker-motion-energy"),
                "other": ("block", "choice", "wheel-speed"),
                "of-all": ("block", "choice", "wheel-speed", "whisker-of-video")}.get(input_mod, (input_mod,))
        for key in need + ("ap",):
            if key not in batch or not torch.is_tensor(batch[key]):
                raise VsError(f"get_rrr_data: batch {n} has no tensor {key!r} ({input_mod!r} needs {need + ('ap',)})")
        if device is None:
            device = batch["ap"].device if batch["ap"].is_cuda else "cuda"
        if input_mod == "whisker-of-video":
            X.append(_frame_medians(batch[input_mod], device))
        elif input_mod in ("all", "other", "of-all"):
            ws = batch["wheel-speed"]
            if ws.dim() != 2:
                raise VsError("get_rrr_data: 'wheel-speed' is (B, T)")
            B, T = ws.shape
            for key in ("choice", "block"):
                if tuple(batch[key].shape) != (B, 1):
                    raise VsError(f"get_rrr_data: {key!r} is one value per trial, (B, 1)")
            if input_mod == "all" and batch["whisker-motion-energy"].shape != ws.shape:
                raise VsError("get_rrr_data: 'whisker-motion-energy' and 'wheel-speed' are both (B, T)")
            if input_mod == "of-all":
                of = batch["whisker-of-video"]
                if of.dim() != 5 or of.shape[0] != B or of.shape[1] + 1 != T:
                    raise VsError(f"get_rrr_data: 'of-all' needs a flow field of T - 1 = {T - 1} frames per trial")
            ws = ws.to(device)
            tail = [ws.unsqueeze(2), _per_trial(batch, "choice", T, device), _per_trial(batch, "block", T, device)]
            if input_mod == "all":
                head = [batch["whisker-motion-energy"].to(device).unsqueeze(2)]
            elif input_mod == "of-all":
                of = _frame_medians(batch["whisker-of-video"], device)
                head = [torch.cat([of, of[:, -1:]], dim=1)]                      # utils.py:284-286
            else:
                head = []
            X.append(_np_cat(head + tail, 2))
        else:
            X.append(batch[input_mod].to(device))
        y.append(batch["ap"].to(device))
        stamps.append(batch["timestamp"].to(device))
    if not X:
        raise VsError("get_rrr_data: no batches")
    return torch.cat(X, dim=0), torch.cat(y, dim=0), torch.cat(stamps, dim=0)


def behaviour_rrr_data(train_batches, test_batches, input_mod: str, eid: str = "session", device=None) -> dict:
    """The dict `train_rrr_baseline(data, input_mod)` takes, from the batches of the training and the test split:
    create_eid_data.py's mapping from the command-line name to the loader key ('me' -> 'whisker-motion-energy',
    'of' -> 'whisker-of', 'of-2d' and 'of-2d-v' -> 'whisker-of-video', 'ws' -> 'wheel-speed', the others unchanged),
    then get_rrr_data per split.  {eid: {'X': [train, test], 'y': [train, test], 'timestamp': [train, test],
    'setup': {}}}."""
    if input_mod not in INPUT_MODS:
        raise VsError(f"behaviour_rrr_data: input_mod {input_mod!r} is none of {INPUT_MODS}")
    key = LOADER_KEY.get(input_mod, input_mod)
    out = {"X": [], "y": [], "timestamp": [], "setup": {}}
    for batches in (train_batches, test_batches):
        X, y, stamps = get_rrr_data(batches, key, device=device)
        out["X"].append(X)
        out["y"].append(y)
        out["timestamp"].append(stamps)
    return {eid: out}
