"""The reduced-rank regression (RRR) validation of the contrastive pretraining path.

The reference's `ContrastTrainer._validate` (src/trainer/contrast.py:129-162) embeds the train and validation
trials, fits an RRR encoding model from the embeddings to the binned spikes (`train_rrr`, src/utils/utils.py:
376-456; the model is `RRRGD`, src/model/rrr.py:29-202) and scores the held-out trials per neuron.

    beta[n,c,t] = sum_j U[n,c,j] V[j,t] (c < C),  beta[n,C,t] = b[n,0,t]
    yhat[k,t,n] = sum_c X[k,t,c] beta[n,c,t],     loss = sum (yhat - y)^2 + l2 sum beta^2

The fit is one `torch.optim.LBFGS(...).step(closure)` with default arguments, exactly `train_model_main`
(rrr.py:192-202): torch's L-BFGS driver is host plumbing and reproduces the reference's step rule and stopping
tests; the closure, evaluated up to 20 times per fit, is the hot path and runs in `vs_rrr_loss_grad`
(csrc/rrr.hip): one pass over y and X gives the loss and dU, dV, db with no autograd graph.  Scoring (clip,
bits per spike, R^2 per trial) is `vs_rrr_score`.  Everything is float64 but y / gt, which stay in the dtype
they come in (float32 in the reference's use).

The RRR baseline `src/train_rrr.py` is the second half of this module: `RRRGD` (the reference's model with its
sessions sharing V; inputs up to 1024 features run `vs_rrr_wide_loss_grad` / `vs_rrr_wide_score`, csrc/rrr_wide.hip),
`prepare_rrr_inputs` (Gaussian smoothing, one-hot choice / block, standardisation, frame selection) and
`train_rrr_baseline`.  Raw pixels ('whisker-video': more than 1024 features, up to 32768) go in as `PixelFeatures`,
a view of the video in its own dtype with the training statistics; such sessions run `vs_rrr_pixel_loss_grad` /
`vs_rrr_pixel_score` (csrc/rrr_pixel.hip), which standardise at the operand load.
"""
from __future__ import annotations

from functools import partial

import numpy as np
import torch

from . import ops
from ._lib import VsError

MAX_FEATURES, MAX_COMPONENTS = 32, 8


def check_dims(C: int, r: int) -> None:
    if not 1 <= C <= MAX_FEATURES:
        raise VsError(f"RRR: {C} features, supported 1..{MAX_FEATURES} (the bias column not counted); "
                      "pixel inputs ('whisker-video') are out of scope")
    if not 1 <= r <= MAX_COMPONENTS:
        raise VsError(f"RRR: {r} components, supported 1..{MAX_COMPONENTS}")


def init_params(T: int, N: int, C: int, r: int):
    """U [N, C, r] and V [r, T] as RRRGD draws them (rrr.py:35,42-43): np.random.seed(0), U first."""
    check_dims(C, r)
    rs = np.random.RandomState(0)
    U = rs.normal(size=(N, C, r)) / np.sqrt(T * r)
    V = rs.normal(size=(r, T)) / np.sqrt(T * r)
    return U, V


class RRR:
    """One session's RRRGD: a single-session front of the `RRRGD` below, capped at 32 features.  `fit(X, y)` takes
    standardised device tensors: X [K, T, C+1] float64 with a last column of ones, y [K, T, N] float32 or float64."""
    _EID = "session"

    def __init__(self, n_comp: int = 3, l2: float = 100.):
        self.n_comp, self.l2 = int(n_comp), float(l2)
        self._m = RRRGD(self.n_comp, self.l2)
        self.losses, self.n_iter, self.func_evals = [], 0, 0

    @property
    def U(self):
        return self._m.U(self._EID)

    @property
    def b(self):
        return self._m.b(self._EID)

    @property
    def V(self):
        return self._m.V

    def _check(self, X, y):
        if X.dim() != 3 or y.dim() != 3 or X.shape[:2] != y.shape[:2]:
            raise VsError("RRR: X [K, T, C+1] and y [K, T, N]")
        check_dims(X.shape[2] - 1, self.n_comp)
        if X.dtype != torch.float64:
            raise VsError("RRR: X must be float64 (the reference's bias column makes it so)")

    def fit(self, X: torch.Tensor, y: torch.Tensor) -> "RRR":
        """RRRGD.fit on the one session: the same draw, parameter order [U, b, V] and closure."""
        self._check(X, y)
        self._m.fit({self._EID: (X, y)})
        self.N, self.C, self.T = y.shape[2], X.shape[2] - 1, X.shape[1]
        self.losses, self.n_iter, self.func_evals = self._m.losses, self._m.n_iter, self._m.func_evals
        return self

    def mse(self, X: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """sum (yhat - y)^2 over everything: the reference's `mse_val_mean` (rrr.py:180-181), a device scalar."""
        self._check(X, y)
        return self._m.mse({self._EID: (X, y)})

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        """yhat [K, T, N] (rrr.py:105-116).  Not on the validation path, which never materialises yhat
        (`score` fuses it); kept as a plain einsum for callers that want the array."""
        beta = torch.cat((self.U @ self.V, self.b), 1)
        return torch.einsum("ktc,nct->ktn", X, beta)

    def score(self, X: torch.Tensor, mean_y: torch.Tensor, std_y: torch.Tensor, gt: torch.Tensor,
              want_pred: bool = True) -> dict:
        """utils.py:411-447 on the held-out trials: device tensors pred [K, T, N] (clipped rates), bps [N],
        r2 [N], co_bps and r2_mean (scalars)."""
        self._check(X, gt)
        return self._m.score(self._EID, X, mean_y, std_y, gt, want_pred=want_pred)

    def state_dict(self, eid: str = "session") -> dict:
        """The layout of RRRGD.state_dict (rrr.py:64-71)."""
        return {"model": {f"{eid}_U": self.U.cpu().clone(), f"{eid}_b": self.b.cpu().clone(), "V": self.V.cpu().clone()},
                "l2": self.l2, "eids": [eid], "N": self.N, "T": self.T, "n_comp": self.n_comp}


def _sum_trials(a: torch.Tensor) -> torch.Tensor:
    """sum over the leading (trial) axis in ascending order, in a's dtype: numpy's order for a reduction over
    the outer axis of a C-ordered array, so the statistics below are numpy's bit for bit (float32 included)."""
    acc = a[0].clone()
    for k in range(1, a.shape[0]):
        acc += a[k]
    return acc


def _div(a: torch.Tensor, b) -> torch.Tensor:
    """a / b rounded once to a's dtype.  A float32 quotient is formed in float64 and rounded, which is the
    correctly rounded float32 quotient (53 >= 2 * 24 + 2 bits) whatever the device's float32 division does:
    with plain float32 division on the device the standardised y differed from numpy's in the last bit of some
    elements, and the fit ended 60 x the reference's own spread away instead of 1e-5 x."""
    if a.dtype == torch.float64:
        return a / b
    b = b.double() if torch.is_tensor(b) else float(b)
    return (a.double() / b).to(a.dtype)


def _mean_trials(a: torch.Tensor) -> torch.Tensor:
    return _div(_sum_trials(a), a.shape[0])


def _std(arr: torch.Tensor):
    """utils.py:107-112: mean and standard deviation over the trials, the latter clipped at 1e-8, in arr's dtype
    like np.mean / np.std.  The order of the sums and the rounding of every step matter more than it looks: the
    fit amplifies a last-bit change of its inputs by ~1e9, so a float32 y standardised
    with differently rounded statistics gives a visibly different model.  The root is taken in float64 and
    rounded, which is the correctly rounded float32 root."""
    mean = _mean_trials(arr)
    d = arr - mean
    var = _mean_trials(d * d)
    std = var.double().sqrt().to(arr.dtype).clamp_min(1e-8)
    return mean, std


def _device_tensor(a, device):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if not t.is_floating_point():
        t = t.to(torch.float32)
    return t.to(device)


def _device_video(a, device):
    """'whisker-video' frames on the device: (K, F, c, h, w) flattened to (K, F, c h w) as a view
    (train_rrr.py:99-102).  More than 1024 pixels per frame stay in their dtype; narrower ones go through
    `_device_tensor` as every other input does."""
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if t.dim() == 5:
        t = t.reshape(t.shape[0], t.shape[1], -1)
    if t.dim() == 3 and t.shape[2] > WIDE_MAX_FEATURES:
        return t.to(device).contiguous()
    return _device_tensor(t, device)


def train_rrr(data_dict: dict, device=None, n_comp: int = 3, l2: float = 100.) -> dict:
    """`train_rrr` of src/utils/utils.py:376-456: data_dict[eid] = {'X': [train, val] (K, T, C), 'y': [train,
    val] (K, T, N), 'setup': {}}, numpy or torch.  Per eid: standardise X and y with the train split's
    statistics, append the bias column, fit an RRR (n_comp 3, l2 100) and score the validation split.
    Returns {eid: {'gt', 'pred', 'bps': [per neuron], 'r2': [per neuron], 'eid'}} with numpy gt / pred.
    Unlike the reference the inputs are left as they were (it standardises data_dict in place); the
    statistics are stored under 'setup' as it does."""
    result = {}
    for eid, d in data_dict.items():
        X = [_device_tensor(x, device or (x.device if torch.is_tensor(x) and x.is_cuda else "cuda")) for x in d["X"]]
        dev = X[0].device
        y = [_device_tensor(v, dev) for v in d["y"]]
        check_dims(X[0].shape[2], n_comp)
        mean_X, std_X = _std(X[0])
        mean_y, std_y = _std(y[0])
        Xs, ys = [], []
        for i in range(2):
            x = _div(X[i] - mean_X, std_X).to(torch.float64)
            ones = torch.ones(x.shape[0], x.shape[1], 1, dtype=torch.float64, device=dev)
            Xs.append(torch.cat([x, ones], dim=2))                           # utils.py:389
            ys.append(_div(y[i] - mean_y, std_y))
        if isinstance(d.get("setup"), dict):
            d["setup"].update(mean_X_Tv=mean_X, std_X_Tv=std_X, mean_y_TN=mean_y, std_y_TN=std_y)
        model = RRR(n_comp=n_comp, l2=l2).fit(Xs[0], ys[0])
        s = model.score(Xs[1], mean_y, std_y, y[1])
        result[eid] = {"gt": y[1].cpu().numpy(), "pred": s["pred"].cpu().numpy(),
                       "bps": s["bps"].cpu().tolist(), "r2": s["r2"].cpu().tolist(), "eid": eid}
    return result


# ---- the RRR baseline (src/train_rrr.py): sessions sharing V, wide inputs, feature preparation ------------------
WIDE_MAX_FEATURES = 1024
EMBEDDING_MODS = ("cebra", "pca", "ws", "whisker-video", "vit", "cm", "m", "c")       # train_rrr.py:119
INPUT_MODS = ("me", "of", "of-2d", "of-2d-v", "all", "other", "me-all", "of-all") + EMBEDDING_MODS


def train_rrr_wide(data_dict: dict, device=None, n_comp: int = 3, l2: float = 100.) -> dict:
    """train_rrr for embeddings of 33 .. 1024 features (the MAE plugin's hidden_size-wide z): the same preparation
    (the train split's `_std`, the bias column), then one RRRGD session per eid in place of RRR, which takes at most
    32 features.  Same return value as train_rrr."""
    result = {}
    for eid, d in data_dict.items():
        X = [_device_tensor(x, device or (x.device if torch.is_tensor(x) and x.is_cuda else "cuda")) for x in d["X"]]
        dev = X[0].device
        y = [_device_tensor(v, dev) for v in d["y"]]
        mean_X, std_X = _std(X[0])
        mean_y, std_y = _std(y[0])
        Xs, ys = [], []
        for i in range(2):
            x = _div(X[i] - mean_X, std_X).to(torch.float64)
            ones = torch.ones(x.shape[0], x.shape[1], 1, dtype=torch.float64, device=dev)
            Xs.append(torch.cat([x, ones], dim=2))
            ys.append(_div(y[i] - mean_y, std_y))
        if isinstance(d.get("setup"), dict):
            d["setup"].update(mean_X_Tv=mean_X, std_X_Tv=std_X, mean_y_TN=mean_y, std_y_TN=std_y)
        model = RRRGD(n_comp=n_comp, l2=l2).fit({eid: (Xs[0], ys[0])})
        s = model.score(eid, Xs[1], mean_y, std_y, y[1])
        result[eid] = {"gt": y[1].cpu().numpy(), "pred": s["pred"].cpu().numpy(),
                       "bps": s["bps"].cpu().tolist(), "r2": s["r2"].cpu().tolist(), "eid": eid}
    return result


def check_dims_wide(C: int, r: int) -> None:
    if not 1 <= C <= WIDE_MAX_FEATURES:
        raise VsError(f"RRRGD: {C} features, supported 1..{WIDE_MAX_FEATURES} (the bias column not counted); "
                      "wider inputs (raw pixels, 'whisker-video') go in as vspike.rrr.PixelFeatures")
    if not 1 <= r <= MAX_COMPONENTS:
        raise VsError(f"RRRGD: {r} components, supported 1..{MAX_COMPONENTS}")


PIXEL_MAX_FEATURES, PIXEL_MAX_COMPONENTS = ops.RRR_PIXEL_MAX_FEATURES, ops.RRR_PIXEL_MAX_COMPONENTS


def check_dims_pixel(C: int, r: int) -> None:
    if not 1 <= C <= PIXEL_MAX_FEATURES:
        raise VsError(f"RRRGD: {C} pixels per frame, supported 1..{PIXEL_MAX_FEATURES}")
    if not 1 <= r <= PIXEL_MAX_COMPONENTS:
        raise VsError(f"RRRGD: {r} components, supported 1..{PIXEL_MAX_COMPONENTS} for pixel features (the gradient "
                      "kernel keeps U and dU of its tile in registers)")


class PixelFeatures:
    """A session's features as raw pixels: X_raw [K, F, C] uint8 or float32 (or [K, F, c, h, w], flattened as
    train_rrr.py:99-102 does) is kept as it is, a view and never a copy; time bin t reads frame idx[t]; mean / std
    [F, C] are the training trials' statistics (`ops.rrr_pixel_stats`: float64 for uint8, float32 for float32, as
    numpy gives them).  It stands where RRRGD takes a standardised float64 X [K, T, C+1]: the kernels form
    (x - mean) / std at the operand load and the bias column is implicit.  `shape` is that tensor's shape."""

    def __init__(self, X_raw: torch.Tensor, idx, mean: torch.Tensor, std: torch.Tensor):
        if not torch.is_tensor(X_raw) or X_raw.dim() not in (3, 5) or X_raw.dtype not in (torch.uint8, torch.float32):
            raise VsError("PixelFeatures: X_raw [K, F, C] (or [K, F, c, h, w]) uint8 / float32 tensor")
        if not X_raw.is_contiguous():
            raise VsError("PixelFeatures: X_raw must be dense (it is used in place, never copied)")
        X = X_raw.view(X_raw.shape[0], X_raw.shape[1], -1)
        K, F, C = X.shape
        ix = idx.detach().cpu().numpy() if torch.is_tensor(idx) else np.asarray(idx)
        if ix.ndim != 1 or ix.dtype.kind not in "iu" or len(ix) < 1:
            raise VsError("PixelFeatures: idx must hold the frame index of every time bin (integers)")
        if ix.min() < 0 or ix.max() >= F:
            raise VsError(f"PixelFeatures: idx must hold frame indices below {F}")
        stat = torch.float64 if X.dtype == torch.uint8 else torch.float32
        for t in (mean, std):
            if not torch.is_tensor(t) or tuple(t.shape) != (F, C) or t.dtype != stat:
                raise VsError(f"PixelFeatures: mean / std must be [F, C] = [{F}, {C}] tensors of {stat} "
                              f"(the statistics numpy gives for {X.dtype})")
        self.X, self.mean, self.std = X, mean.contiguous(), std.contiguous()
        self.idx = torch.from_numpy(ix.astype(np.int64)).to(X.device)
        self.shape = torch.Size((K, len(ix), C + 1))
        self.device = X.device

    def materialise(self) -> torch.Tensor:
        """The float64 X [K, T, C+1] this object stands for, in the kernels' arithmetic (tests and small inputs
        only: it is the buffer the pixel entries exist to avoid)."""
        x = self.X.index_select(1, self.idx)
        m, s = self.mean.index_select(0, self.idx), self.std.index_select(0, self.idx)
        z = (x.double() - m) / s if self.X.dtype == torch.uint8 else _div(x - m, s).double()
        return torch.cat([z, torch.ones(z.shape[0], z.shape[1], 1, dtype=torch.float64, device=z.device)], dim=2)


def _entries(X, N: int, r: int):
    """(loss_grad, score, workspace bytes of loss_grad) for a session's X, a dense tensor [K, T, C+1] or a
    PixelFeatures, and N neurons, r components: the ops.rrr*_loss_grad / ops.rrr*_score entry with its leading
    operands bound, to be called with what follows them (y or U, ...).  C <= 32 runs the narrow entries."""
    K, T, C1 = X.shape
    if isinstance(X, PixelFeatures):
        lead = (X.X, X.idx, X.mean, X.std)
        return (partial(ops.rrr_pixel_loss_grad, *lead), partial(ops.rrr_pixel_score, *lead),
                ops.rrr_pixel_loss_grad_workspace_bytes(K, T, N, C1 - 1, r))
    X = X.contiguous()
    if C1 - 1 > MAX_FEATURES:
        return (partial(ops.rrr_wide_loss_grad, X), partial(ops.rrr_wide_score, X),
                ops.rrr_wide_loss_grad_workspace_bytes(K, T, N, C1 - 1))
    return (partial(ops.rrr_loss_grad, X), partial(ops.rrr_score, X),
            ops.rrr_loss_grad_workspace_bytes(K, T, N, C1 - 1))


class RRRGD:
    """The reference's RRRGD with its sessions (src/model/rrr.py:29-202): every session has its own U [N, C, r] and
    b [N, 1, T]; one V [r, T] is shared by all.  `fit({eid: (X, y)})` takes standardised device tensors per
    session, X [K, T, C+1] float64 with a last column of ones and y [K, T, N] float32 or float64; T is common,
    K, N and C may differ.  Sessions with C <= 32 run vs_rrr_loss_grad, wider ones vs_rrr_wide_loss_grad.  A
    session's X may instead be a PixelFeatures (raw pixels, C <= 32768, n_comp <= 4): it runs
    vs_rrr_pixel_loss_grad / vs_rrr_pixel_score, and pixel, wide and narrow sessions mix in one fit."""

    def __init__(self, n_comp: int = 3, l2: float = 100.):
        self.n_comp, self.l2 = int(n_comp), float(l2)
        self.eids, self._U, self._b, self._V = [], {}, {}, None
        self.losses, self.n_iter, self.func_evals = [], 0, 0

    def _check(self, X, y, what="RRRGD"):
        if isinstance(X, PixelFeatures):
            if not torch.is_tensor(y) or y.dim() != 3 or X.shape[:2] != y.shape[:2] or y.device != X.device:
                raise VsError(f"{what}: PixelFeatures of [K, F, C] pixels with T frame indices and y [K, T, N] on "
                              "its device")
            check_dims_pixel(X.shape[2] - 1, self.n_comp)
            if y.dtype not in (torch.float32, torch.float64):
                raise VsError(f"{what}: y must be float32 or float64")
            return
        if not (torch.is_tensor(X) and torch.is_tensor(y)) or X.dim() != 3 or y.dim() != 3 \
                or X.shape[:2] != y.shape[:2]:
            raise VsError(f"{what}: X [K, T, C+1] and y [K, T, N] device tensors per session")
        check_dims_wide(X.shape[2] - 1, self.n_comp)
        if X.dtype != torch.float64:
            raise VsError(f"{what}: X must be float64 (the reference's bias column makes it so)")
        if y.dtype not in (torch.float32, torch.float64):
            raise VsError(f"{what}: y must be float32 or float64")

    def fit(self, data: dict) -> "RRRGD":
        """One default torch L-BFGS step over [U_0, b_0, U_1, b_1, ..., V] (the reference's ParameterDict order,
        rrr.py:46-49,199).  The initial values are rrr.py:35-49 exactly: one RandomState(0), per session in dict
        order a U and then a V draw, and the LAST session's V is the one kept.  The closure adds the sessions'
        losses and dVs in session order with plain float64 adds.
        Each b's master copy is a parameter of its y's dtype, because the reference's is (rrr.py:44-47: b = mean_k y,
        float32 when y is): autograd rounds its gradient to that dtype and L-BFGS updates it in that dtype.  Keeping
        b in float64 instead moves the fit a hundred times further from the reference's than the reference moves
        under a reordering of its trials, so the closure copies b into a float64 tensor
        before the kernel and db out of one afterwards (N T elements)."""
        if not isinstance(data, dict) or not data:
            raise VsError("RRRGD.fit: {eid: (X, y)} with at least one session")
        sess = {}
        for eid, (X, y) in data.items():
            self._check(X, y)
            sess[eid] = (X, y.contiguous())
        Ts = {X.shape[1] for X, _ in sess.values()}
        if len(Ts) != 1:
            raise VsError(f"RRRGD.fit: the sessions share V, so T must be equal across them (got {sorted(Ts)})")
        T, r = Ts.pop(), self.n_comp
        self.T, self.eids = T, list(sess)
        dev = next(iter(sess.values()))[0].device
        rs = np.random.RandomState(0)
        U, b_master, b64, dU, db64, dVs, ws, fn = {}, {}, {}, {}, {}, {}, {}, {}
        V0 = None
        for eid, (X, y) in sess.items():
            N, C = y.shape[2], X.shape[2] - 1
            U0 = rs.normal(size=(N, C, r)) / np.sqrt(T * r)                      # rrr.py:42
            V0 = rs.normal(size=(r, T)) / np.sqrt(T * r)                         # rrr.py:43: the last one is kept
            U[eid] = torch.from_numpy(U0).to(dev).requires_grad_(True)
            b_master[eid] = _mean_trials(y).t().unsqueeze(1).contiguous().requires_grad_(True)    # rrr.py:44
            b64[eid] = b_master[eid].detach().double()
            dU[eid], db64[eid] = torch.zeros_like(U[eid]), torch.zeros_like(b64[eid])
            dVs[eid] = torch.zeros(r, T, dtype=torch.float64, device=dev)
            U[eid].grad, b_master[eid].grad = dU[eid], torch.zeros_like(b_master[eid])
            fn[eid], _, need = _entries(X, N, r)
            ws[eid] = torch.empty(need // 8 + 2, dtype=torch.float64, device=dev)
        V = torch.from_numpy(V0).to(dev).requires_grad_(True)
        V.grad = torch.zeros_like(V)
        losses = []

        def closure():
            with torch.no_grad():
                total = None
                for i, (eid, (_, y)) in enumerate(sess.items()):
                    b64[eid].copy_(b_master[eid])
                    loss = torch.empty(1, dtype=torch.float64, device=dev)
                    fn[eid](y, U[eid], V, b64[eid], self.l2, loss, dU=dU[eid], dV=dVs[eid], db=db64[eid],
                            workspace=ws[eid])
                    b_master[eid].grad.copy_(db64[eid])
                    if i == 0:
                        total = loss
                        V.grad.copy_(dVs[eid])
                    else:
                        total = total + loss
                        V.grad.add_(dVs[eid])
            losses.append(total)
            return total[0]

        params = [p for eid in sess for p in (U[eid], b_master[eid])] + [V]
        opt = torch.optim.LBFGS(params)                                          # rrr.py:199
        opt.step(closure)                                                        # rrr.py:177
        st = opt.state[params[0]]
        self.n_iter, self.func_evals = int(st["n_iter"]), int(st["func_evals"])
        self.losses = torch.cat(losses).cpu().numpy()
        with torch.no_grad():
            for eid in sess:
                b64[eid].copy_(b_master[eid])
        self._U = {eid: U[eid].detach() for eid in sess}
        self._b = b64
        self._V = V.detach()
        self._N = {eid: y.shape[2] for eid, (_, y) in sess.items()}
        return self

    def _known(self, eid):
        if eid not in self._U:
            raise VsError(f"RRRGD: no fitted session {eid!r} (sessions: {self.eids})")

    def U(self, eid) -> torch.Tensor:
        self._known(eid)
        return self._U[eid]

    def b(self, eid) -> torch.Tensor:
        self._known(eid)
        return self._b[eid]

    @property
    def V(self) -> torch.Tensor:
        return self._V

    def _check_session(self, eid, X, y, what):
        self._known(eid)
        self._check(X, y, what)
        U = self._U[eid]
        if X.shape[1] != self.T or X.shape[2] - 1 != U.shape[1] or y.shape[2] != U.shape[0]:
            raise VsError(f"{what}: session {eid!r} was fitted with T {self.T}, C {U.shape[1]}, N {U.shape[0]}")

    def mse(self, data: dict) -> torch.Tensor:
        """sum (yhat - y)^2 over everything and every session given: the reference's `mse_val_mean`
        (rrr.py:180-181), a device scalar; the sessions are added in dict order."""
        total = None
        for eid, (X, y) in data.items():
            self._check_session(eid, X, y, "RRRGD.mse")
            loss = torch.empty(1, dtype=torch.float64, device=X.device)
            _entries(X, y.shape[2], self.n_comp)[0](y.contiguous(), self._U[eid], self._V, self._b[eid], 0.0, loss)
            total = loss if total is None else total + loss
        if total is None:
            raise VsError("RRRGD.mse: {eid: (X, y)} with at least one session")
        return total[0]

    def score(self, eid, X: torch.Tensor, mean_y: torch.Tensor, std_y: torch.Tensor, gt: torch.Tensor,
              want_pred: bool = True) -> dict:
        """train_rrr.py:193-224 on a session's held-out trials: device tensors pred [K, T, N] (clipped rates),
        bps [N], r2 [N], co_bps and r2_mean (scalars)."""
        self._check_session(eid, X, gt, "RRRGD.score")
        dev = X.device
        K, T, N = gt.shape
        pred = torch.empty(K, T, N, dtype=torch.float64, device=dev) if want_pred else None
        bps, r2 = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(2))
        out = torch.empty(2, dtype=torch.float64, device=dev)
        _entries(X, N, self.n_comp)[1](self._U[eid], self._V, self._b[eid], mean_y.to(torch.float64).contiguous(),
                                       std_y.to(torch.float64).contiguous(), gt.contiguous(), bps, r2, out, pred=pred)
        return {"pred": pred, "bps": bps, "r2": r2, "co_bps": out[0], "r2_mean": out[1]}

    def state_dict(self) -> dict:
        """The layout of RRRGD.state_dict (rrr.py:64-71)."""
        model = {}
        for eid in self.eids:
            model[f"{eid}_U"] = self._U[eid].cpu().clone()
            model[f"{eid}_b"] = self._b[eid].cpu().clone()
        model["V"] = self._V.cpu().clone()
        return {"model": model, "l2": self.l2, "eids": list(self.eids), "N": sum(self._N.values()), "T": self.T,
                "n_comp": self.n_comp}


def _one_hot(col: torch.Tensor, frames: int):
    """utils.py:114-119 for a (K, 1) column: (K, frames, number of distinct values) float64, the categories being
    the sorted distinct values of this very column.  Returns (one-hot, categories)."""
    uni = torch.unique(col)                                                      # sorted
    ret = (col.reshape(-1, 1, 1) == uni.reshape(1, 1, -1)).to(torch.float64)
    return ret.expand(-1, frames, -1), uni


def prepare_rrr_inputs(data: dict, input_mod: str, idx=None, smooth_w=2, device=None):
    """train_rrr.py:108-171 on the device: data[eid] = {'X': [train, val] (K, F, C), 'y': [train, val] (K, T, N)
    counts, 'setup': {}}, numpy or torch, left as they are.  Per session (in sorted order): the raw validation
    counts are kept as the ground truth; both y splits are smoothed along time (gaussian_filter1d, sigma
    `smooth_w`); for the behaviour modes choice and block (the last two columns, constant within a trial) become
    one-hot columns in front of the continuous ones; X and y are standardised with the train split's statistics;
    the bias column is appended and the T frames `idx` of F are selected (default: the reference's draw
    sort(choice(F - 1, T, replace=False)) from numpy's global generator, once for all sessions).
    Returns (prepared, ground_truth): prepared[eid] = {'X': [..], 'y': [..], 'setup': {mean_X_Tv, std_X_Tv,
    mean_y_TN, std_y_TN}} as device tensors, ground_truth[eid] the raw validation counts.
    'whisker-video': X may be (K, F, c, h, w) and is flattened to (K, F, c h w) as a view (train_rrr.py:99-102).  A
    session with more than 1024 pixels per frame comes back as PixelFeatures for both splits: X stays on the
    device in its own dtype, uint8 or float32 (uint8 is NOT converted to float32 here, unlike narrower integer
    inputs, which `_device_tensor` converts as before; numpy's statistics of a uint8 array are float64, and so are
    these), the statistics come from vs_rrr_pixel_stats, and nothing of the video's size is written."""
    if input_mod not in INPUT_MODS:
        raise VsError(f"prepare_rrr_inputs: input_mod {input_mod!r} is none of {INPUT_MODS}")
    if not isinstance(data, dict) or not data:
        raise VsError("prepare_rrr_inputs: {eid: {'X': [train, val], 'y': [train, val]}} with at least one session")
    eids = sorted(data)                                                          # train_rrr.py:112
    loaded = {}
    for eid in eids:
        d = data[eid]
        X = [_device_video(x, device or (x.device if torch.is_tensor(x) and x.is_cuda else "cuda"))
             if input_mod == "whisker-video" else
             _device_tensor(x, device or (x.device if torch.is_tensor(x) and x.is_cuda else "cuda")) for x in d["X"]]
        y = [_device_tensor(v, X[0].device) for v in d["y"]]
        if any(x.dim() != 3 for x in X) or any(v.dim() != 3 for v in y) or X[0].shape[1:] != X[1].shape[1:] \
                or y[0].shape[1:] != y[1].shape[1:] or any(x.shape[0] != v.shape[0] for x, v in zip(X, y)):
            raise VsError(f"prepare_rrr_inputs: session {eid!r}: X [K, F, C] and y [K, T, N] per split")
        if input_mod == "whisker-video" and X[0].shape[2] > WIDE_MAX_FEATURES \
                and (X[0].dtype != X[1].dtype or X[0].dtype not in (torch.uint8, torch.float32)):
            raise VsError(f"prepare_rrr_inputs: session {eid!r}: more than {WIDE_MAX_FEATURES} pixels per frame need "
                          "uint8 or float32 frames, the same dtype in both splits")
        loaded[eid] = (X, y)
    Ts = {y[0].shape[1] for _, y in loaded.values()}
    if len(Ts) != 1:
        raise VsError(f"prepare_rrr_inputs: T must be equal across sessions (got {sorted(Ts)})")
    T = Ts.pop()
    if idx is None:
        F = loaded[eids[0]][0][0].shape[1]
        if F - 1 < T:
            raise VsError(f"prepare_rrr_inputs: cannot draw {T} of {F} - 1 frames")
        idx = np.sort(np.random.choice(F - 1, T, replace=False))                 # train_rrr.py:48-49
    idx = np.asarray(idx)
    if idx.ndim != 1 or idx.dtype.kind not in "iu" or len(idx) != T:
        raise VsError(f"prepare_rrr_inputs: idx must hold {T} frame indices (one per bin of y)")
    prepared, ground_truth = {}, {}
    for eid in eids:
        X, y = loaded[eid]
        dev = X[0].device
        F = X[0].shape[1]
        if idx.min() < 0 or idx.max() >= F:
            raise VsError(f"prepare_rrr_inputs: idx must hold {T} frame indices below {F} (session {eid!r})")
        ground_truth[eid] = y[1]                                                 # train_rrr.py:116
        if input_mod in EMBEDDING_MODS:
            if input_mod == "m":
                X = [x[..., :3] for x in X]                                      # train_rrr.py:126
        elif input_mod not in ("me", "of-2d"):                                   # train_rrr.py:129-141
            const = 3 if input_mod in ("me-all", "of-all") else 2
            cats, new = [], []
            for x in X:
                if x.shape[2] < const:
                    raise VsError(f"prepare_rrr_inputs: {input_mod!r} needs at least {const} columns of X")
                contin_dim = x.shape[2] - const
                choice, c_cat = _one_hot(x[:, 0, -2:-1], F)
                block, b_cat = _one_hot(x[:, 0, -1:], F)
                new.append(torch.cat([choice, block, x[..., x.shape[2] - 2 - contin_dim:-2].double()], dim=2))
                cats.append((c_cat, b_cat))
            if not all(torch.equal(p, q) for p, q in zip(*cats)):
                raise VsError(f"prepare_rrr_inputs: session {eid!r}: the two splits do not have the same choice / "
                              "block categories, so their one-hot columns differ (the reference fails with a "
                              "shape error at the standardisation)")
            X = new
        y = [ops.gauss_smooth_time(v.contiguous(), smooth_w) for v in y]         # train_rrr.py:118
        pixels = input_mod == "whisker-video" and X[0].shape[2] > WIDE_MAX_FEATURES
        mean_X, std_X = ops.rrr_pixel_stats(X[0]) if pixels else _std(X[0])      # train_rrr.py:144-145
        mean_y, std_y = _std(y[0])
        sel = torch.from_numpy(idx.astype(np.int64)).to(dev)
        Xs, ys = [], []
        for i in range(2):
            if pixels:
                Xs.append(PixelFeatures(X[i], idx, mean_X, std_X))
            else:
                x = _div(X[i] - mean_X, std_X).to(torch.float64)
                ones = torch.ones(x.shape[0], x.shape[1], 1, dtype=torch.float64, device=dev)
                Xs.append(torch.cat([x, ones], dim=2).index_select(1, sel).contiguous())   # train_rrr.py:156-163
            ys.append(_div(y[i] - mean_y, std_y))
        setup = dict(mean_X_Tv=mean_X, std_X_Tv=std_X, mean_y_TN=mean_y, std_y_TN=std_y)
        if isinstance(data[eid].get("setup"), dict):
            data[eid]["setup"].update(setup)
        prepared[eid] = {"X": Xs, "y": ys, "setup": setup}
    return prepared, ground_truth


def train_rrr_baseline(data: dict, input_mod: str, idx=None, n_comp: int = 3, l2: float = 100., joint: bool = False,
                       device=None):
    """src/train_rrr.py's main() from the loaded dict on: prepare (prepare_rrr_inputs), fit and score.
    joint = False is the script's loop, one RRRGD per session; joint = True fits all sessions in one RRRGD with a
    shared V (train_model_main supports it; the script does not use it).
    Returns ({eid: {'gt', 'pred', 'co_bps': [per neuron], 'r2': [per neuron], 'eid'}}, mean co-bps): the
    reference's keys (train_rrr.py:230-236) and its 'mean bps' (the mean over sessions of each session's
    NaN-ignoring mean over neurons)."""
    prepared, ground_truth = prepare_rrr_inputs(data, input_mod, idx=idx, device=device)
    models = {}
    if joint:
        m = RRRGD(n_comp=n_comp, l2=l2).fit({eid: (p["X"][0], p["y"][0]) for eid, p in prepared.items()})
        models = {eid: m for eid in prepared}
    result, test_bps = {}, []
    for eid, p in prepared.items():
        m = models.get(eid) or RRRGD(n_comp=n_comp, l2=l2).fit({eid: (p["X"][0], p["y"][0])})
        gt = ground_truth[eid]
        s = m.score(eid, p["X"][1], p["setup"]["mean_y_TN"], p["setup"]["std_y_TN"], gt)
        test_bps.append(float(s["co_bps"]))
        result[eid] = {"gt": gt.cpu().numpy(), "pred": s["pred"].cpu().numpy(), "co_bps": s["bps"].cpu().tolist(),
                       "r2": s["r2"].cpu().tolist(), "eid": eid}
    return result, float(np.mean(test_bps))


def pixel_rrr_data(train_X, train_y, test_X, test_y, eid: str = "session") -> dict:
    """The dict `train_rrr_baseline(., 'whisker-video')` takes, from two videos (K, F, h w) or (K, F, c, h, w),
    uint8 or float32, numpy or torch, and the binned spikes (K, T, N) of the same trials, like pca.pca_rrr_data.
    Nothing is copied or converted here."""
    for X, y in ((train_X, train_y), (test_X, test_y)):
        if len(X.shape) not in (3, 5) or len(y.shape) != 3 or X.shape[0] != y.shape[0]:
            raise VsError("pixel_rrr_data: videos (K, F, h w) or (K, F, c, h, w) and spikes (K, T, N) of the same trials")
    return {eid: {"X": [train_X, test_X], "y": [train_y, test_y], "setup": {}}}
