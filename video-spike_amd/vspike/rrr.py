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
"""
from __future__ import annotations

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
    """One session's RRRGD.  `fit(X, y)` takes standardised device tensors: X [K, T, C+1] float64 with a last
    column of ones, y [K, T, N] float32 or float64."""

    def __init__(self, n_comp: int = 3, l2: float = 100.):
        self.n_comp, self.l2 = int(n_comp), float(l2)
        self.flat = None
        self.losses, self.n_iter, self.func_evals = [], 0, 0

    # views of the flat parameter tensor, ordered [U, b, V] like the reference's ParameterDict
    def _views(self, flat):
        N, C, r, T = self.N, self.C, self.n_comp, self.T
        nu, nb = N * C * r, N * T
        return flat[:nu].view(N, C, r), flat[nu:nu + nb].view(N, 1, T), flat[nu + nb:].view(r, T)

    @property
    def U(self):
        return self._views(self.flat)[0]

    @property
    def b(self):
        return self._views(self.flat)[1]

    @property
    def V(self):
        return self._views(self.flat)[2]

    def _check(self, X, y):
        if X.dim() != 3 or y.dim() != 3 or X.shape[:2] != y.shape[:2]:
            raise VsError("RRR: X [K, T, C+1] and y [K, T, N]")
        check_dims(X.shape[2] - 1, self.n_comp)
        if X.dtype != torch.float64:
            raise VsError("RRR: X must be float64 (the reference's bias column makes it so)")

    def fit(self, X: torch.Tensor, y: torch.Tensor) -> "RRR":
        """The kernel-side parameters live in one flat float64 tensor ordered [U, b, V]; L-BFGS drives U and V as
        views of it.  b's master copy is a separate parameter of y's dtype, because the reference's is
        (rrr.py:44-47: b = mean_k y, float32 when y is): autograd rounds its gradient to that dtype and L-BFGS
        updates it in that dtype.  Keeping b in float64 instead moves the fit a hundred times further from the
        reference's than the reference moves under a reordering of its trials, so the
        closure copies b into the flat tensor before the kernel and db out of it afterwards (N T elements)."""
        self._check(X, y)
        X, y = X.contiguous(), y.contiguous()
        K, T, C1 = X.shape
        self.N, self.C, self.T = y.shape[2], C1 - 1, T
        U0, V0 = init_params(T, self.N, self.C, self.n_comp)
        dev = X.device
        b_master = _mean_trials(y).t().unsqueeze(1).contiguous().requires_grad_(True)    # rrr.py:44
        self.flat = torch.cat([torch.from_numpy(U0).reshape(-1).to(dev), b_master.detach().reshape(-1).double(),
                               torch.from_numpy(V0).reshape(-1).to(dev)])
        grad = torch.zeros_like(self.flat)
        U, b64, V = self._views(self.flat)
        dU, db64, dV = self._views(grad)
        U.requires_grad_(True)
        V.requires_grad_(True)
        U.grad, V.grad, b_master.grad = dU, dV, torch.zeros_like(b_master)
        ws = torch.empty(ops.rrr_loss_grad_workspace_bytes(K, T, self.N, self.C) // 8 + 2, dtype=torch.float64,
                         device=dev)
        losses = []

        def closure():
            with torch.no_grad():
                b64.copy_(b_master)
                loss = torch.empty(1, dtype=torch.float64, device=dev)
                ops.rrr_loss_grad(X, y, U, V, b64, self.l2, loss, dU=dU, dV=dV, db=db64, workspace=ws)
                b_master.grad.copy_(db64)
            losses.append(loss)
            return loss[0]

        opt = torch.optim.LBFGS([U, b_master, V])                            # rrr.py:199
        opt.step(closure)                                                    # rrr.py:177
        st = opt.state[U]
        self.n_iter, self.func_evals = int(st["n_iter"]), int(st["func_evals"])
        self.losses = torch.cat(losses).cpu().numpy()
        with torch.no_grad():
            b64.copy_(b_master)
        self.flat = self.flat.detach()
        return self

    def mse(self, X: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """sum (yhat - y)^2 over everything: the reference's `mse_val_mean` (rrr.py:180-181), a device scalar."""
        self._check(X, y)
        loss = torch.empty(1, dtype=torch.float64, device=X.device)
        ops.rrr_loss_grad(X.contiguous(), y.contiguous(), self.U, self.V, self.b, 0.0, loss)
        return loss[0]

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
        dev = X.device
        K, T, N = gt.shape
        pred = torch.empty(K, T, N, dtype=torch.float64, device=dev) if want_pred else None
        bps, r2 = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(2))
        out = torch.empty(2, dtype=torch.float64, device=dev)
        ops.rrr_score(X.contiguous(), self.U, self.V, self.b, mean_y.to(torch.float64).contiguous(),
                      std_y.to(torch.float64).contiguous(), gt.contiguous(), bps, r2, out, pred=pred)
        return {"pred": pred, "bps": bps, "r2": r2, "co_bps": out[0], "r2_mean": out[1]}

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
