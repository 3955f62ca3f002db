"""PCA video embeddings for the RRR baseline: the reference's `get_pca_embedding` (src/utils/utils.py:350-360,
driven by src/use_cebra.py:59-97 with use_pca = True), which is sklearn's PCA(n_components).fit_transform on the
(n t, h w) pixel matrix of a session's whisker video.

sklearn takes its randomized solver at these shapes.  Here the same subspace is found by a block subspace iteration
on the centred matrix Xc = X - 1 mu^T, whose two products per step stream the pixels, stored once as uint8 or
float32, through the exact-f32 MFMA (csrc/pca.hip: vs_pca_colmean, vs_pca_gram_apply, vs_pca_project):

    l = min(k + oversample, min(M - 1, D));  Q = qr(G) for a fixed seeded Gaussian G [D, l]
    each step:  W = Xc^T (Xc Q);  B = Q^T W;  B = S diag(theta) S^T;
                residual_i = |W s_i - theta_i Q s_i| / theta_1 for the top k;  Q = qr(W)
    stop when every residual is below tol, or after max_iter steps (converged_ = False, with a warning)
    Rayleigh-Ritz:  Y = Xc Q (float64 out),  Y^T Y = Z diag(sigma^2) Z^T,  components = (Q Z)[:, :k]^T
    sign rule: sklearn's svd_flip(u_based_decision=False), the entry of largest magnitude of a component is positive
    scores = Xc components^T (vs_pca_project), float64

The orthonormalisations and the l x l eigenproblems are float64 torch.linalg calls on D x l and l x l operands: host
plumbing, on the device where this torch build has a device QR / eigh and on the host otherwise (`linalg_device()`
says which; it is probed once, never switched silently in the middle of a fit).
"""
from __future__ import annotations

import time
import warnings

import numpy as np
import torch

from . import ops
from ._lib import VsError

MAX_COMPONENTS = 16
# 4 x the level at which the largest top-k residual stalls under f32 products in the CPU restatement
# (tests/pca_ref.py) on the three fixture geometries: DESIGN.md section 7 has the figures
DEFAULT_TOL = 1.3e-6
SEED = 0

_LINALG_DEVICE = None


def linalg_device(device) -> str:
    """'device' when torch.linalg.qr and eigh run on `device` in float64, else 'host'.  Probed once."""
    global _LINALG_DEVICE
    if _LINALG_DEVICE is None:
        try:
            a = torch.eye(3, dtype=torch.float64, device=device) * 2.0
            q, _ = torch.linalg.qr(a)
            w, _ = torch.linalg.eigh(a)
            ok = bool(torch.isfinite(q).all()) and bool(torch.isfinite(w).all())
            _LINALG_DEVICE = "device" if ok else "host"
        except RuntimeError:
            _LINALG_DEVICE = "host"
    return _LINALG_DEVICE


def sign_flip(components: torch.Tensor) -> torch.Tensor:
    """sklearn's svd_flip(u_based_decision=False) on components [k, D]: in every row the entry of largest magnitude
    becomes positive."""
    idx = components.abs().argmax(dim=1, keepdim=True)
    sign = torch.sign(components.gather(1, idx))
    sign = torch.where(sign == 0, torch.ones_like(sign), sign)
    return components * sign


def start_block(D: int, l: int) -> torch.Tensor:
    """The fixed starting block G [D, l] float64: a Gaussian from a torch generator of its own seeded with SEED, so
    it is the same on every call and touches no global generator."""
    g = torch.Generator(device="cpu")
    g.manual_seed(SEED)
    return torch.randn(D, l, generator=g, dtype=torch.float64)


def _as_matrix(X, device=None) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(X)) if isinstance(X, np.ndarray) else X
    if not torch.is_tensor(t) or t.dim() != 2:
        raise VsError("PCA: X must be a [M, D] numpy array or tensor")
    if t.dtype not in (torch.uint8, torch.float32):
        raise VsError(f"PCA: X must be uint8 or float32 (got {t.dtype}); the products run in f32, so a float64 "
                      "input would be rounded without the caller's saying so")
    dev = device or (t.device if t.is_cuda else "cuda")
    return t.to(dev).contiguous()


class PCA:
    """sklearn.decomposition.PCA(n_components)'s fit / transform / fit_transform on the device, for 1 <= k <= 16
    components of a [M, D] uint8 or float32 matrix (M >= 2 rows, k < min(M, D)).

    After fit: mean_ [D], components_ [k, D], singular_values_ [k], explained_variance_ [k] (S^2 / (M - 1)),
    float64 device tensors; n_iter_, converged_, residuals_ (the top-k residuals of the last step) and timing_
    (host-clock seconds: the whole fit, the host's time issuing the small linear algebra, its waits on the stop
    test; scripts/pca_bench.py measures the device's share of each)."""

    def __init__(self, n_components: int = 5, oversample: int = 10, max_iter: int = 60, tol: float = DEFAULT_TOL,
                 device=None):
        self.n_components, self.oversample = int(n_components), int(oversample)
        self.max_iter, self.tol, self.device = int(max_iter), float(tol), device
        if not 1 <= self.n_components <= MAX_COMPONENTS:
            raise VsError(f"PCA: {self.n_components} components, supported 1..{MAX_COMPONENTS}")
        if self.oversample < 0 or self.n_components + self.oversample > 32:
            raise VsError("PCA: oversample >= 0 and n_components + oversample <= 32 (the kernels' block width)")
        if self.max_iter < 1 or not self.tol > 0:
            raise VsError("PCA: max_iter >= 1 and tol > 0")
        self.mean_ = self.components_ = self.singular_values_ = self.explained_variance_ = None
        self.n_iter_, self.converged_, self.residuals_, self.timing_ = 0, False, None, {}

    # the float64 plumbing: on the device, or through the host where this torch has no device QR / eigh
    def _qr(self, A):
        if self._where == "device":
            return torch.linalg.qr(A)[0].contiguous()
        return torch.linalg.qr(A.cpu())[0].to(A.device).contiguous()

    def _eigh_desc(self, B):
        B = (B + B.t()) * 0.5
        if self._where == "device":
            w, S = torch.linalg.eigh(B)
        else:
            w, S = (t.to(B.device) for t in torch.linalg.eigh(B.cpu()))
        return w.flip(0), S.flip(1)

    def fit(self, X) -> "PCA":
        X = _as_matrix(X, self.device)
        M, D = X.shape
        k = self.n_components
        if M < 2 or k >= min(M, D):
            raise VsError(f"PCA: {k} components need a matrix with more than {k} rows and columns (got {M} x {D})")
        dev = X.device
        self._where = linalg_device(dev)
        l = min(k + self.oversample, min(M - 1, D))
        t_small = t_wait = 0.0
        torch.cuda.synchronize(dev)
        t_start = time.perf_counter()
        mu = ops.pca_colmean(X)
        ws = torch.empty(ops.pca_gram_apply_workspace_bytes(M, D, l) // 8 + 2, dtype=torch.float64, device=dev)
        W = torch.empty(D, l, dtype=torch.float64, device=dev)
        t0 = time.perf_counter()
        Q = self._qr(start_block(D, l).to(dev))
        t_small += time.perf_counter() - t0
        self.converged_, self.n_iter_ = False, 0
        for it in range(1, self.max_iter + 1):
            ops.pca_gram_apply(X, mu, Q, W=W, workspace=ws)
            t0 = time.perf_counter()
            theta, S = self._eigh_desc(Q.t() @ W)
            Sk = S[:, :k]
            res = torch.linalg.vector_norm(W @ Sk - (Q @ Sk) * theta[:k], dim=0) / theta[0]
            Qn = self._qr(W)
            t1 = time.perf_counter()
            stop = torch.cat([theta[:1], res]).cpu()            # the step's only wait on the stream
            t2 = time.perf_counter()
            t_small, t_wait = t_small + (t1 - t0), t_wait + (t2 - t1)
            self.n_iter_ = it
            if not (torch.isfinite(stop[0]) and stop[0] > 0):
                raise VsError("PCA: the matrix has zero total variance (every row equals the mean), or holds "
                              "values that are not finite")
            Q = Qn
            self.residuals_ = stop[1:].numpy().copy()
            if bool((stop[1:] < self.tol).all()):
                self.converged_ = True
                break
        if not self.converged_:
            warnings.warn(f"PCA: the subspace iteration did not reach tol = {self.tol:g} in {self.max_iter} steps "
                          f"(largest residual {float(self.residuals_.max()):.3g})", RuntimeWarning, stacklevel=2)
        # Rayleigh-Ritz on the last block, from the float64 Y
        Y = ops.pca_project(X, mu, Q)
        t0 = time.perf_counter()
        s2, Z = self._eigh_desc(Y.t() @ Y)
        comps = sign_flip((Q @ Z[:, :k]).t().contiguous())
        t_small += time.perf_counter() - t0
        self.mean_, self.components_ = mu, comps
        self.singular_values_ = s2[:k].clamp_min(0).sqrt()
        self.explained_variance_ = s2[:k].clamp_min(0) / (M - 1)
        torch.cuda.synchronize(dev)
        total = time.perf_counter() - t_start
        self.timing_ = {"total_s": total, "small_linalg_s": t_small, "wait_s": t_wait, "linalg": self._where}
        return self

    def transform(self, X) -> torch.Tensor:
        """The scores (X - mean_) components_^T, [M, k] float64 on the device."""
        if self.components_ is None:
            raise VsError("PCA.transform: call fit first")
        X = _as_matrix(X, self.components_.device)
        if X.shape[1] != self.components_.shape[1]:
            raise VsError(f"PCA.transform: X has {X.shape[1]} columns, the fit saw {self.components_.shape[1]}")
        if X.shape[0] < 2:
            raise VsError("PCA.transform: at least 2 rows")
        return ops.pca_project(X, self.mean_, self.components_.t().contiguous())

    def fit_transform(self, X) -> torch.Tensor:
        X = _as_matrix(X, self.device)
        return self.fit(X).transform(X)


def _as_video(video):
    t = torch.from_numpy(np.ascontiguousarray(video)) if isinstance(video, np.ndarray) else video
    if not torch.is_tensor(t) or t.dim() not in (4, 5) or (t.dim() == 5 and t.shape[2] != 1):
        raise VsError("pca_embedding: video must be (n, t, 1, h, w) or (n, t, h, w)")
    return t


def pca_embedding(video, out_dim: int = 5, device=None, **pca_args) -> torch.Tensor:
    """get_pca_embedding (utils.py:350-360): video (n, t, 1, h, w) or (n, t, h, w), uint8 or float32, numpy or
    tensor -> the PCA scores of its n t frames, (n, t, out_dim) float64 on the device."""
    v = _as_video(video)
    n, t = v.shape[:2]
    scores = PCA(n_components=out_dim, device=device, **pca_args).fit_transform(v.reshape(n * t, -1))
    return scores.reshape(n, t, out_dim)


def pca_rrr_data(train_X, train_y, test_X, test_y, out_dim: int = 5, eid: str = "session", device=None) -> dict:
    """use_cebra.py:59-76 with use_pca = True, from its loaded arrays on: the two splits' videos are concatenated
    along the trials, one PCA is fitted to all their frames, and the scores are split back.  Returns
    {eid: {'X': [train, test], 'y': [train_y, test_y], 'setup': {}}}, the dict train_rrr_baseline(data, 'pca')
    takes."""
    a, b = _as_video(train_X), _as_video(test_X)
    if a.shape[1:] != b.shape[1:] or a.dtype != b.dtype:
        raise VsError("pca_rrr_data: the two splits' videos must agree in everything but the number of trials")
    if len(train_y) != a.shape[0] or len(test_y) != b.shape[0]:
        raise VsError("pca_rrr_data: one row of y per trial of X in each split")
    dev = device or (a.device if a.is_cuda else "cuda")
    emb = pca_embedding(torch.cat([a.to(dev), b.to(dev)], dim=0), out_dim=out_dim, device=dev)
    return {eid: {"X": [emb[:a.shape[0]], emb[a.shape[0]:]], "y": [train_y, test_y], "setup": {}}}
