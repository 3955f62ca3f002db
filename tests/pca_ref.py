"""CPU restatement of the PCA video embedding for the tests and the fixture generator.

TEST INFRASTRUCTURE ONLY.  Numpy statements of
  * the exact answer: the PCA of the float64 pixel matrix by a full SVD, with sklearn's sign rule (`exact_pca`);
  * the block subspace iteration of vspike/pca.py with its two products in float32 (numpy's sgemm on the centred
    matrix rounded to float32, which is what the f32 MFMA kernels compute up to the order of the sums) and the small
    problems in float64 (`subspace_pca`).  The starting block is numpy's RandomState(0) here and a torch generator in
    the product: the answer does not depend on it beyond the stopping tolerance.
tests/golden/pca.npz (scripts/gen_pca_fixture.py) holds the three videos made by `make_video`, the exact answer as
sklearn's PCA(svd_solver='full') gives it, and the reference's own get_pca_embedding outputs under 8 seeds.
"""
import numpy as np

SEED = 47
K_COMP = 5
# (n, t, h, w): M = n t frames of D = h w pixels.  max(M, D) > 500 and k < 0.8 min(M, D), so sklearn's 'auto' takes
# the randomized solver, the reference's real path.  B: D = 703 is odd, and two of its latents have nearly equal
# strength (singular values 2 and 3 within 4 %).  C carries the end-to-end RRR run.
GEOMETRIES = {"A": (7, 12, 22, 26), "B": (5, 24, 37, 19), "C": (9, 30, 20, 52)}
LATENT_GAIN = {"A": (60.0, 38.0, 25.0, 16.0, 10.5, 4.0, 2.5), "B": (60.0, 33.0, 32.0, 18.0, 11.0, 4.0, 2.5),
               "C": (60.0, 40.0, 27.0, 18.0, 12.0, 4.0, 2.5)}
# white noise per geometry: its largest singular value, NOISE (sqrt(M) + sqrt(D)), sits at about half the fifth
# latent's, so that sklearn's randomized solver (7 power iterations at this k) stays visibly short of the exact answer
NOISE = {"A": 10.0, "B": 12.0, "C": 16.0}
# the end-to-end run on geometry C: trials in the train split, neurons, bins, and the frame draw's seed
C_TRAIN, C_NEURONS, C_BINS, C_IDX_SEED = 6, 9, 20, 5


def make_video(geom: str, seed: int = SEED) -> np.ndarray:
    """(n, t, 1, h, w) uint8: smooth temporal latents times smooth spatial maps around a mean image, plus white noise,
    clipped to 0..255."""
    n, t, h, w = GEOMETRIES[geom]
    rs = np.random.RandomState(seed + sum(map(ord, geom)))
    gains = LATENT_GAIN[geom]
    M, D = n * t, h * w
    tt = np.arange(M) / M
    yy, xx = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    mean = 120.0 + 40.0 * np.exp(-(yy ** 2 + xx ** 2))
    lats, maps = [], []
    for j in range(len(gains)):
        f, ph = 1.0 + 0.7 * j + rs.uniform(0, 0.3), rs.uniform(0, 2 * np.pi)
        lat = np.sin(2 * np.pi * f * tt + ph) + 0.3 * rs.normal(size=M).cumsum() / np.sqrt(M)
        lats.append(lat - lat.mean())
        cy, cx, s = rs.uniform(-0.7, 0.7), rs.uniform(-0.7, 0.7), rs.uniform(0.25, 0.6)
        sp = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) * np.cos(3 * (j + 1) * xx + rs.uniform(0, 3))
        maps.append(sp.reshape(D))
    # orthonormal latents and maps (still smooth: Gram-Schmidt of smooth functions), so the signal's singular
    # values are the gains times sqrt(M D) / 4 and their ratios are what LATENT_GAIN says
    lats = np.linalg.qr(np.stack(lats, axis=1))[0] * np.sqrt(M)
    maps = np.linalg.qr(np.stack(maps, axis=1))[0] * np.sqrt(D) * 0.5
    frames = np.broadcast_to(mean.reshape(1, D), (M, D)) + 0.5 * (lats * np.asarray(gains)) @ maps.T
    frames = frames + NOISE[geom] * rs.normal(size=(M, D))
    return np.clip(np.rint(frames), 0, 255).astype(np.uint8).reshape(n, t, 1, h, w)


def sign_flip(components: np.ndarray) -> np.ndarray:
    """sklearn's svd_flip(u_based_decision=False): the entry of largest magnitude of every row becomes positive."""
    idx = np.abs(components).argmax(axis=1)
    sign = np.sign(components[np.arange(len(components)), idx])
    sign[sign == 0] = 1.0
    return components * sign[:, None]


def sign_margin(components: np.ndarray) -> np.ndarray:
    """Per component, the relative gap between its two largest |entries|: the sign rule is a coin toss at 0."""
    a = np.sort(np.abs(components), axis=1)
    return (a[:, -1] - a[:, -2]) / a[:, -1]


def exact_pca(X: np.ndarray, k: int = K_COMP) -> dict:
    """The PCA of X [M, D] in float64 by a full SVD of the centred matrix."""
    X = np.asarray(X, np.float64)
    mean = X.mean(axis=0)
    Xc = X - mean
    _, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    comps = sign_flip(Vt[:k])
    return {"mean": mean, "components": comps, "singular_values": S[:k], "scores": Xc @ comps.T,
            "explained_variance": S[:k] ** 2 / (X.shape[0] - 1), "all_singular_values": S}


def subspace_pca(X: np.ndarray, k: int = K_COMP, oversample: int = 10, max_iter: int = 60, tol: float = 1.3e-6,
                 products=np.float32, seed: int = 0) -> dict:
    """vspike/pca.py's iteration with the two products in `products` precision (float32: the kernels' arithmetic;
    float64: the iteration's own limit).  `history` holds the largest top-k residual of every step."""
    X64 = np.asarray(X, np.float64)
    M, D = X64.shape
    mean = X64.mean(axis=0)
    Xc = (X64 - mean).astype(products)                       # x - mu in float64, rounded once

    def project(Q):
        return (Xc @ Q.astype(products)).astype(np.float64)

    def gram_apply(Q):
        Y = Xc @ Q.astype(products)                          # kept in the products' precision, as in the workspace
        return (Xc.T @ Y).astype(np.float64)

    def eigh_desc(B):
        w, S = np.linalg.eigh((B + B.T) * 0.5)
        return w[::-1], S[:, ::-1]

    l = min(k + oversample, min(M - 1, D))
    Q = np.linalg.qr(np.random.RandomState(seed).normal(size=(D, l)))[0]
    history, converged, n_iter, res = [], False, 0, None
    for it in range(1, max_iter + 1):
        W = gram_apply(Q)
        theta, S = eigh_desc(Q.T @ W)
        if not theta[0] > 0:
            raise ValueError("zero total variance")
        Sk = S[:, :k]
        res = np.linalg.norm(W @ Sk - (Q @ Sk) * theta[:k], axis=0) / theta[0]
        Q = np.linalg.qr(W)[0]
        history.append(float(res.max()))
        n_iter = it
        if (res < tol).all():
            converged = True
            break
    Y = project(Q)
    s2, Z = eigh_desc(Y.T @ Y)
    comps = sign_flip((Q @ Z[:, :k]).T)
    sv = np.sqrt(np.clip(s2[:k], 0, None))
    return {"mean": mean, "components": comps, "singular_values": sv, "scores": project(comps.T.copy()),
            "explained_variance": sv ** 2 / (M - 1), "n_iter": n_iter, "converged": converged,
            "residuals": res, "history": np.array(history)}


def score_distance(z, Z) -> float:
    """max |z - Z| / max |Z|: the distance of a set of scores (or singular values) to the exact ones."""
    z, Z = np.asarray(z, np.float64), np.asarray(Z, np.float64)
    return float(np.abs(z - Z).max() / np.abs(Z).max())


def c_spikes(seed: int = SEED) -> np.ndarray:
    """Geometry C's spike counts (n, C_BINS, C_NEURONS) float32: Poisson with rates driven by the trial's mean
    frame brightness pattern through the video's own exact PCA scores, so the embedding predicts them."""
    n, t, h, w = GEOMETRIES["C"]
    X = make_video("C", seed).reshape(n * t, h * w)
    z = exact_pca(X)["scores"].reshape(n, t, K_COMP)
    z = z / np.abs(z).max()
    rs = np.random.RandomState(seed + 1)
    wgt = rs.normal(size=(K_COMP, C_NEURONS)) * 0.9
    base = rs.uniform(-0.4, 0.6, size=C_NEURONS)
    zb = z[:, np.linspace(0, t - 2, C_BINS).astype(int)]                     # (n, bins, k)
    lam = np.exp(base[None, None] + zb @ wgt)
    return rs.poisson(np.clip(lam, 0.05, 6.0)).astype(np.float32)


def c_frame_idx() -> np.ndarray:
    """The C_BINS frames of geometry C's t that reach the fit: train_rrr.py:48-49's draw with a fixed seed."""
    t = GEOMETRIES["C"][1]
    return np.sort(np.random.RandomState(C_IDX_SEED).choice(t - 1, C_BINS, replace=False))
