"""CPU restatement of the RRR baseline for the tests: src/train_rrr.py's preparation and the
multi-session RRRGD fit.

TEST INFRASTRUCTURE ONLY.  It extends tests/rrr_ref.py (imported for the loss, the scoring and the distances) by
  * the preparation of train_rrr.py:108-171 in numpy (smoothing, one-hot choice / block, standardisation, bias
    column, frame selection).  This is the script's own glue inside main(): it cannot be taken from the reference
    as a function, so it is restated here line by line and is pinned only through the outputs of geometry P;
  * gaussian_filter1d(., sigma, axis=1) in scipy's order of additions (`smooth`), bit-equal to scipy's outputs in
    the fixture;
  * the fit of several sessions sharing V (src/model/rrr.py:29-49,147-177), parameters in the reference's order
    [U_0, b_0, U_1, b_1, ..., V].
Inputs are re-derived from (seed, name) by oracle/prng.py, so tests/golden/rrr_baseline.npz
(scripts/gen_rrr_baseline_fixture.py) holds outputs only.
"""
import numpy as np
import torch

import rrr_ref as rr
from oracle import prng

SEED = 33
T, N_COMP, SMOOTH_W = 20, 3, 2
SILENT, SILENT_IN_TRAIN, SPARSE = rr.SILENT, rr.SILENT_IN_TRAIN, rr.SPARSE
# sessions: K_train / K_val trials, N neurons, C features of the raw X.  W: one wide session.  M: a narrow and a
# wide session (and a one-feature one) in one fit, sharing V, with different N, C and K.  P: the preparation:
# 24 frames, 4 continuous columns + choice (2 values) + block (3 values), input_mod 'all', 20 of 23 frames.
GEOMETRIES = {
    "W": dict(F=T, sessions={"W": dict(k_train=13, k_val=5, N=65, C=40)}),
    "M": dict(F=T, sessions={"M0": dict(k_train=9, k_val=4, N=65, C=5), "M1": dict(k_train=14, k_val=5, N=9, C=40),
                             "M2": dict(k_train=6, k_val=3, N=70, C=1)}),
    "P": dict(F=24, sessions={"P": dict(k_train=11, k_val=6, N=66, C=4)}, input_mod="all", idx_seed=5),
}
CHOICES, BLOCKS = (-1.0, 1.0), (0.2, 0.5, 0.8)
SMOOTH_INPUTS = {"a": ((7, 20, 9), np.float32), "b": ((3, 9, 70), np.float64)}     # b: T at the minimum, radius + 1


def frame_idx(geom: str) -> np.ndarray:
    """The T frames of F that reach the fit: all of them (W, M: F = T), or train_rrr.py:48-49's draw with a fixed
    seed (P)."""
    g = GEOMETRIES[geom]
    if g["F"] == T:
        return np.arange(T)
    return np.sort(np.random.RandomState(g["idx_seed"]).choice(g["F"] - 1, T, replace=False))


def make_raw(geom: str, seed: int = SEED) -> dict:
    """{eid: {'X': [train, val], 'y': [train, val], 'setup': {}}}: X float64 (K, F, C [+ 2]) normal with a
    per-feature scale and offset (P: + a choice and a block column, constant within a trial, every category in
    both splits), y float32 Poisson counts (K, T, N) whose rates depend on X at the selected frames and on time.
    The neuron roles are rrr_ref.make_data's: SILENT never fires, SILENT_IN_TRAIN fires in validation only,
    SPARSE fires rarely; neuron 3 is silent in validation trial 0."""
    g = GEOMETRIES[geom]
    F, idx, out = g["F"], frame_idx(geom), {}
    for eid, s in g["sessions"].items():
        kt, K, N, C = s["k_train"], s["k_train"] + s["k_val"], s["N"], s["C"]
        name = f"rrrb.{geom}.{eid}."
        z = prng.normal(seed, (K, F, C), name + "X").astype(np.float64)
        X = z * (1.0 + 0.25 * (np.arange(C) % 7)) + 0.3 * (np.arange(C) % 5)
        w = prng.normal(seed, (N, C), name + "w", std=1.1 / np.sqrt(C)).astype(np.float64)
        a = prng.normal(seed, (N,), name + "a", std=0.6, mean=-0.7).astype(np.float64)
        phase = 2 * np.pi * prng.uniform(seed, N, name + "phase")
        a[SPARSE] = -4.5
        log_lam = a[None, None, :] + np.einsum("ktc,nc->ktn", z[:, idx], w) \
            + 0.5 * np.sin(2 * np.pi * np.arange(T)[None, :, None] / T + phase[None, None, :])
        if "input_mod" in g:
            within = np.concatenate([np.arange(kt), np.arange(K - kt)])        # the trial's number in its split
            choice = np.array(CHOICES)[within % 2]
            block = np.array(BLOCKS)[within % 3]
            log_lam = log_lam + 0.3 * choice[:, None, None] + 0.5 * (block[:, None, None] - 0.5)
            X = np.concatenate([X, np.broadcast_to(choice[:, None, None], (K, F, 1)),
                                np.broadcast_to(block[:, None, None], (K, F, 1))], axis=2)
        lam = np.clip(np.exp(log_lam), 0.005, 5.0)
        y = prng.poisson(seed, lam, name + "cnt")
        y[:, :, SILENT] = 0
        y[:kt, :, SILENT_IN_TRAIN] = 0
        y[kt, :, 3] = 0
        out[eid] = {"X": [np.ascontiguousarray(X[:kt]), np.ascontiguousarray(X[kt:])], "y": [y[:kt], y[kt:]],
                    "setup": {}}
    return out


def smooth_input(name: str) -> np.ndarray:
    shape, dtype = SMOOTH_INPUTS[name]
    lam = np.clip(np.exp(prng.normal(SEED, shape, f"rrrb.smooth.{name}.rate").astype(np.float64)), 0.01, 6.0)
    return prng.poisson(SEED, lam, f"rrrb.smooth.{name}.cnt").astype(dtype)


def gauss_weights(sigma: float):
    """scipy's _gaussian_kernel1d (order 0, truncate 4): (weights [2 radius + 1] float64, radius)."""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum(), radius


def smooth(y: np.ndarray, sigma: float = SMOOTH_W) -> np.ndarray:
    """scipy.ndimage.gaussian_filter1d(y, sigma, axis=1), mode 'reflect', in scipy's order: the line in float64,
    the centre tap first, then the pairs from the outermost to the innermost, product and sum rounded
    separately; one rounding to y's dtype at the end."""
    w, R = gauss_weights(sigma)
    K, Tn, N = y.shape
    assert Tn >= R + 1, "a single reflection at each end"
    line = y.astype(np.float64)
    t = np.arange(Tn)

    def at(i):
        i = np.where(i < 0, -i - 1, i)
        return line[:, np.where(i >= Tn, 2 * Tn - 1 - i, i)]
    acc = line * w[R]
    for j in range(R, 0, -1):
        acc = (at(t - j) + at(t + j)) * w[R - j] + acc
    return acc.astype(y.dtype)


def _one_hot(arr, frames):
    """utils.py:114-119."""
    uni = np.sort(np.unique(arr))
    ret = np.zeros((len(arr), frames, len(uni)))
    for i, u in enumerate(uni):
        ret[:, :, i] = (arr == u)
    return ret


def _stats(a):
    return np.mean(a, axis=0), np.clip(np.std(a, axis=0), 1e-8, None)          # utils.py:107-110


def prepare(data: dict, input_mod: str, idx, smooth_w=SMOOTH_W, smooth_fn=smooth, one_hot=_one_hot, stats=_stats):
    """train_rrr.py:108-171 (the glue of main(), restated; the reference's hard-coded 120 frames are X's own
    frame count here).  Returns ({eid: {'X', 'y', 'setup'}}, ground_truth); the inputs are left alone."""
    embedding = ("cebra", "pca", "ws", "whisker-video", "vit", "cm", "m", "c")
    out, ground_truth = {}, {}
    for eid in sorted(data):                                                    # :112
        X, y = list(data[eid]["X"]), list(data[eid]["y"])
        ground_truth[eid] = y[1]                                                # :116
        for i in range(2):
            y[i] = smooth_fn(y[i], smooth_w)                                    # :118
            if input_mod in embedding:                                          # :119-127
                if input_mod == "m":
                    X[i] = X[i][..., :3]
                continue
            if input_mod != "me" and input_mod != "of-2d":                      # :129-141
                inp = X[i]
                choice, block = inp[:, 0, -2:-1], inp[:, 0, -1:]
                const = 3 if input_mod in ("me-all", "of-all") else 2
                contin_dim = inp.shape[2] - const
                X[i] = np.concatenate([one_hot(choice, inp.shape[1]), one_hot(block, inp.shape[1]),
                                       inp[..., -2 - contin_dim:-2]], axis=2)
        mean_X, std_X = stats(X[0])                                             # :144-145
        mean_y, std_y = stats(y[0])
        for i in range(2):
            K, F = X[i].shape[:2]
            X[i] = np.concatenate([(X[i] - mean_X) / std_X, np.ones((K, F, 1))], axis=2)[:, idx]   # :151-163
            y[i] = (y[i] - mean_y) / std_y                                      # :165
        out[eid] = {"X": X, "y": y, "setup": {"mean_X_Tv": mean_X, "std_X_Tv": std_X, "mean_y_TN": mean_y,
                                              "std_y_TN": std_y}}
    return out, ground_truth


def standardised(geom: str) -> dict:
    """The sessions of W / M as the fit and the scoring take them: rrr_ref.standardise per session (no smoothing,
    every frame).  {eid: {'X': [..], 'y': [..], 'mean_y', 'std_y', 'gt'}}."""
    out = {}
    for eid, d in make_raw(geom).items():
        Xs, ys, mean_y, std_y = rr.standardise(d)
        out[eid] = {"X": Xs, "y": ys, "mean_y": mean_y, "std_y": std_y, "gt": d["y"][1]}
    return out


def fit(sessions: dict, r: int = N_COMP, l2: float = rr.L2) -> dict:
    """rrr_ref.fit for several sessions {eid: (X, y)} sharing V.  rrr.py:35-49: one RandomState(0), per session in
    dict order a U and then a V draw, the last V kept; every b a parameter of its y's dtype.  One default L-BFGS
    step over [U_0, b_0, U_1, b_1, ..., V]; the closure is train_model's (rrr.py:165-175): per session the squared
    error summed per neuron and then over neurons, plus the l2 term, added in session order."""
    rs = np.random.RandomState(0)
    U, b, Xt, yt = {}, {}, {}, {}
    V0 = None
    for eid, (X, y) in sessions.items():
        K, Tn, C1 = X.shape
        y = np.asarray(y)
        N = y.shape[2]
        U0 = rs.normal(size=(N, C1 - 1, r)) / np.sqrt(Tn * r)
        V0 = rs.normal(size=(r, Tn)) / np.sqrt(Tn * r)
        U[eid] = torch.from_numpy(U0).requires_grad_(True)
        b[eid] = torch.from_numpy(np.ascontiguousarray(np.expand_dims(y.mean(0).T, 1))).requires_grad_(True)
        Xt[eid], yt[eid] = torch.from_numpy(np.ascontiguousarray(X)), torch.from_numpy(np.ascontiguousarray(y))
    V = torch.from_numpy(V0).requires_grad_(True)
    params = [p for eid in sessions for p in (U[eid], b[eid])] + [V]
    opt = torch.optim.LBFGS(params)
    losses = []

    def closure():
        opt.zero_grad()
        betas = {eid: torch.cat((U[eid] @ V, b[eid]), 1) for eid in sessions}
        mses = {eid: torch.sum((torch.einsum("ktc,nct->ktn", Xt[eid], betas[eid]) - yt[eid]) ** 2, axis=(0, 1))
                for eid in sessions}
        total = 0.0
        for eid in sessions:
            total = total + mses[eid].sum()
            total = total + l2 * torch.sum(betas[eid] ** 2)
        total.backward()
        losses.append(float(total.detach()))
        return total

    opt.step(closure)
    st = opt.state[params[0]]
    out = {"V": V.detach().numpy(), "losses": np.array(losses), "n_iter": int(st["n_iter"]),
           "func_evals": int(st["func_evals"])}
    for eid in sessions:
        out[eid] = {"U": U[eid].detach().numpy(), "b": b[eid].detach().double().numpy()}
    return out


def run(geom: str) -> dict:
    """The whole path on a geometry: W / M standardise, fit, score; P prepare, fit, score."""
    g = GEOMETRIES[geom]
    if "input_mod" in g:
        prepared, gt = prepare(make_raw(geom), g["input_mod"], frame_idx(geom))
        sess = {eid: {"X": p["X"], "y": p["y"], "mean_y": p["setup"]["mean_y_TN"], "std_y": p["setup"]["std_y_TN"],
                      "gt": gt[eid]} for eid, p in prepared.items()}
    else:
        sess = standardised(geom)
    out = fit({eid: (s["X"][0], s["y"][0]) for eid, s in sess.items()})
    for eid, s in sess.items():
        out[eid].update(rr.score(s["X"][1], out[eid]["U"], out["V"], out[eid]["b"], s["mean_y"], s["std_y"], s["gt"]))
    return out


# ---- distances to the fixture -------------------------------------------------------------------------------
KEYS = ("losses", "U", "V", "b", "bps", "r2", "co_bps", "pred")


def _measure(a, fx, geom, keys):
    """Distances of a run (`a`: this module's layout, or None for the fixture's second run) to the fixture's first
    run, in rrr_ref's units; per key the largest over the sessions."""
    def second(k, eid=None):
        return fx[f"{geom}/perm/{k}" if eid is None else f"{geom}/perm/{eid}/{k}"]
    d = {}
    for k in keys:
        if k in ("losses", "V"):
            d[k] = rr.dist(a[k] if a is not None else second(k), fx[f"{geom}/{k}"])
            continue
        per = []
        for eid in GEOMETRIES[geom]["sessions"]:
            first = lambda q: fx[f"{geom}/{eid}/{q}"]                           # noqa: E731
            if k == "pred":
                if a is None:
                    per.append(float(second("pred_maxdiff", eid)))
                elif f"{geom}/{eid}/pred" in fx:
                    per.append(float(np.abs(np.asarray(a[eid]["pred"], np.float64) - first("pred")).max()))
                continue
            v = a[eid][k] if a is not None else second(k, eid)
            if k == "b":
                per.append(rr.dist(v, first("b"), scale=np.abs(first("U") @ fx[f"{geom}/V"]).max()))
            elif k == "co_bps":
                per.append(abs(float(v) - float(first(k))) / abs(float(first(k))))
            else:
                per.append(rr.dist(v, first(k)))
        if per:
            d[k] = max(per)
    return d


def spreads(fx, geom, keys=KEYS):
    """The reference's own spread per quantity: its distance to its second run, whose fit saw the standardised
    training trials of every session in another order."""
    return _measure(None, fx, geom, keys)


def distances(got, fx, geom, keys=KEYS, label="restatement"):
    """(distances of a run to the fixture, the reference's spreads); printed, so that a run with -s shows every
    figure before anything is asserted."""
    d, s = _measure(got, fx, geom, keys), spreads(fx, geom, keys)
    for k, v in d.items():
        print(f"rrr baseline {label} {geom} {k}: distance {v:.3e}, reference spread {s[k]:.3e} ({v / s[k]:.2g} x)")
    return d, s
