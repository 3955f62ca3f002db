"""CPU restatement of the reduced-rank regression validation for the tests.

TEST INFRASTRUCTURE ONLY.  A fresh float64 torch-CPU statement of what the reference's `train_rrr`
(src/utils/utils.py:376-456) and `RRRGD` (src/model/rrr.py) compute: the standardisation, the model and its loss,
the single L-BFGS step, and the scoring (clipped rates, bits per spike, sklearn's 1-D r2_score per trial).  It is
pinned: tests/golden/rrr.npz holds what the reference's own functions give on the inputs defined here
(scripts/gen_rrr_fixture.py), and tests/test_cpu_rrr.py holds this file to that fixture.

    beta[n,c,t] = sum_j U[n,c,j] V[j,t] (c < C),  beta[n,C,t] = b[n,0,t]
    yhat[k,t,n] = sum_c X[k,t,c] beta[n,c,t],     loss = sum (yhat - y)^2 + l2 sum beta^2   (b^2 included)
"""
import numpy as np
import torch

from oracle import prng

SEED = 21
L2, N_COMP = 100.0, 3
# K_train / K_val trials, T bins, N neurons, C features (A: N = 64 + 1, B: N = 64 + 6)
GEOMETRIES = {"A": dict(k_train=13, k_val=5, T=100, N=65, C=5, r=3),
              "B": dict(k_train=40, k_val=13, T=100, N=70, C=3, r=3)}
SILENT, SILENT_IN_TRAIN, SPARSE = 0, 1, 2     # neuron roles every geometry contains


def make_data(geom: str, seed: int = SEED) -> dict:
    """Raw inputs of a geometry, re-derived from (seed, name): X float64 (K, T, C) normal with a per-feature
    scale and offset, y float32 Poisson counts whose rates depend on X and on time.  Neuron SILENT never fires,
    SILENT_IN_TRAIN fires in the validation split only (its training std is clipped), SPARSE fires so rarely
    that most of its trials are silent (the SS_tot = 0 branch of r2_score); neuron 3 is silent in validation
    trial 0."""
    g = GEOMETRIES[geom]
    K, T, N, C = g["k_train"] + g["k_val"], g["T"], g["N"], g["C"]
    name = f"rrr.{geom}."
    z = prng.normal(seed, (K, T, C), name + "X").astype(np.float64)
    X = z * (1.0 + 0.25 * np.arange(C)) + 0.3 * np.arange(C)
    w = prng.normal(seed, (N, C), name + "w", std=0.5).astype(np.float64)
    a = prng.normal(seed, (N,), name + "a", std=0.6, mean=-0.7).astype(np.float64)
    phase = 2 * np.pi * prng.uniform(seed, N, name + "phase")
    a[SPARSE] = -4.5
    log_lam = a[None, None, :] + np.einsum("ktc,nc->ktn", z, w) \
        + 0.5 * np.sin(2 * np.pi * np.arange(T)[None, :, None] / T + phase[None, None, :])
    lam = np.clip(np.exp(log_lam), 0.005, 5.0)
    y = prng.poisson(seed, lam, name + "cnt")
    y[:, :, SILENT] = 0
    y[:g["k_train"], :, SILENT_IN_TRAIN] = 0
    y[g["k_train"], :, 3] = 0
    kt = g["k_train"]
    return {"X": [X[:kt], X[kt:]], "y": [y[:kt], y[kt:]], "setup": {}}


def standardise(data: dict):
    """utils.py:379-390 on the host, in the arrays' own dtypes (X float64, y float32): statistics of split 0,
    std clipped at 1e-8, applied to both splits; a column of ones appended to X."""
    def stats(a):
        return np.mean(a, axis=0), np.clip(np.std(a, axis=0), 1e-8, None)
    mean_X, std_X = stats(data["X"][0])
    mean_y, std_y = stats(data["y"][0])
    Xs = [np.concatenate([(x - mean_X) / std_X, np.ones(x.shape[:2] + (1,))], axis=2) for x in data["X"]]
    ys = [(v - mean_y) / std_y for v in data["y"]]
    return Xs, ys, mean_y, std_y


def init(T: int, N: int, C: int, r: int):
    rs = np.random.RandomState(0)
    U = rs.normal(size=(N, C, r)) / np.sqrt(T * r)
    V = rs.normal(size=(r, T)) / np.sqrt(T * r)
    return U, V


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64) if not torch.is_tensor(a) else a.to(torch.float64)


def predict(X, U, V, b):
    beta = torch.cat((_t(U) @ _t(V), _t(b)), 1)                               # (N, C+1, T)
    return torch.einsum("ktc,nct->ktn", _t(X), beta)


def loss(X, y, U, V, b, l2):
    U, V, b = _t(U), _t(V), _t(b)
    beta = torch.cat((U @ V, b), 1)
    res = torch.einsum("ktc,nct->ktn", _t(X), beta) - _t(y)
    return (res ** 2).sum() + l2 * (beta ** 2).sum()


def fit(X, y, r: int = N_COMP, l2: float = L2, U0=None, V0=None) -> dict:
    """One default torch L-BFGS step from the reference's initialisation; parameters in the order U, b, V.
    b is a parameter of y's dtype, as in the reference (rrr.py:44-47: b = mean_k y, float32 when y is): its
    gradient is rounded to that dtype and L-BFGS updates it in that dtype.  This matters: with a float64 b the
    fit ends 1e-6 (losses) / 3e-5 (U) away from the reference's, a hundred times the reference's own spread,
    because 20 L-BFGS iterations without a line search amplify a 1e-15 perturbation of b that far."""
    K, T, C1 = X.shape
    y = np.asarray(y)
    N = y.shape[2]
    if U0 is None:
        U0, V0 = init(T, N, C1 - 1, r)
    U = _t(U0).clone().requires_grad_(True)
    V = _t(V0).clone().requires_grad_(True)
    b = torch.from_numpy(np.ascontiguousarray(np.expand_dims(y.mean(0).T, 1))).requires_grad_(True)
    Xt, yt = _t(X), _t(y)
    opt = torch.optim.LBFGS([U, b, V])
    losses = []

    def closure():
        opt.zero_grad()
        beta = torch.cat((U @ V, b), 1)                                       # promotes b to float64
        v = ((torch.einsum("ktc,nct->ktn", Xt, beta) - yt) ** 2).sum() + l2 * (beta ** 2).sum()
        v.backward()
        losses.append(float(v.detach()))
        return v

    opt.step(closure)
    st = opt.state[U]
    return {"U": U.detach().numpy(), "V": V.detach().numpy(), "b": b.detach().double().numpy(),
            "losses": np.array(losses), "n_iter": int(st["n_iter"]), "func_evals": int(st["func_evals"])}


def score(X_val, U, V, b, mean_y, std_y, gt) -> dict:
    """utils.py:411-447: pred = clip(yhat std_y + mean_y, 1e-3); per neuron bits per spike over all (k, t) and
    the NaN-ignoring mean over trials of r2_score(gt[k, :, n], pred[k, :, n])."""
    gt = np.asarray(gt, dtype=np.float64)
    pred = predict(X_val, U, V, b).numpy() * np.asarray(std_y, np.float64) + np.asarray(mean_y, np.float64)
    pred = np.clip(pred, 1e-3, None)
    K, T, N = gt.shape
    S = gt.sum((0, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        null = S / (K * T)
        null = np.where(null == 0, 1e-9, null)
        nll_model = (pred - gt * np.log(pred)).sum((0, 1))                    # the log(n!) terms cancel
        nll_null = (null[None, None] - gt * np.log(null)[None, None]).sum((0, 1))
        bps = (nll_null - nll_model) / S / np.log(2)
        bps[np.isinf(bps)] = np.nan
        ss_res = ((gt - pred) ** 2).sum(1)                                    # (K, N)
        ss_tot = ((gt - gt.mean(1, keepdims=True)) ** 2).sum(1)
        r2_kn = np.where(ss_res == 0, 1.0, np.where(ss_tot == 0, 0.0, 1.0 - ss_res / np.where(ss_tot == 0, 1, ss_tot)))
    r2 = np.nanmean(r2_kn, axis=0)
    return {"pred": pred, "bps": bps, "r2": r2, "r2_kn": r2_kn, "co_bps": np.nanmean(bps), "r2_mean": np.nanmean(r2)}


def run(geom: str) -> dict:
    """The whole path on a geometry's data: standardise, fit, score."""
    g = GEOMETRIES[geom]
    data = make_data(geom)
    Xs, ys, mean_y, std_y = standardise(data)
    out = fit(Xs[0], ys[0], g["r"], L2)
    out.update(score(Xs[1], out["U"], out["V"], out["b"], mean_y, std_y, data["y"][1]))
    return out


# ---- distances to the fixture -------------------------------------------------------------------------------
def dist(a, b, scale=None):
    """max |a - b| / max |b| (or / scale), NaN positions required equal."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN positions differ"
    scale = np.nanmax(np.abs(b)) if scale is None else scale
    return float(np.nanmax(np.abs(a - b)) / scale)


def spreads(fx, geom):
    """The reference's own spread per quantity: its distance to its second run, whose fit saw the standardised
    training trials in another order.  b is judged against max |U V| (it sits at 1e-8 after standardisation,
    its own scale means nothing), pred absolutely (rates, clipped at 1e-3)."""
    uv = np.abs(fx[f"{geom}/U"] @ fx[f"{geom}/V"]).max()
    s = {k: dist(fx[f"{geom}/perm/{k}"], fx[f"{geom}/{k}"]) for k in ("losses", "U", "V", "bps", "r2")}
    s["b"] = dist(fx[f"{geom}/perm/b"], fx[f"{geom}/b"], scale=uv)
    s["co_bps"] = abs(float(fx[f"{geom}/perm/co_bps"] - fx[f"{geom}/co_bps"])) / abs(float(fx[f"{geom}/co_bps"]))
    s["pred"] = float(fx[f"{geom}/perm/pred_maxdiff"])
    return s


def distances(got, fx, geom, keys=("losses", "U", "V", "b", "bps", "r2", "co_bps", "pred"), label="restatement"):
    """Distances of a run's outputs to the fixture in the units of `spreads`; printed, so that a run with -s
    shows every figure before anything is asserted."""
    uv = np.abs(fx[f"{geom}/U"] @ fx[f"{geom}/V"]).max()
    s, d = spreads(fx, geom), {}
    for k in keys:
        if k == "b":
            d[k] = dist(got[k], fx[f"{geom}/b"], scale=uv)
        elif k == "co_bps":
            d[k] = abs(float(got[k]) - float(fx[f"{geom}/co_bps"])) / abs(float(fx[f"{geom}/co_bps"]))
        elif k == "pred":
            if f"{geom}/pred" in fx:
                d[k] = float(np.abs(np.asarray(got[k], np.float64) - fx[f"{geom}/pred"]).max())
        else:
            d[k] = dist(got[k], fx[f"{geom}/{k}"])
    for k, v in d.items():
        print(f"rrr {label} {geom} {k}: distance {v:.3e}, reference spread {s[k]:.3e} ({v / s[k]:.2g} x)")
    return d, s
