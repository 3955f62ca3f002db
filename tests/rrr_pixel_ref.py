"""CPU restatement of the RRR baseline on raw pixels for the tests: src/train_rrr.py with
input_mod == 'whisker-video'.

TEST INFRASTRUCTURE ONLY.  It adds to tests/rrr_baseline_ref.py only what the pixel branch has of its own: the
flatten of train_rrr.py:99-102 and numpy's statistics of a uint8 array (float64: np.mean sums the integers in
float64, np.std squares the float64 differences).  The smoothing, the standardisation, the bias column, the frame
selection (`rb.prepare` with an embedding mode), the fit (`rb.fit`) and the scoring (`rr.score`) are reused.
Inputs are re-derived from (seed, name) by oracle/prng.py, so tests/golden/rrr_pixel.npz
(scripts/gen_rrr_pixel_fixture.py) holds outputs only.
"""
import numpy as np

import rrr_baseline_ref as rb
import rrr_ref as rr
from oracle import prng

SEED = 47
GEOM = "X"
EID = "X"
# one session of uint8 frames (K, F, 1, H, W): C = 25 x 44 = 1100, just over the wide cap of 1024; T = 12 >= 9 (the
# smoothing radius is 8); F = 16 > T, 12 of the first 15 frames are drawn
H, W = 25, 44
C = H * W
K_TRAIN, K_VAL, F, T, N = 14, 5, 16, 12, 9
IDX_SEED = 3
LATENTS = 4
CONSTANT_PIXEL, SATURATED_PIXEL = 7, 8   # constant over every trial (std clipped to 1e-8) | 255 in most frames
SILENT, SILENT_IN_TRAIN, SPARSE = rr.SILENT, rr.SILENT_IN_TRAIN, rr.SPARSE
INPUT_MOD = "whisker-video"


def frame_idx() -> np.ndarray:
    """train_rrr.py:48-49's draw with a fixed seed: sort(choice(F - 1, T, replace=False))."""
    return np.sort(np.random.RandomState(IDX_SEED).choice(F - 1, T, replace=False))


def make_raw(seed: int = SEED) -> dict:
    """{EID: {'X': [train, val] uint8 (K, F, 1, H, W), 'y': [train, val] float32 counts (K, T, N), 'setup': {}}}.
    A frame is 128 + 40 (latents . patterns) / 2 + 12 noise, rounded and clipped to 0..255; the rates depend on the
    latents at the selected frames and on time.  Neuron roles are rrr_ref.make_data's (SILENT never fires,
    SILENT_IN_TRAIN fires in validation only, SPARSE rarely; neuron 3 is silent in validation trial 0)."""
    K = K_TRAIN + K_VAL
    idx = frame_idx()
    name = "rrrp.X."
    z = prng.normal(seed, (K, F, LATENTS), name + "z").astype(np.float64)
    pat = prng.normal(seed, (LATENTS, C), name + "pat").astype(np.float64)
    noise = prng.normal(seed, (K, F, C), name + "noise").astype(np.float64)
    pix = 128.0 + 40.0 * (z @ pat) / np.sqrt(LATENTS) + 12.0 * noise
    pix[:, :, CONSTANT_PIXEL] = 13.0
    pix[:, :, SATURATED_PIXEL] += 150.0
    pix[0, :, SATURATED_PIXEL] = 200.0             # never constant over the training trials of a frame
    X = np.clip(np.rint(pix), 0, 255).astype(np.uint8).reshape(K, F, 1, H, W)
    w = prng.normal(seed, (N, LATENTS), name + "w", std=0.5).astype(np.float64)
    a = prng.normal(seed, (N,), name + "a", std=0.6, mean=-0.7).astype(np.float64)
    phase = 2 * np.pi * prng.uniform(seed, N, name + "phase")
    a[SPARSE] = -4.5
    log_lam = a[None, None, :] + np.einsum("ktc,nc->ktn", z[:, idx], w) \
        + 0.5 * np.sin(2 * np.pi * np.arange(T)[None, :, None] / T + phase[None, None, :])
    y = prng.poisson(seed, np.clip(np.exp(log_lam), 0.005, 5.0), name + "cnt")
    y[:, :, SILENT] = 0
    y[:K_TRAIN, :, SILENT_IN_TRAIN] = 0
    y[K_TRAIN, :, 3] = 0
    kt = K_TRAIN
    return {EID: {"X": [np.ascontiguousarray(X[:kt]), np.ascontiguousarray(X[kt:])], "y": [y[:kt], y[kt:]],
                  "setup": {}}}


def flatten(data: dict) -> dict:
    """train_rrr.py:98-102: (n, t, c, h, w) -> (n, t, c h w), a view."""
    out = {}
    for eid, d in data.items():
        out[eid] = {"X": [x.reshape(x.shape[0], x.shape[1], -1) for x in d["X"]], "y": list(d["y"]), "setup": {}}
    return out


def stats_u8(a: np.ndarray):
    """utils.py:107-110 on a uint8 array, spelled out: float64 statistics, every sum ascending over the trials."""
    assert a.dtype == np.uint8
    s = np.zeros(a.shape[1:], np.float64)
    for k in range(a.shape[0]):
        s += a[k]
    mean = s / a.shape[0]
    q = np.zeros(a.shape[1:], np.float64)
    for k in range(a.shape[0]):
        d = a[k] - mean
        q += d * d
    return mean, np.clip(np.sqrt(q / a.shape[0]), 1e-8, None)


def prepare(data: dict = None, stats=stats_u8, smooth_fn=rb.smooth):
    """The flatten and rb.prepare's embedding branch (smoothing, standardisation, bias column, frame selection).
    Returns ({eid: {'X', 'y', 'setup'}}, ground_truth)."""
    return rb.prepare(flatten(make_raw() if data is None else data), INPUT_MOD, frame_idx(), smooth_fn=smooth_fn,
                      stats=lambda a: stats(a) if a.dtype == np.uint8 else rb._stats(a))


def run() -> dict:
    """The whole path: flatten, prepare, fit, score; rrr_ref.run's layout (one session)."""
    prepared, gt = prepare()
    p = prepared[EID]
    fit = rb.fit({EID: (p["X"][0], p["y"][0])})
    out = {k: fit[k] for k in ("V", "losses", "n_iter", "func_evals")}
    out.update(fit[EID])
    out.update(rr.score(p["X"][1], out["U"], out["V"], out["b"], p["setup"]["mean_y_TN"], p["setup"]["std_y_TN"],
                        gt[EID]))
    return out


KEYS = ("losses", "U", "V", "b", "bps", "r2", "co_bps", "pred")


def distances(got, fx, keys=KEYS, label="restatement"):
    """rrr_ref.distances on the fixture's only geometry: (distances to the reference's first run, its spreads)."""
    return rr.distances(got, fx, GEOM, keys=keys, label=f"pixel {label}")
