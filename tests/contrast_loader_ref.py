"""Float64 restatement of the contrastive loader's frame transform, written from its definition, and the seeded
inputs the fixture (scripts/gen_contrast_loader_fixture.py -> tests/golden/contrast_loader.npz) and the tests share.

The transform is torchvision 0.17's for a float tensor, `Normalize([mean], [std])(Resize((S, S))(x))` with
x = float32(pixel) / 255 and Resize = F.interpolate(x, (S, S), mode="bilinear", align_corners=False, antialias=True):
a separable triangle filter, width first, then height.  Per axis and output index i

    scale = n_in / n_out, support = max(scale, 1), center = scale (i + 0.5)
    xmin = max(int(center - support + 0.5), 0), xsize = min(int(center + support + 0.5), n_in) - xmin
    w_j = max(0, 1 - |(j + xmin - center + 0.5) / support|) / (their sum),    j = 0 .. xsize - 1

Everything after the float32 pixel scaling is float64 here and nothing is rounded on the way, so this is the exact
filter up to float64 rounding: the yardstick both torch's float32 result (the fixture's d_ref) and the kernel's are
measured against.
"""
import numpy as np

MEAN, STD = 0.5, 0.5
# (H, W, S) of the kernel cases beside the fixture's sessions: the 8x limit (16 taps) | one pixel | one
# more / one less than the output (windows cut at both edges, a tail band)
EXTRA_GEOMETRIES = [(7, 192, 24), (1, 1, 24), (145, 143, 144)]
EXTRA_FRAMES = 3


def axis_windows(n_in: int, n_out: int):
    """(xmin [n_out], xsize [n_out]) of the filter windows."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    center = scale * (np.arange(n_out, dtype=np.float64) + 0.5)
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    return xmin, xmax - xmin


def axis_matrix(n_in: int, n_out: int) -> np.ndarray:
    """The dense (n_out, n_in) float64 matrix of the normalised weights."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    xmin, xsize = axis_windows(n_in, n_out)
    M = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        center = scale * (i + 0.5)
        j = np.arange(xsize[i], dtype=np.float64)
        w = np.maximum(0.0, 1.0 - np.abs((j + xmin[i] - center + 0.5) / support))
        M[i, xmin[i]:xmin[i] + xsize[i]] = w / w.sum()
    return M


def transform(frames, size: int, mean: float = MEAN, std: float = STD) -> np.ndarray:
    """frames (G, 1, H, W) uint8 or float32 -> (G, 1, size, size) float64."""
    f = np.asarray(frames)
    assert f.ndim == 4 and f.shape[1] == 1
    x = (f.astype(np.float32) / np.float32(255.0)).astype(np.float64)[:, 0]     # the reference's div_(255.0) in f32
    Wx, Wy = axis_matrix(f.shape[3], size), axis_matrix(f.shape[2], size)
    wide = x @ Wx.T                                                             # width first (G, H, S)
    out = np.einsum("yh,ghx->gyx", Wy, wide)                                    # then height (G, S, S)
    return ((out - mean) / std)[:, None]


def identity_expected(frames, mean: float = MEAN, std: float = STD) -> np.ndarray:
    """What H == W == S must give bit for bit: (float32(p) / 255 - mean) / std in float32 operations."""
    x = np.asarray(frames).astype(np.float32) / np.float32(255.0)
    return (x - np.float32(mean)) / np.float32(std)


def noise_frames(H: int, W: int, n: int, seed: int) -> np.ndarray:
    """(n, 1, H, W) uint8 noise (numpy's frozen legacy generator: the same bytes everywhere)."""
    return np.random.RandomState(seed).randint(0, 256, size=(n, 1, H, W)).astype(np.uint8)


def extra_frames(H: int, W: int, S: int) -> np.ndarray:
    return noise_frames(H, W, EXTRA_FRAMES, 7000 + 131 * H + 17 * W + S)


# ---- seeded tiny sessions: the dict `load_h5_file` returns for one session ---------------------------------------
SESSIONS = {
    # name: frame (H, W), output size, trials per split, frames per trial, time bins, neurons, seed
    "A": dict(H=20, W=28, S=24, splits=(4, 2, 2), t=6, T=5, N=7, seed=101),
    "B": dict(H=40, W=19, S=24, splits=(4, 2, 2), t=6, T=5, N=7, seed=202),
}
BATCH = 5               # 48 frames: nine batches of 5 and one of 3
IDX_OFFSET = 4
TIME_OFFSET = 0.06      # seconds: a handful of frames at 60 frames per second with jitter
EPOCHS = {"A": ("idx", 2, 11), "B": ("time", 1, 12)}     # mode, epochs recorded, seed of torch and numpy


def make_session(name: str) -> dict:
    """Splits of uint8 noise video, Poisson spikes and timestamps that interleave the trials: every frame has
    its own time, a trial's frames are not consecutive in time, so the sort permutes across the splits."""
    g = SESSIONS[name]
    rs = np.random.RandomState(g["seed"])
    n, t = sum(g["splits"]), g["t"]
    times = np.cumsum(rs.uniform(0.5, 1.5, size=n * t)) / 60.0
    times = times[rs.permutation(n * t)].reshape(n, t)
    video = rs.randint(0, 256, size=(n, t, 1, g["H"], g["W"])).astype(np.uint8)
    spikes = rs.poisson(1.5, size=(n, g["T"], g["N"])).astype(np.float32)
    out, lo = {}, 0
    for split, k in zip(("train", "val", "test"), g["splits"]):
        out[f"{split}_X"] = video[lo:lo + k]
        out[f"{split}_y"] = spikes[lo:lo + k]
        out[f"{split}_timestamp"] = times[lo:lo + k]
        lo += k
    return out


def peek_numpy() -> float:
    """numpy's global generator's next draw, without advancing it."""
    st = np.random.get_state()
    v = float(np.random.rand())
    np.random.set_state(st)
    return v
