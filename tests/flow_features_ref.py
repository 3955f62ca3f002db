"""Restatement of the behaviour features (vspike.behaviour) written from their definitions, and the seeded inputs the
fixture (scripts/gen_flow_features_fixture.py -> tests/golden/flow_features.npz) and the tests share.

The reference's get_optic_flow (src/utils/ibl_data_utils.py:1103-1243) computes, per trial,

    me    = mean_{h,w} |video[f + 1] - video[f]|
    med_c = median_{h,w} |flow[f, :, :, c]|
    of    = mean_{h,w,c} clip(|flow[f, :, :, c]|, P10_c, P90_c),   P_c = np.percentile(|flow[..., c]|, 10 / 90)

min-max normalises each series over the trial and appends its last value.  Here the order statistics are taken from
a full sort, the percentile's interpolation is numpy 2's for a float32 array and a scalar q written out (quantile,
virtual index, weight and _lerp all float32), and the two means and the normalisation are float64: the yardstick both
the reference's float32 result (the fixture's d_ref) and the kernels' are measured against.
"""
import numpy as np

# (trials, flow frames, H, W): an even and an odd pixel count and single pixels.  n = frames H W values per
# component and trial: 210 and 315 (n - 1 no multiple of 10: the percentiles interpolate), 11 (n - 1 = 10: they do not)
GEOMETRIES = {"A": (3, 7, 6, 5), "B": (3, 5, 7, 9), "C": (3, 11, 1, 1)}
SEEDS = {"A": 11, "B": 12, "C": 13}
N_NEURONS = 4
BATCHES = (2, 1)          # geometry A's trials as two loader batches


def make_inputs(name):
    """(video uint8 (K, F, H, W), flow float32 (K, F - 1, H, W, 2)): the flow is quantised to eighths so that ties
    straddle the median and the percentile ranks, both signs occur, and its scale grows along the trial so that no
    series is flat."""
    K, Fp, H, W = GEOMETRIES[name]
    rng = np.random.default_rng(SEEDS[name])
    video = rng.integers(0, 256, size=(K, Fp + 1, H, W)).astype(np.uint8)
    # frames differ in contrast, so the motion energy moves
    gain = rng.uniform(0.2, 1.0, size=(K, Fp + 1, 1, 1))
    video = (video * gain).astype(np.uint8)
    scale = rng.uniform(4.0, 40.0, size=(K, Fp, 1, 1, 2))
    flow = np.round(rng.standard_normal((K, Fp, H, W, 2)) * scale) / 8.0
    return video, flow.astype(np.float32)


def make_batches(name="A"):
    """Loader batches of geometry `name` as dicts of numpy arrays (the tests and the generator wrap them in torch
    tensors): what the reference's loader yields per key."""
    video, flow = make_inputs(name)
    K, Fp, H, W = GEOMETRIES[name]
    T = Fp + 1
    rng = np.random.default_rng(SEEDS[name] + 100)
    full = {
        "whisker-of-video": flow,
        "whisker-video": video[:, :, None],
        "wheel-speed": rng.standard_normal((K, T)).astype(np.float32),
        "whisker-motion-energy": rng.uniform(0, 1, (K, T)).astype(np.float32),
        "whisker-of": rng.uniform(0, 1, (K, T)).astype(np.float32),
        "choice": rng.choice([-1.0, 1.0], size=(K, 1)),
        "block": rng.choice([0.2, 0.5, 0.8], size=(K, 1)),
        "ap": rng.poisson(1.0, (K, T, N_NEURONS)).astype(np.float32),
        "timestamp": np.sort(rng.uniform(0, 100, (K, T)), axis=1),
    }
    out, at = [], 0
    for b in BATCHES:
        out.append({k: v[at:at + b] for k, v in full.items()})
        at += b
    assert at == K
    return out


RRR_BRANCHES = ("whisker-of-video", "all", "other", "of-all", "whisker-video", "wheel-speed", "whisker-of")


def median_f32(x):
    """np.median of a 1-D float32 array from a full sort: the middle element, or the float32 mean of the two."""
    s = np.sort(np.asarray(x, dtype=np.float32))
    n = len(s)
    if np.isnan(s[-1]):
        return np.float32(np.nan)
    if n % 2:
        return s[n // 2]
    return np.float32((s[n // 2 - 1] + s[n // 2]) / np.float32(2))


def percentile_ranks(n, q):
    """(previous index, next index, weight) of np.percentile(x, q) for a float32 x of n values and a Python scalar q:
    numpy 2 divides q by float32(100), so the quantile, the virtual index (n - 1) q, its floor and the weight are
    float32."""
    quant = np.float32(q) / np.float32(100)
    last = np.float32(n - 1)
    v = np.float32(last * quant)
    if v >= last:
        return n - 1, n - 1, np.float32(np.float64(v) + 1.0)
    p = np.floor(v)
    nxt = np.float32(p + np.float32(1))
    return int(p), min(int(nxt), n - 1), np.float32(np.float64(v) - np.float64(p))


def percentile_f32(x, q):
    s = np.sort(np.asarray(x, dtype=np.float32).reshape(-1))
    p, nxt, t = percentile_ranks(len(s), q)
    if np.isnan(s[-1]):
        return np.float32(np.nan)
    a, b = s[p], s[nxt]
    with np.errstate(invalid="ignore"):
        d = np.float32(b - a)
        r = np.float32(a + np.float32(d * t))
        if t >= np.float32(0.5):
            r = np.float32(b - np.float32(d * np.float32(np.float32(1) - t)))
    return r


def raw_series(video, flow):
    """One trial: the series before the normalisation.  me, of float64 (F - 1,), med float32 (F - 1, 2),
    bounds float32 (2, 2) = [component][P10, P90]."""
    v = np.asarray(video)
    d = np.abs(np.diff(v.astype(np.float32), axis=0))                     # float32 differences, as the reference's
    me = d.astype(np.float64).reshape(d.shape[0], -1).mean(axis=1)
    a = np.abs(np.asarray(flow, dtype=np.float32))
    Fp = a.shape[0]
    med = np.array([[median_f32(a[f, :, :, c].reshape(-1)) for c in range(2)] for f in range(Fp)], dtype=np.float32)
    bounds = np.array([[percentile_f32(a[..., c], 10), percentile_f32(a[..., c], 90)] for c in range(2)],
                      dtype=np.float32)
    clipped = np.stack([np.clip(a[..., c], bounds[c, 0], bounds[c, 1]) for c in range(2)], axis=-1)
    of = clipped.astype(np.float64).reshape(Fp, -1).mean(axis=1)
    return me, of, med, bounds


def minmax_append(x, dtype):
    """(x - min) / (max - min) over axis 0 in `dtype`, the last value appended."""
    x = np.asarray(x, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        y = (x - x.min(axis=0)) / (x.max(axis=0) - x.min(axis=0))
    return np.concatenate([y, y[-1:]], axis=0)


def flow_features(video, flow):
    """One trial's {'me', 'of': (F,) float64, 'of-2d': (F, 2) float32 with numpy's float32 roundings, 'bounds',
    'med'}."""
    me, of, med, bounds = raw_series(video, flow)
    return {"me": minmax_append(me, np.float64), "of": minmax_append(of, np.float64),
            "of-2d": minmax_append(med, np.float32), "bounds": bounds, "med": med}


def denominators(video, flow):
    """max - min over max of each raw series of a trial: the generator checks that none is near zero."""
    me, of, med, _ = raw_series(video, flow)
    return [float((s.max() - s.min()) / s.max()) for s in (me, of, med[:, 0].astype(np.float64),
                                                           med[:, 1].astype(np.float64))]


def rrr_data(batches, input_mod):
    """get_rrr_data's X with numpy on the host: the medians are np.median itself."""
    X = []
    for b in batches:
        def med(key="whisker-of-video"):
            return np.stack([np.median(b[key][..., c], axis=(2, 3)) for c in range(2)], axis=2)
        ws = b["wheel-speed"]
        T = ws.shape[1]
        tail = [ws[..., None], np.repeat(b["choice"], T, axis=1)[..., None], np.repeat(b["block"], T, axis=1)[..., None]]
        if input_mod == "whisker-of-video":
            X.append(med())
        elif input_mod == "all":
            X.append(np.concatenate([b["whisker-motion-energy"][..., None]] + tail, axis=2))
        elif input_mod == "other":
            X.append(np.concatenate(tail, axis=2))
        elif input_mod == "of-all":
            of = med()
            X.append(np.concatenate([np.concatenate([of, of[:, -1:]], axis=1)] + tail, axis=2))
        else:
            X.append(b[input_mod])
    return np.concatenate(X, axis=0)
