"""The behaviour features on the GPU: vs_flow_median2, vs_flow_quantiles, vs_flow_clip_mean, vs_motion_energy
(csrc/flow_features.hip) and vspike.behaviour's flow_features, get_rrr_data and behaviour_rrr_data.

Bars.  Order statistics are exact, so medians and percentiles are compared bit for bit with np.median /
np.percentile computed here (a zero of either sign equals a zero; NaN equals NaN).  'me' and 'of' are float64 sums
rounded once and then normalised with the reference's float32 roundings: they must lie within 1 x d_ref of the
float64 restatement (tests/flow_features_ref.py), d_ref being the reference's own float32 distance to it recorded in
tests/golden/flow_features.npz.  The end-to-end fit on kernel-made inputs equals the fit on numpy-made inputs bit for
bit, because the inputs are equal bit for bit.
"""
import warnings

import numpy as np
import pytest
import torch

import flow_features_ref as fr
import rrr_baseline_ref as rb

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("flow_features.npz")


@pytest.fixture(scope="module")
def plan():
    from vspike import ops
    return ops.flow_plan()


def _same(got, want):
    """Equal bits, or zeros of either sign, or NaN in both."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    ok = (got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0)) | (np.isnan(got) & np.isnan(want))
    return bool(ok.all())


def _median_inputs(hw, seed):
    """{kind: (2 trials, 2 frames, hw, 2) float32}: the cases of the issue."""
    rng = np.random.default_rng(seed)
    shape = (2, 2, hw, 2)
    out = {"ties": (np.round(rng.standard_normal(shape) * 6) / 4).astype(np.float32),            # both signs, many ties
           "continuous": rng.standard_normal(shape).astype(np.float32),
           "equal": np.full(shape, -1.75, dtype=np.float32)}
    mid = rng.standard_normal(shape).astype(np.float32)                                           # all ties at the middle:
    order = np.argsort(mid, axis=2)                                                              # the middle third of each
    ranks = np.argsort(order, axis=2)                                                            # frame is one value
    out["middle"] = np.where((ranks >= hw // 3) & (ranks <= hw - 1 - hw // 3), np.float32(0.125), mid)
    low = (np.float32(1.5).view(np.uint32) + rng.integers(0, 256, size=shape).astype(np.uint32)).view(np.float32)
    out["low_byte"] = np.where(rng.random(shape) < 0.5, low, -low).astype(np.float32)            # keys differ in one byte
    den = rng.integers(-200, 200, size=shape).astype(np.float32) * np.float32(1e-45)             # denormals and zeros
    out["denormal"] = den
    inf = rng.standard_normal(shape).astype(np.float32)
    inf[rng.random(shape) < 0.3] = np.inf
    inf[rng.random(shape) < 0.3] = -np.inf
    out["inf"] = inf
    nan = rng.standard_normal(shape).astype(np.float32)
    nan[0, 1, hw // 2, 0] = np.nan                                                               # one NaN: that frame's
    out["nan"] = nan                                                                             # component only
    return out


def _np_median(x, absolute):
    a = np.abs(x) if absolute else x
    return np.stack([np.median(a[..., c], axis=2) for c in range(2)], axis=2)


@pytest.mark.parametrize("hw", [1, 2, 63, 64, 65, 255, 256, 257, "at_lds", "past_lds"])
def test_medians_are_numpys_bits(hw, plan):
    """at_lds: the largest frame whose keys are staged (158 KiB of LDS in one workgroup); past_lds: one pixel more,
    the kernel that re-reads the frame."""
    from vspike import ops
    past = hw == "past_lds"
    hw = plan["stage_max"] + past if isinstance(hw, str) else hw
    assert (hw > plan["stage_max"]) == past
    for kind, x in _median_inputs(hw, 100 + hw).items():
        assert x.dtype == np.float32
        if kind == "denormal":
            assert (np.abs(x[x != 0]) < 1.2e-38).all() and (x != 0).any()
        flow = torch.from_numpy(x.reshape(2, 2, 1, hw, 2)).to(DEV)
        for absolute in (False, True):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                  # numpy warns about inf - inf and NaN
                want = _np_median(x, absolute)
            got = ops.flow_median2(flow, absolute=absolute).cpu().numpy()
            assert want.dtype == np.float32 and _same(got, want), (kind, absolute, hw, got.ravel()[:8], want.ravel()[:8])
            if kind == "nan":
                assert np.isnan(got[0, 1, 0]) and not np.isnan(got[0, 1, 1]) and np.isnan(got).sum() == 1
        again = ops.flow_median2(flow, absolute=True)
        assert torch.equal(again.view(torch.int32), ops.flow_median2(flow, absolute=True).view(torch.int32))


def test_median_trial_strides_and_frame_shapes():
    """(H, W) only enters as H W, and trial k's frames follow trial k - 1's."""
    from vspike import ops
    rng = np.random.default_rng(3)
    x = (np.round(rng.standard_normal((2, 3, 7, 9, 2)) * 5) / 2).astype(np.float32)
    got = ops.flow_median2(torch.from_numpy(x).to(DEV)).cpu().numpy()
    want = np.stack([np.median(x[..., c], axis=(2, 3)) for c in range(2)], axis=2)
    assert _same(got, want)
    with pytest.raises(Exception, match="dense float32"):
        ops.flow_median2(torch.from_numpy(x).to(DEV)[:, :, ::2])


def _quantile_cases(plan):
    chunk = plan["quantile_chunk"]
    return [(1, 1), (1, 2), (1, 11), (1, chunk - 1), (1, chunk), (1, chunk + 1), (3, chunk + 7)]


@pytest.mark.parametrize("case", range(7))
def test_quantiles_are_numpys_bits(case, plan):
    from vspike import ops
    Fp, hw = _quantile_cases(plan)[case]
    n = Fp * hw
    rng = np.random.default_rng(200 + case)
    for kind in ("ties", "continuous"):
        x = rng.standard_normal((2, Fp, 1, hw, 2)).astype(np.float32) * np.float32(3)
        if kind == "ties":
            x = (np.round(x * 2) / 4).astype(np.float32)
        x[1] *= np.float32(0.01)                                 # the trials' ranges differ
        flow = torch.from_numpy(x).to(DEV)
        ws = torch.full((int(ops.lib().vs_flow_quantiles_workspace_bytes(2)),), 0xA5, dtype=torch.uint8, device=DEV)
        bounds, stats = ops.flow_quantiles(flow, (10, 90), with_stats=True, workspace=ws)
        a = np.abs(x)
        want = np.array([[[np.percentile(a[k, ..., c], 10), np.percentile(a[k, ..., c], 90)] for c in range(2)]
                         for k in range(2)])
        assert want.dtype == np.float32 and _same(bounds.cpu().numpy(), want), (kind, n, bounds, want)
        s = np.sort(a.reshape(2, n, 2), axis=1)
        ranks = [r for q in (10, 90) for r in fr.percentile_ranks(n, q)[:2]]
        assert _same(stats.cpu().numpy(), np.stack([s[:, r, :] for r in ranks], axis=2))
        again = ops.flow_quantiles(flow, (10, 90))               # a fresh workspace: the same bits
        assert torch.equal(again.view(torch.int32), bounds.view(torch.int32))
        for q in ((0, 100), (50, 25)):                           # the ends and ranks that do not come in pairs
            got = ops.flow_quantiles(flow, q).cpu().numpy()
            want = np.array([[[np.percentile(a[k, ..., c], q[0]), np.percentile(a[k, ..., c], q[1])]
                              for c in range(2)] for k in range(2)])
            assert _same(got, want), (kind, n, q)
    x[1, 0, 0, hw // 2, 1] = np.nan                              # a NaN: that trial's component only
    got = ops.flow_quantiles(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert np.isnan(got[1, 1]).all() and np.isnan(got).sum() == 2


@pytest.fixture(scope="module")
def features(fixture):
    """Per geometry: what flow_features gives for the fixture's inputs (uint8 video), and the restatement."""
    from vspike import behaviour
    out = {}
    for g, (K, Fp, H, W) in fr.GEOMETRIES.items():
        video = torch.from_numpy(fixture[f"{g}/video"]).to(DEV)
        flow = torch.from_numpy(fixture[f"{g}/flow"]).to(DEV)
        got = behaviour.flow_features(video, flow)
        want = [fr.flow_features(fixture[f"{g}/video"][k], fixture[f"{g}/flow"][k]) for k in range(K)]
        out[g] = (video, flow, got, want)
    return out


@pytest.mark.parametrize("g", list(fr.GEOMETRIES))
def test_flow_features_order_statistics_equal_the_fixture(g, fixture, features):
    from vspike import ops
    video, flow, got, _ = features[g]
    K, Fp, H, W = fr.GEOMETRIES[g]
    assert got["of-video"] is flow and got["me"].shape == (K, Fp + 1) and got["of-2d"].shape == (K, Fp + 1, 2)
    assert _same(ops.flow_median2(flow, absolute=True).cpu().numpy(), fixture[f"{g}/med"])
    assert _same(ops.flow_quantiles(flow).cpu().numpy(), fixture[f"{g}/bounds"])
    assert _same(got["of-2d"].cpu().numpy(), fixture[f"{g}/of-2d"])


@pytest.mark.parametrize("g", list(fr.GEOMETRIES))
def test_flow_features_means_within_the_references_error(g, fixture, features):
    """me / of within 1 x d_ref of the float64 restatement.  Measured on an MI355X: see MEASURED below."""
    _, _, got, want = features[g]
    for name in ("me", "of"):
        d_ref = float(fixture[f"{g}/d_ref_{name}"])
        x = got[name].cpu().numpy()
        assert x.dtype == np.float32 and np.isfinite(x).all()
        d = max(float(np.abs(x[k].astype(np.float64) - want[k][name]).max()) for k in range(len(want)))
        print(f"flow_features {g} {name}: distance {d:.3e}, d_ref {d_ref:.3e}, ratio {d / d_ref:.3f}")
        assert d <= d_ref, (g, name, d, d_ref)
        assert np.array_equal(x[:, -1], x[:, -2])                # the last value is appended once


@pytest.mark.parametrize("g", list(fr.GEOMETRIES))
def test_flow_features_video_dtype_and_repeatability(g, features):
    from vspike import behaviour
    video, flow, got, _ = features[g]
    ptr = video.data_ptr()
    as_f32 = behaviour.flow_features(video.float(), flow)
    again = behaviour.flow_features(video, flow)
    assert video.dtype == torch.uint8 and video.data_ptr() == ptr
    for name in ("me", "of", "of-2d"):
        assert torch.equal(as_f32[name].view(torch.int32), got[name].view(torch.int32)), name
        assert torch.equal(again[name].view(torch.int32), got[name].view(torch.int32)), name


def test_motion_energy_paths_agree():
    """Byte loads (H W odd, or an odd address) and dword loads give the same exact sums; float32 frames with
    fractions match the float64 mean of the float32 differences."""
    from vspike import ops
    rng = np.random.default_rng(9)
    for hw in (1, 3, 64, 1028, 1031):
        v = rng.integers(0, 256, size=(2, 4, 1, hw)).astype(np.uint8)
        want = np.abs(np.diff(v.astype(np.float64), axis=1)).mean(axis=(2, 3)).astype(np.float32)
        buf = torch.zeros(v.size + 1, dtype=torch.uint8, device=DEV)
        for off in (0, 1):
            t = buf[off:off + v.size].view(v.shape)
            t.copy_(torch.from_numpy(v))
            assert _same(ops.motion_energy(t).cpu().numpy(), want), (hw, off)
        f = (rng.standard_normal((2, 4, 1, hw)) * 10).astype(np.float32)
        want = np.abs(np.diff(f, axis=1)).astype(np.float64).mean(axis=(2, 3)).astype(np.float32)
        assert _same(ops.motion_energy(torch.from_numpy(f).to(DEV)).cpu().numpy(), want), hw


def test_clip_mean_matches_float64_and_propagates_nan():
    from vspike import ops
    rng = np.random.default_rng(10)
    x = rng.standard_normal((2, 3, 5, 53, 2)).astype(np.float32)
    b = np.array([[[0.2, 1.1], [0.3, 0.9]], [[0.0, 0.5], [0.7, 0.7]]], dtype=np.float32)
    a = np.abs(x)
    clipped = np.stack([np.clip(a[..., c], b[:, c, 0, None, None, None], b[:, c, 1, None, None, None])
                        for c in range(2)], axis=-1)
    want = clipped.astype(np.float64).mean(axis=(2, 3, 4)).astype(np.float32)
    got = ops.flow_clip_mean(torch.from_numpy(x).to(DEV), torch.from_numpy(b).to(DEV)).cpu().numpy()
    assert _same(got, want)
    b[1, 0, 0] = np.nan
    got = ops.flow_clip_mean(torch.from_numpy(x).to(DEV), torch.from_numpy(b).to(DEV)).cpu().numpy()
    assert np.isnan(got[1]).all() and _same(got[0], want[0])


def test_constant_series_is_nan_as_in_the_reference():
    """A still video: max - min = 0, so 'me' is 0 / 0 = NaN for that trial only."""
    from vspike import behaviour
    video = torch.from_numpy(fr.make_inputs("A")[0]).to(DEV).clone()
    flow = torch.from_numpy(fr.make_inputs("A")[1]).to(DEV)
    video[1] = 7
    got = behaviour.flow_features(video, flow)
    assert torch.isnan(got["me"][1]).all() and torch.isfinite(got["me"][[0, 2]]).all()
    assert torch.isfinite(got["of"]).all() and torch.isfinite(got["of-2d"]).all()


def _tensors(batches, device="cpu"):
    return [{k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in b.items()} for b in batches]


@pytest.mark.parametrize("mod", fr.RRR_BRANCHES)
def test_get_rrr_data_equals_the_fixture(mod, fixture):
    from vspike import behaviour
    batches = fr.make_batches("A")
    for device in ("cpu", DEV):                                  # host batches (a loader's) and device batches
        X, y, stamps = behaviour.get_rrr_data(_tensors(batches, device), mod)
        assert X.is_cuda and y.is_cuda and stamps.is_cuda
        want = fixture[f"rrr/{mod}/X"]
        got = X.cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, (mod, got.dtype, want.dtype)
        assert _same(got, want) if want.dtype == np.float32 else np.array_equal(got, want), mod
        assert np.array_equal(y.cpu().numpy(), fixture["rrr/y"])
        assert np.array_equal(stamps.cpu().numpy(), fixture["rrr/timestamp"])


def _session():
    """rrr_baseline.npz's narrow session (M0: 9 + 4 trials, 20 bins, 65 neurons) with behaviour inputs: 23 flow frames
    of 6 x 5, 24 frames of wheel speed, choice and block as in that fixture's preparation geometry."""
    raw = rb.make_raw("M")["M0"]
    g = rb.GEOMETRIES["M"]["sessions"]["M0"]
    kt, kv, T = g["k_train"], g["k_val"], rb.T
    assert (kt, kv, T, g["N"]) == (9, 4, 20, 65)
    Fp = 23
    rng = np.random.default_rng(77)
    idx = np.sort(np.random.RandomState(5).choice(Fp, T, replace=False))
    splits = []
    for K, y in ((kt, raw["y"][0]), (kv, raw["y"][1])):
        within = np.arange(K)
        scale = rng.uniform(2.0, 30.0, size=(K, Fp, 1, 1, 2))
        b = {"whisker-of-video": (np.round(rng.standard_normal((K, Fp, 6, 5, 2)) * scale) / 8).astype(np.float32),
             "wheel-speed": rng.standard_normal((K, Fp + 1)).astype(np.float32),
             "choice": np.array(rb.CHOICES)[within % 2][:, None], "block": np.array(rb.BLOCKS)[within % 3][:, None],
             "ap": np.ascontiguousarray(y), "timestamp": np.sort(rng.uniform(0, 9, (K, Fp + 1)), axis=1)}
        cut = K // 2
        splits.append([{k: v[:cut] for k, v in b.items()}, {k: v[cut:] for k, v in b.items()}])
    return splits, idx


@pytest.mark.parametrize("mod", ["of-2d", "of-all"])
def test_end_to_end_fit_equals_the_fit_on_host_made_inputs(mod):
    from vspike import behaviour
    from vspike.rrr import train_rrr_baseline
    (train, test), idx = _session()
    data = behaviour.behaviour_rrr_data(_tensors(train), _tensors(test), mod, eid="M0")
    key = behaviour.LOADER_KEY.get(mod, mod)
    host = {"M0": {"X": [fr.rrr_data(train, key), fr.rrr_data(test, key)],
                   "y": [np.concatenate([b["ap"] for b in s]) for s in (train, test)], "setup": {}}}
    for i in range(2):
        got = data["M0"]["X"][i].cpu().numpy()
        assert got.dtype == host["M0"]["X"][i].dtype and np.array_equal(got, host["M0"]["X"][i])
    res, bps = train_rrr_baseline(data, mod, idx=idx)
    res_h, bps_h = train_rrr_baseline(host, mod, idx=idx)
    assert np.isfinite(bps) and bps == bps_h
    for k in ("pred", "gt"):
        assert np.array_equal(res["M0"][k], res_h["M0"][k], equal_nan=True), k
    for k in ("co_bps", "r2"):
        assert np.array_equal(np.array(res["M0"][k]), np.array(res_h["M0"][k]), equal_nan=True), k
