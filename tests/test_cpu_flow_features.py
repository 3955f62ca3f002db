"""The behaviour features without a GPU: tests/flow_features_ref.py (the restatement the GPU tests compare against)
held to tests/golden/flow_features.npz (the reference's own get_optic_flow / get_rrr_data,
scripts/gen_flow_features_fixture.py), the library's new symbols and size checks, and the argument checks of
vspike.behaviour's three functions.

Bars: the order statistics (medians, percentiles, the normalised medians) are numpy's bit for bit; 'me' and 'of' lie
at the distance d_ref the fixture records for the reference's float32 series from this float64 restatement.
"""
import ctypes

import numpy as np
import pytest
import torch

import flow_features_ref as fr


@pytest.fixture(scope="module")
def built_lib():
    from vspike import build
    build.build(verbose=False)
    return build.LIB_PATH


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("flow_features.npz")


def test_fixture_is_what_the_issue_asks(fixture):
    assert {g: v[1:] for g, v in fr.GEOMETRIES.items()} == {"A": (7, 6, 5), "B": (5, 7, 9), "C": (11, 1, 1)}
    for g, (K, Fp, H, W) in fr.GEOMETRIES.items():
        video, flow = fr.make_inputs(g)
        assert np.array_equal(video, fixture[f"{g}/video"]) and np.array_equal(flow, fixture[f"{g}/flow"])
        assert video.dtype == np.uint8 and flow.dtype == np.float32 and flow.shape == (K, Fp, H, W, 2)
        assert (flow > 0).any() and (flow < 0).any() and np.array_equal(flow * 8, np.round(flow * 8))
        assert fixture[f"{g}/me"].shape == (K, Fp + 1) and fixture[f"{g}/of-2d"].shape == (K, Fp + 1, 2)
        for k in range(K):                                  # every min-max denominator is far from zero
            assert min(fr.denominators(video[k], flow[k])) > 0.05
        assert 0 < fixture[f"{g}/d_ref_me"] < 1e-6 and 0 < fixture[f"{g}/d_ref_of"] < 1e-6
    # an even and an odd pixel count; the percentiles interpolate at n = 210, 315 and do not at n = 11
    assert (6 * 5) % 2 == 0 and (7 * 9) % 2 == 1
    assert fr.percentile_ranks(11, 10) == (1, 2, 0) and fr.percentile_ranks(11, 90) == (9, 10, 0)
    assert all(fr.percentile_ranks(n, q)[2] != 0 for n in (210, 315) for q in (10, 90))
    # ties straddle the median: some frame's two middle elements are equal, and some frame's are not
    a = np.sort(np.abs(fixture["A/flow"]).reshape(3, 7, 30, 2), axis=2)
    same = a[:, :, 14] == a[:, :, 15]
    assert same.any() and not same.all()


def test_restatement_matches_the_reference(fixture):
    for g, (K, Fp, H, W) in fr.GEOMETRIES.items():
        video, flow = fixture[f"{g}/video"], fixture[f"{g}/flow"]
        d_me = d_of = 0.0
        for k in range(K):
            got = fr.flow_features(video[k], flow[k])
            assert np.array_equal(got["med"], fixture[f"{g}/med"][k])
            assert np.array_equal(got["bounds"], fixture[f"{g}/bounds"][k])
            assert got["of-2d"].dtype == np.float32 and np.array_equal(got["of-2d"], fixture[f"{g}/of-2d"][k])
            d_me = max(d_me, np.abs(got["me"] - fixture[f"{g}/me"][k]).max())
            d_of = max(d_of, np.abs(got["of"] - fixture[f"{g}/of"][k]).max())
            # a float32 video gives the same series
            again = fr.flow_features(video[k].astype(np.float32), flow[k])
            assert np.array_equal(again["me"], got["me"])
        # d_ref is ~1e-7; the float64 sums behind it may differ in their last bit (1e-16) between numpy builds
        assert abs(d_me - fixture[f"{g}/d_ref_me"]) < 1e-12 and abs(d_of - fixture[f"{g}/d_ref_of"]) < 1e-12


def test_restated_order_statistics_are_numpys():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 10, 11, 64, 101, 1000, 32769):
        x = (np.round(rng.standard_normal(n) * 6) / 4).astype(np.float32)
        assert fr.median_f32(x).tobytes() == np.median(x).tobytes()
        for q in (10, 90, 0, 100, 50):
            assert fr.percentile_f32(np.abs(x), q).tobytes() == np.percentile(np.abs(x), q).tobytes(), (n, q)
    x = np.array([1.0, np.nan, 3.0], dtype=np.float32)
    assert np.isnan(fr.median_f32(x)) and np.isnan(fr.percentile_f32(x, 10))


def test_rrr_data_restatement_matches_the_reference(fixture):
    batches = fr.make_batches("A")
    for i, b in enumerate(batches):
        for k, v in b.items():
            assert np.array_equal(v, fixture[f"rrr/batch{i}/{k}"])
    for mod in fr.RRR_BRANCHES:
        X = fr.rrr_data(batches, mod)
        assert X.dtype == fixture[f"rrr/{mod}/X"].dtype and np.array_equal(X, fixture[f"rrr/{mod}/X"]), mod
    # of-all repeats the last flow frame's medians and the per-trial choice / block
    X = fixture["rrr/of-all/X"]
    assert np.array_equal(X[:, -1, :2], X[:, -2, :2]) and (X[:, :, 3:] == X[:, :1, 3:]).all()
    assert np.array_equal(X[:, :-1, :2], fixture["rrr/whisker-of-video/X"])
    # the medians are of the signed components
    assert (fixture["rrr/whisker-of-video/X"] < 0).any()


def test_library_has_the_flow_entries(built_lib):
    from vspike import _lib, ops
    lib = _lib.lib()
    assert lib.vs_version() >= 13
    for name in ("vs_flow_median2", "vs_flow_quantiles", "vs_flow_quantiles_workspace_bytes", "vs_flow_clip_mean",
                 "vs_motion_energy", "vs_flow_plan"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    plan = ops.flow_plan()
    # both components' keys and the histograms fit the CU's 160 KiB at the staging limit, and the workload's
    # 110 x 166 frame is staged
    assert (528 + 2 * plan["stage_max"]) * 4 <= 160 * 1024 and plan["stage_max"] >= 110 * 166
    assert plan["quantile_chunk"] % 256 == 0
    one = ctypes.c_void_p(64)                     # never dereferenced: the size checks come first
    for HW in (0, (1 << 20) + 1):
        assert lib.vs_flow_median2(3, HW, one, 0, one, None) == -1 and "H W <= 2^20" in lib.vs_last_error().decode()
        assert lib.vs_flow_quantiles(3, 2, HW, one, 10.0, 90.0, one, None, one, None) == -1
        assert "H W <= 2^20" in lib.vs_last_error().decode()
        assert lib.vs_flow_clip_mean(3, 2, HW, one, one, one, None) == -1
        assert lib.vs_motion_energy(_lib.VS_U8, 3, 4, HW, one, one, None) == -1
        assert "H W <= 2^20" in lib.vs_last_error().decode()
    assert lib.vs_flow_median2(3, 30, one, 2, one, None) == -1 and "absolute" in lib.vs_last_error().decode()
    assert lib.vs_flow_median2(3, 30, ctypes.c_void_p(4), 0, one, None) == -1 and "aligned" in lib.vs_last_error().decode()
    assert lib.vs_flow_median2(3, 30, None, 0, one, None) == -1 and "null" in lib.vs_last_error().decode()
    assert lib.vs_flow_quantiles(3, 1 << 12, 1 << 20, one, 10.0, 90.0, one, None, one, None) == -1
    assert "2^31" in lib.vs_last_error().decode()
    assert lib.vs_flow_quantiles(3, 2, 30, one, 10.0, 101.0, one, None, one, None) == -1
    assert "[0, 100]" in lib.vs_last_error().decode()
    assert lib.vs_flow_quantiles(65536, 2, 30, one, 10.0, 90.0, one, None, one, None) == -1
    assert lib.vs_motion_energy(_lib.VS_BF16, 3, 4, 30, one, one, None) == -1 and "VS_U8" in lib.vs_last_error().decode()
    assert lib.vs_motion_energy(_lib.VS_U8, 3, 1, 30, one, one, None) == -1 and "F >= 2" in lib.vs_last_error().decode()
    q = lib.vs_flow_quantiles_workspace_bytes
    assert q(0) == 0 and q(65536) == 0 and q(400) == 256 * -(-400 * 2 * 64 // 256) + 400 * 2 * 4096
    # nothing to do is not an error and touches nothing
    assert lib.vs_flow_median2(0, 30, None, 0, None, None) == 0
    assert lib.vs_flow_quantiles(0, 2, 30, None, 10.0, 90.0, None, None, None, None) == 0


def test_python_functions_check_their_arguments():
    from vspike import behaviour
    from vspike._lib import VsError
    video = torch.zeros(2, 4, 3, 5, dtype=torch.uint8)
    flow = torch.zeros(2, 3, 3, 5, 2)
    for v, f, word in ((video[0], flow, "video (K, F, H, W)"), (video.double(), flow, "uint8 or float32"),
                       (video, flow[..., 0], "flow (K, F - 1, H, W, 2)"), (video, flow.double(), "float32"),
                       (video, flow[:, :2], "needs a flow field"), (video[:, :1], flow[:, :0], "needs a flow field"),
                       (video, flow.transpose(2, 3).contiguous().transpose(2, 3), "dense"),
                       (video.numpy(), flow, "tensors")):
        with pytest.raises(VsError, match=word.replace("(", r"\(").replace(")", r"\)")):
            behaviour.flow_features(v, f)
    with pytest.raises(VsError, match="GPU only"):           # no fallback: host tensors are refused
        behaviour.flow_features(video, flow)

    batches = [{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in b.items()} for b in fr.make_batches("A")]
    drop = lambda key: [{k: v for k, v in b.items() if k != key} for b in batches]      # noqa: E731
    with pytest.raises(VsError, match="timestamp is not in batch 0"):
        behaviour.get_rrr_data(drop("timestamp"), "wheel-speed")
    with pytest.raises(VsError, match="no tensor 'block'"):
        behaviour.get_rrr_data(drop("block"), "other")
    with pytest.raises(VsError, match="no tensor 'whisker-of-video'"):
        behaviour.get_rrr_data(drop("whisker-of-video"), "of-all")
    with pytest.raises(VsError, match="no tensor 'ap'"):
        behaviour.get_rrr_data(drop("ap"), "wheel-speed")
    with pytest.raises(VsError, match="no tensor 'nothing'"):
        behaviour.get_rrr_data(batches, "nothing")
    with pytest.raises(VsError, match="no batches"):
        behaviour.get_rrr_data([], "other")
    with pytest.raises(VsError, match="not a dict"):
        behaviour.get_rrr_data([batches[0]["ap"]], "other")
    bad = [dict(batches[0], choice=batches[0]["choice"][:, 0])]
    with pytest.raises(VsError, match=r"'choice' is one value per trial"):
        behaviour.get_rrr_data(bad, "all")
    bad = [dict(batches[0], **{"whisker-of-video": batches[0]["whisker-of-video"][:, :-1]})]
    with pytest.raises(VsError, match="T - 1 = 7 frames"):
        behaviour.get_rrr_data(bad, "of-all")
    bad = [dict(batches[0], **{"whisker-of-video": batches[0]["whisker-of-video"].double()})]
    with pytest.raises(VsError, match="float32 flow field"):
        behaviour.get_rrr_data(bad, "whisker-of-video")

    with pytest.raises(VsError, match="none of"):
        behaviour.behaviour_rrr_data(batches, batches, "whisker-of-video")            # a loader key, not a mode
    with pytest.raises(VsError, match="timestamp"):
        behaviour.behaviour_rrr_data(drop("timestamp"), batches, "ws")
    assert behaviour.LOADER_KEY == {"me": "whisker-motion-energy", "of": "whisker-of", "of-2d": "whisker-of-video",
                                    "of-2d-v": "whisker-of-video", "ws": "wheel-speed"}
    import vspike
    assert vspike.flow_features is behaviour.flow_features and vspike.get_rrr_data is behaviour.get_rrr_data
    assert vspike.behaviour_rrr_data is behaviour.behaviour_rrr_data
    from vspike import rrr
    assert rrr.INPUT_MODS[:8] == ("me", "of", "of-2d", "of-2d-v", "all", "other", "me-all", "of-all")
