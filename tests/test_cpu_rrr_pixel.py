"""The RRR baseline on raw pixels without a GPU: tests/rrr_pixel_ref.py (the restatement the GPU tests compare
against) held to tests/golden/rrr_pixel.npz (the reference's own RRRGD / helpers, scripts/gen_rrr_pixel_fixture.py),
the library's size checks and workspace formula, and the host logic of vspike.rrr.PixelFeatures.

Bars: 100 x the spread the fixture records for the reference itself (its second run, whose fit saw the
standardised training trials in another order), as in tests/test_cpu_rrr_baseline.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import rrr_pixel_ref as rp
import rrr_ref as rr

FACTOR = 100.0


@pytest.fixture(scope="module")
def built_lib():
    from vspike import build
    build.build(verbose=False)
    return build.LIB_PATH


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("rrr_pixel.npz")


def test_fixture_is_what_the_issue_asks(fixture):
    assert (rp.C, rp.T, rp.F, rp.K_TRAIN, rp.K_VAL, rp.N) == (1100, 12, 16, 14, 5, 9) and rp.C > 1024 and rp.T >= 9
    raw = rp.make_raw()[rp.EID]
    assert all(x.dtype == np.uint8 and x.shape[1:] == (rp.F, 1, rp.H, rp.W) for x in raw["X"])
    flat = rp.flatten(rp.make_raw())[rp.EID]["X"]
    assert flat[0].shape == (rp.K_TRAIN, rp.F, rp.C) and np.shares_memory(flat[0], flat[0].reshape(-1))
    mean, std = rp.stats_u8(flat[0])
    assert mean.dtype == np.float64 and np.array_equal(mean, np.mean(flat[0], axis=0))
    assert np.array_equal(std, np.clip(np.std(flat[0], axis=0), 1e-8, None))
    assert (std[:, rp.CONSTANT_PIXEL] == 1e-8).all() and (std == 1e-8).sum() == rp.F
    assert (flat[0][:, :, rp.SATURATED_PIXEL] == 255).mean() > 0.5
    idx = rp.frame_idx()
    assert len(idx) == rp.T and idx.max() < rp.F - 1 and np.all(np.diff(idx) > 0) and list(idx) != list(range(rp.T))
    assert fixture["X/n_iter"] == 20 and fixture["X/func_evals"] == 20 and fixture["X/perm/n_iter"] == 20
    assert fixture["X/losses"].shape == (20,) and fixture["X/V"].shape == (3, rp.T)
    assert fixture["X/U"].shape == (rp.N, rp.C, 3) and fixture["X/b"].shape == (rp.N, 1, rp.T)
    nan = np.isnan(fixture["X/bps"])
    assert np.flatnonzero(nan).tolist() == [rp.SILENT] and np.isfinite(fixture["X/bps"][rp.SILENT_IN_TRAIN])
    sp = rr.spreads(fixture, rp.GEOM)
    assert all(0 < sp[k] < 1e-5 for k in ("losses", "U", "V", "bps", "r2", "co_bps")), sp


def test_restatement_matches_the_reference(fixture):
    out = rp.run()
    assert out["n_iter"] == fixture["X/n_iter"] and out["func_evals"] == fixture["X/func_evals"]
    d, s = rp.distances(out, fixture)
    for k, v in d.items():
        assert v <= FACTOR * s[k], (k, v, s[k])


def test_library_rejects_unsupported_sizes_without_launching(built_lib):
    from vspike import _lib
    lib = _lib.lib()
    assert lib.vs_version() >= 12
    one = ctypes.c_void_p(16)                      # never dereferenced: the size checks come first
    for C, r, word in ((32769, 3, "C <= 32768"), (0, 3, "C <= 32768"), (40, 5, "r <= 4"), (40, 0, "r <= 4")):
        rc = lib.vs_rrr_pixel_loss_grad(4, 6, 5, 6, C, r, one, _lib.VS_U8, one, one, one, one, _lib.VS_F32, one, one,
                                        one, 100.0, one, None, None, None, one, None)
        assert rc == -1 and word in lib.vs_last_error().decode(), (C, r, lib.vs_last_error())
        rc = lib.vs_rrr_pixel_score(4, 6, 5, 6, C, r, one, _lib.VS_U8, one, one, one, one, one, one, one, one, one,
                                    _lib.VS_F32, None, one, one, one, one, None)
        assert rc == -1 and word in lib.vs_last_error().decode(), (C, r, lib.vs_last_error())
    rc = lib.vs_rrr_pixel_stats(4, 6, 32769, one, _lib.VS_U8, one, one, None)
    assert rc == -1 and "C <= 32768" in lib.vs_last_error().decode()
    rc = lib.vs_rrr_pixel_loss_grad(4, 6, 5, 6, 40, 3, one, _lib.VS_U8, one, one, one, one, _lib.VS_BF16, one, one,
                                    one, 100.0, one, None, None, None, one, None)
    assert rc == -1 and "f32 or f64" in lib.vs_last_error().decode()
    rc = lib.vs_rrr_pixel_loss_grad(4, 6, 5, 6, 40, 3, one, _lib.VS_BF16, one, one, one, one, _lib.VS_F32, one, one,
                                    one, 100.0, one, None, None, None, one, None)
    assert rc == -1 and "u8 or f32" in lib.vs_last_error().decode()
    rc = lib.vs_rrr_pixel_loss_grad(4, 6, 5, 6, 40, 3, one, _lib.VS_U8, one, one, one, one, _lib.VS_F64, one, one,
                                    one, 100.0, one, one, None, None, one, None)
    assert rc == -1 and "together" in lib.vs_last_error().decode()
    # the workspace formula of the header comment: K T N + T ceil(N/256) + ceil(N (C + T) / 256) +
    # ceil((C+1)/64) ceil(N/64) r T doubles, each piece rounded up to 256 bytes
    q = lib.vs_rrr_pixel_loss_grad_workspace_bytes
    assert q(4, 5, 6, 32769, 3) == 0 and q(4, 5, 6, 40, 5) == 0 and q(4, 5, 6, 0, 3) == 0
    need = q(13, 20, 65, 1100, 3)
    exact = 8 * (13 * 20 * 65 + (20 * 1 + -(-65 * (1100 + 20) // 256)) + 18 * 2 * 3 * 20)
    assert exact <= need <= exact + 3 * 256 and need % 256 == 0
    # the session the loader and the PCA are measured on: under 1 GB where the wide layout needs 7.7 GB
    big = q(400, 100, 512, 18260, 3)
    wide_formula = 8 * (400 * 100 * 512 + 100 * (18260 + 2) * 512)
    assert 0.16e9 < big < 0.18e9 and big < 1e9 and 7.6e9 < wide_formula < 7.8e9
    assert lib.vs_rrr_pixel_score_workspace_bytes(5, 20, 65) == lib.vs_rrr_wide_score_workspace_bytes(5, 20, 65)
    # the pixel counters are a group of their own; the pinned groups have not moved
    assert _lib.RRR_PIXEL_PATH_NAMES == ("rrr_pixel", "rrr_pixel_stats")
    assert _lib.RRR_PATH_NAMES == ("rrr_wide", "gauss_smooth")
    _lib.dispatch_reset()
    assert _lib.rrr_pixel_dispatch_counts() == {"rrr_pixel": 0, "rrr_pixel_stats": 0}


def test_pixel_features_host_argument_errors():
    from vspike._lib import VsError
    from vspike.rrr import RRRGD, PixelFeatures, check_dims_pixel, pixel_rrr_data, prepare_rrr_inputs
    K, F, C = 3, 5, 7
    X = torch.zeros(K, F, C, dtype=torch.uint8)
    mean, std = torch.zeros(F, C, dtype=torch.float64), torch.ones(F, C, dtype=torch.float64)
    p = PixelFeatures(X, [0, 2, 4], mean, std)
    assert p.shape == (K, 3, C + 1) and p.X.data_ptr() == X.data_ptr() and p.idx.dtype == torch.int64
    five = PixelFeatures(torch.zeros(K, F, 1, 1, C, dtype=torch.uint8), np.array([1, 3]), mean, std)
    assert five.shape == (K, 2, C + 1)
    with pytest.raises(VsError, match="uint8 / float32"):
        PixelFeatures(X.double(), [0, 2], mean, std)
    with pytest.raises(VsError, match="uint8 / float32"):
        PixelFeatures(X.numpy(), [0, 2], mean, std)
    for bad in ([0, F], [-1, 2], [0.5, 1.0], []):
        with pytest.raises(VsError, match="idx"):
            PixelFeatures(X, bad, mean, std)
    with pytest.raises(VsError, match="mean / std"):
        PixelFeatures(X, [0, 2], mean[:, :-1], std)
    with pytest.raises(VsError, match="mean / std"):
        PixelFeatures(X, [0, 2], mean, std.t())
    with pytest.raises(VsError, match="mean / std"):
        PixelFeatures(X, [0, 2], mean.float(), std.float())                     # uint8 frames take float64 statistics
    with pytest.raises(VsError, match="mean / std"):
        PixelFeatures(X.float(), [0, 2], mean, std)                             # float32 frames float32 ones
    with pytest.raises(VsError, match="dense"):
        PixelFeatures(torch.zeros(K, F, 2 * C, dtype=torch.uint8)[:, :, ::2], [0, 2], mean, std)
    # the float64 tensor it stands for
    Xr = torch.arange(K * F * C, dtype=torch.uint8).view(K, F, C)
    m = PixelFeatures(Xr, [4, 1], mean + 2, std * 4).materialise()
    assert m.shape == (K, 2, C + 1) and m.dtype == torch.float64 and bool((m[:, :, C] == 1).all())
    assert torch.equal(m[:, 0, :C], (Xr[:, 4].double() - 2) / 4)
    # RRRGD: the sizes and the pairing with y are checked before anything reaches the device
    check_dims_pixel(32768, 4)
    y = torch.zeros(K, 3, 4)
    with pytest.raises(VsError, match="5 components"):
        RRRGD(n_comp=5).fit({"a": (p, y)})
    with pytest.raises(VsError, match="y \\[K, T, N\\]"):
        RRRGD().fit({"a": (p, torch.zeros(K, 2, 4))})
    with pytest.raises(VsError, match="float32 or float64"):
        RRRGD().fit({"a": (p, y.to(torch.bfloat16))})
    with pytest.raises(VsError, match="32769 pixels"):
        check_dims_pixel(32769, 3)
    # tensor sessions keep their cap, and the message now points at PixelFeatures
    with pytest.raises(VsError, match="1025 features.*PixelFeatures"):
        RRRGD().fit({"a": (torch.zeros(2, 3, 1026, dtype=torch.float64), torch.zeros(2, 3, 4))})
    # prepare_rrr_inputs: wide float64 frames are refused (uint8 / float32 only), before the device is touched
    d = pixel_rrr_data(np.zeros((2, 12, 1, 25, 44)), np.zeros((2, 10, 3), np.float32),
                       np.zeros((2, 12, 1, 25, 44)), np.zeros((2, 10, 3), np.float32))
    assert list(d) == ["session"] and d["session"]["X"][0].shape == (2, 12, 1, 25, 44)
    with pytest.raises(VsError, match="uint8 or float32 frames"):
        prepare_rrr_inputs(d, "whisker-video", idx=np.arange(10), device="cpu")
    with pytest.raises(VsError, match="pixel_rrr_data"):
        pixel_rrr_data(np.zeros((2, 12, 9)), np.zeros((3, 10, 3)), np.zeros((2, 12, 9)), np.zeros((2, 10, 3)))
