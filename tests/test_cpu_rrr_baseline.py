"""The RRR baseline without a GPU: tests/rrr_baseline_ref.py (the restatement the GPU tests compare against) held
to tests/golden/rrr_baseline.npz (the reference's own RRRGD / helpers, scripts/gen_rrr_baseline_fixture.py), the
scipy-order smoothing held to scipy's outputs, and the host logic of vspike.rrr's RRRGD / prepare_rrr_inputs and
of the ops wrappers.

Bars: 100 x the spread the fixture records for the reference itself (its second run, whose fit saw the
standardised training trials of every session in another order), as in tests/test_cpu_rrr.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import rrr_baseline_ref as rb
import rrr_ref as rr

FACTOR = 100.0


@pytest.fixture(scope="module")
def built_lib():
    from vspike import build
    build.build(verbose=False)
    return build.LIB_PATH


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("rrr_baseline.npz")


def test_fixture_is_what_the_issue_asks(fixture):
    assert rb.GEOMETRIES["W"]["sessions"] == {"W": dict(k_train=13, k_val=5, N=65, C=40)}
    assert [tuple(s.values()) for s in rb.GEOMETRIES["M"]["sessions"].values()] == \
        [(9, 4, 65, 5), (14, 5, 9, 40), (6, 3, 70, 1)]
    assert rb.GEOMETRIES["P"]["F"] == 24 and rb.GEOMETRIES["P"]["input_mod"] == "all" and rb.T == 20
    for geom, g in rb.GEOMETRIES.items():
        assert fixture[f"{geom}/n_iter"] == 20 and fixture[f"{geom}/func_evals"] == 20
        assert fixture[f"{geom}/losses"].shape == (20,) and fixture[f"{geom}/V"].shape == (3, 20)
        for eid, s in g["sessions"].items():
            nan = np.isnan(fixture[f"{geom}/{eid}/bps"])
            assert nan[rb.SILENT] and nan.sum() <= 3 and np.isfinite(fixture[f"{geom}/{eid}/bps"][rb.SILENT_IN_TRAIN])
            assert fixture[f"{geom}/{eid}/b"].shape == (s["N"], 1, 20)
        sp = rb.spreads(fixture, geom, keys=("losses", "U", "V", "bps", "r2", "co_bps"))
        assert all(0 < v < 1e-5 for v in sp.values()), sp
    assert "W/W/pred" in fixture and "M/M0/pred" not in fixture
    # P: every category in both splits, the frames a sorted draw of 20 from 23
    raw = rb.make_raw("P")["P"]
    for x in raw["X"]:
        assert set(np.unique(x[:, :, -2])) == set(rb.CHOICES) and set(np.unique(x[:, :, -1])) == set(rb.BLOCKS)
    idx = rb.frame_idx("P")
    assert len(idx) == 20 and idx.max() < 23 and np.all(np.diff(idx) > 0)


@pytest.mark.parametrize("geom", list(rb.GEOMETRIES))
def test_restatement_matches_the_reference(fixture, geom):
    out = rb.run(geom)
    assert out["n_iter"] == fixture[f"{geom}/n_iter"] and out["func_evals"] == fixture[f"{geom}/func_evals"]
    d, s = rb.distances(out, fixture, geom)
    for k, v in d.items():
        assert v <= FACTOR * s[k], (geom, k, v, s[k])


def test_prepared_inputs_have_the_references_layout():
    prepared, gt = rb.prepare(rb.make_raw("P"), "all", rb.frame_idx("P"))
    raw = rb.make_raw("P")["P"]
    p = prepared["P"]
    assert p["X"][0].shape == (11, 20, 2 + 3 + 4 + 1) and p["X"][0].dtype == np.float64
    assert np.all(p["X"][1][:, :, -1] == 1.0) and p["y"][0].dtype == np.float32
    assert np.array_equal(gt["P"], raw["y"][1])
    # const = 3 drops the first continuous column (train_rrr.py:133-140), 'me' leaves X alone
    assert rb.prepare(rb.make_raw("P"), "me-all", rb.frame_idx("P"))[0]["P"]["X"][0].shape[2] == 2 + 3 + 3 + 1
    assert rb.prepare(rb.make_raw("P"), "me", rb.frame_idx("P"))[0]["P"]["X"][0].shape[2] == 6 + 1


@pytest.mark.parametrize("name", list(rb.SMOOTH_INPUTS))
def test_scipy_order_smoothing_is_bit_equal(fixture, name):
    y = rb.smooth_input(name)
    want = fixture[f"smooth/{name}"]
    got = rb.smooth(y)
    assert got.dtype == want.dtype == y.dtype and np.array_equal(got, want)
    # the weights the library is given are the restatement's
    from vspike import ops
    w, radius = ops.gauss_weights(rb.SMOOTH_W)
    w2, r2 = rb.gauss_weights(rb.SMOOTH_W)
    assert radius == r2 == 8 and np.array_equal(w, w2) and w.dtype == np.float64


def test_host_argument_errors():
    from vspike._lib import VsError
    from vspike.rrr import RRRGD, check_dims_wide, prepare_rrr_inputs
    check_dims_wide(1024, 8)
    y = torch.zeros(2, 3, 4)
    with pytest.raises(VsError, match="1025 features"):
        RRRGD().fit({"a": (torch.zeros(2, 3, 1026, dtype=torch.float64), y)})
    with pytest.raises(VsError, match="9 components"):
        RRRGD(n_comp=9).fit({"a": (torch.zeros(2, 3, 4, dtype=torch.float64), y)})
    with pytest.raises(VsError, match="float64"):
        RRRGD().fit({"a": (torch.zeros(2, 3, 4), y)})
    with pytest.raises(VsError, match="T must be equal"):
        RRRGD().fit({"a": (torch.zeros(2, 3, 4, dtype=torch.float64), y),
                     "b": (torch.zeros(2, 5, 4, dtype=torch.float64), torch.zeros(2, 5, 4))})
    with pytest.raises(VsError, match="at least one session"):
        RRRGD().fit({})
    with pytest.raises(VsError, match="no fitted session"):
        RRRGD().U("a")
    # prepare_rrr_inputs: the checks come before anything reaches the device
    dev = "cpu"
    d = {"a": {"X": [np.zeros((2, 6, 3)), np.zeros((2, 6, 3))], "y": [np.zeros((2, 5, 4), np.float32)] * 2},
         "b": {"X": [np.zeros((2, 6, 3)), np.zeros((2, 6, 3))], "y": [np.zeros((2, 4, 4), np.float32)] * 2}}
    with pytest.raises(VsError, match="T must be equal"):
        prepare_rrr_inputs(d, "vit", device=dev)
    one = {"a": d["a"]}
    with pytest.raises(VsError, match="input_mod"):
        prepare_rrr_inputs(one, "pixels", device=dev)
    for bad in (np.arange(4), np.arange(5) + 2, np.arange(5) - 1, np.arange(5) * 1.0):
        with pytest.raises(VsError, match="frame indices"):
            prepare_rrr_inputs(one, "vit", idx=bad, device=dev)
    with pytest.raises(VsError, match="cannot draw"):
        prepare_rrr_inputs({"a": {"X": [np.zeros((2, 5, 3))] * 2, "y": d["a"]["y"]}}, "vit", device=dev)


def test_one_hot_categories_must_match():
    """The two splits' categories are the sorted distinct values of each split; when they differ the reference
    fails with a shape error at the standardisation, here a VsError says so."""
    from vspike._lib import VsError
    from vspike.rrr import _one_hot, prepare_rrr_inputs
    col = torch.tensor([[0.5], [0.2], [0.5], [0.8]], dtype=torch.float64)
    oh, cats = _one_hot(col, 3)
    assert oh.shape == (4, 3, 3) and cats.tolist() == [0.2, 0.5, 0.8]
    want = rb._one_hot(col.numpy(), 3)
    assert np.array_equal(oh.numpy(), want) and oh.dtype == torch.float64
    # a validation split without the third block: the check fires before anything reaches the device
    X = np.zeros((4, 6, 3))
    X[:, :, 1] = np.array([-1.0, 1.0, -1.0, 1.0])[:, None]
    X[:, :, 2] = np.array([0.2, 0.5, 0.8, 0.2])[:, None]
    Xv = X[:3].copy()
    Xv[2, :, 2] = 0.5
    y = [np.zeros((4, 5, 2), np.float32), np.zeros((3, 5, 2), np.float32)]
    with pytest.raises(VsError, match="do not have the same choice / block categories"):
        prepare_rrr_inputs({"a": {"X": [X, Xv], "y": y}}, "all", idx=np.arange(5), device="cpu")


def test_library_rejects_unsupported_sizes_without_launching(built_lib):
    from vspike import _lib
    lib = _lib.lib()
    assert lib.vs_version() >= 9
    one = ctypes.c_void_p(16)                      # never dereferenced: the size checks come first
    for C, r, word in ((1025, 3, "C <= 1024"), (0, 3, "C <= 1024"), (40, 9, "r <= 8"), (40, 0, "r <= 8")):
        rc = lib.vs_rrr_wide_loss_grad(4, 5, 6, C, r, one, one, _lib.VS_F32, one, one, one, 100.0, one, None, None,
                                       None, one, None)
        assert rc == -1 and word in lib.vs_last_error().decode(), (C, r, lib.vs_last_error())
        rc = lib.vs_rrr_wide_score(4, 5, 6, C, r, one, one, one, one, one, one, one, _lib.VS_F32, None, one, one,
                                   one, one, None)
        assert rc == -1 and word in lib.vs_last_error().decode(), (C, r, lib.vs_last_error())
    rc = lib.vs_rrr_wide_loss_grad(4, 5, 6, 40, 3, one, one, _lib.VS_BF16, one, one, one, 100.0, one, None, None, None,
                                   one, None)
    assert rc == -1 and "f32 or f64" in lib.vs_last_error().decode()
    rc = lib.vs_rrr_wide_loss_grad(4, 5, 6, 40, 3, one, one, _lib.VS_F64, one, one, one, 100.0, one, one, None, None,
                                   one, None)
    assert rc == -1 and "together" in lib.vs_last_error().decode()
    # T < radius + 1: a second reflection would be needed
    rc = lib.vs_gauss_smooth_time(3, 8, 5, one, _lib.VS_F32, one, 8, ctypes.c_void_p(32), None)
    assert rc == -1 and "radius + 1" in lib.vs_last_error().decode()
    rc = lib.vs_gauss_smooth_time(3, 9, 5, one, _lib.VS_BF16, one, 8, ctypes.c_void_p(32), None)
    assert rc == -1 and "f32 or f64" in lib.vs_last_error().decode()
    # the workspace formula of the header comment: K T N + T (C+2) N + (C+2) ceil(N/64) + chunks 8 T doubles, each piece
    # rounded up to 256 bytes
    assert lib.vs_rrr_wide_loss_grad_workspace_bytes(4, 5, 6, 1025) == 0
    need = lib.vs_rrr_wide_loss_grad_workspace_bytes(13, 20, 65, 40)
    exact = 8 * (13 * 20 * 65 + 20 * 42 * 65 + 42 * 2 + 20 * 8 * 20)
    assert exact <= need <= exact + 4 * 256 and need % 256 == 0
    big = lib.vs_rrr_wide_loss_grad_workspace_bytes(400, 100, 512, 768)
    assert 0.47e9 < big < 0.49e9
    assert lib.vs_rrr_wide_score_workspace_bytes(5, 20, 65) >= 8 * (5 * 20 * 65 + 5 * 65)
    # the RRR counters are a group of their own; the pinned VS_PATH_* total has not moved
    assert _lib.RRR_PATH_NAMES == ("rrr_wide", "gauss_smooth")
    _lib.dispatch_reset()
    assert _lib.rrr_dispatch_counts() == {"rrr_wide": 0, "gauss_smooth": 0}
