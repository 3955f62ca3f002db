"""The reduced-rank regression validation without a GPU: tests/rrr_ref.py (the float64 restatement the GPU tests
compare against) held to tests/golden/rrr.npz (the reference's own train_rrr / RRRGD, scripts/gen_rrr_fixture.py),
and the host logic of vspike.rrr.

Bars: 100 x the spread the fixture records for the reference itself (the same run with the standardised training
trials in another order: one sample of what float64 summation order does to a 20-iteration L-BFGS fit without a
line search; U and V move by ~2e-7 of their largest element, the losses by ~5e-9).  Distances and spreads are
max |a - b| / max |a|; b is judged against max |U V|, since it sits at 1e-8 after standardisation and its own
scale means nothing.
"""
import ctypes

import numpy as np
import pytest
import torch

import rrr_ref as rr

FACTOR = 100.0


@pytest.fixture(scope="module")
def built_lib():
    from vspike import build
    build.build(verbose=False)
    return build.LIB_PATH


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("rrr.npz")


def compare(got, fx, geom, factor=FACTOR):
    d, s = rr.distances(got, fx, geom)
    for k, v in d.items():
        assert v <= factor * s[k], (geom, k, v, s[k])


def test_fixture_is_what_the_issue_asks(fixture):
    for geom in rr.GEOMETRIES:
        assert fixture[f"{geom}/n_iter"] == 20 and fixture[f"{geom}/func_evals"] == 20
        assert fixture[f"{geom}/losses"].shape == (20,)
        nan = np.isnan(fixture[f"{geom}/bps"])
        assert nan[rr.SILENT] and nan.sum() <= 3 and np.isfinite(fixture[f"{geom}/bps"][rr.SILENT_IN_TRAIN])
        s = rr.spreads(fixture, geom)
        assert all(0 < v < 1e-5 for v in s.values()), s


@pytest.mark.parametrize("geom", list(rr.GEOMETRIES))
def test_restatement_matches_the_reference(fixture, geom):
    out = rr.run(geom)
    assert out["n_iter"] == fixture[f"{geom}/n_iter"] and out["func_evals"] == fixture[f"{geom}/func_evals"]
    compare(out, fixture, geom)
    # the branches the data was built to reach: a silent neuron (NaN bps), silent neuron-trials scoring exactly 0
    gt = rr.make_data(geom)["y"][1]
    silent = gt.sum(1) == 0                                                   # (K, N)
    assert silent[:, rr.SPARSE].any() and silent[0, 3] and silent[:, rr.SILENT].all()
    assert np.all(out["r2_kn"][silent] == 0.0)
    assert np.isnan(out["bps"][rr.SILENT]) and out["r2"][rr.SILENT] == 0.0


@pytest.mark.parametrize("geom", list(rr.GEOMETRIES))
def test_initialisation_is_the_reference_draw(fixture, geom):
    """vspike.rrr.init_params draws RRRGD's U and V: the loss at (U0, V0, b0 = mean_k y) is the fixture's first
    closure value to rounding (1e-13 relative: a float64 sum of 1e5 terms in another order)."""
    from vspike.rrr import init_params
    g = rr.GEOMETRIES[geom]
    Xs, ys, _, _ = rr.standardise(rr.make_data(geom))
    U0, V0 = init_params(g["T"], g["N"], g["C"], g["r"])
    Ur, Vr = rr.init(g["T"], g["N"], g["C"], g["r"])
    assert np.array_equal(U0, Ur) and np.array_equal(V0, Vr) and U0.dtype == np.float64
    b0 = torch.from_numpy(ys[0]).double().mean(0).t().unsqueeze(1)
    first = float(rr.loss(Xs[0], ys[0], U0, V0, b0, rr.L2))
    want = float(fixture[f"{geom}/losses"][0])
    assert abs(first - want) <= 1e-13 * want, (first, want)
    # another seed does not reproduce it
    Ux = np.random.RandomState(1).normal(size=U0.shape) / np.sqrt(g["T"] * g["r"])
    assert abs(float(rr.loss(Xs[0], ys[0], Ux, V0, b0, rr.L2)) - want) > 1e-6 * want


def test_host_argument_errors():
    from vspike._lib import VsError
    from vspike.rrr import RRR, check_dims, init_params
    check_dims(32, 8)
    y = torch.zeros(2, 3, 4)
    with pytest.raises(VsError, match="33 features"):
        RRR().fit(torch.zeros(2, 3, 34, dtype=torch.float64), y)
    with pytest.raises(VsError, match="9 components"):
        RRR(n_comp=9).fit(torch.zeros(2, 3, 4, dtype=torch.float64), y)
    with pytest.raises(VsError, match="components"):
        init_params(5, 4, 3, 0)
    with pytest.raises(VsError, match="float64"):
        RRR().fit(torch.zeros(2, 3, 4), y)
    with pytest.raises(VsError):
        RRR().fit(torch.zeros(2, 3, 4, dtype=torch.float64), torch.zeros(2, 5, 4))


def test_library_rejects_unsupported_sizes_without_launching(built_lib):
    from vspike import _lib
    lib = _lib.lib()
    assert lib.vs_version() >= 8
    one = ctypes.c_void_p(16)                      # never dereferenced: the size checks come first
    for C, r, word in ((33, 3, "C <= 32"), (0, 3, "C <= 32"), (3, 9, "r <= 8"), (3, 0, "r <= 8")):
        rc = lib.vs_rrr_loss_grad(4, 5, 6, C, r, one, one, _lib.VS_F32, one, one, one, 100.0, one, None, None, None,
                                  one, None)
        assert rc == -1 and word in lib.vs_last_error().decode(), (C, r, lib.vs_last_error())
        rc = lib.vs_rrr_score(4, 5, 6, C, r, one, one, one, one, one, one, one, _lib.VS_F32, None, one, one, one, one,
                              None)
        assert rc == -1 and word in lib.vs_last_error().decode(), (C, r, lib.vs_last_error())
    rc = lib.vs_rrr_loss_grad(4, 5, 6, 3, 3, one, one, _lib.VS_BF16, one, one, one, 100.0, one, None, None, None, one,
                              None)
    assert rc == -1 and "f32 or f64" in lib.vs_last_error().decode()
    rc = lib.vs_rrr_loss_grad(4, 5, 6, 3, 3, one, one, _lib.VS_F64, one, one, one, 100.0, one, one, None, None, one,
                              None)
    assert rc == -1 and "together" in lib.vs_last_error().decode()
    assert lib.vs_rrr_loss_grad_workspace_bytes(4, 5, 6, 33) == 0
    # S T (C+2) N partials + T (C+1) N + (C+2) N doubles, each rounded up to 256 bytes; 13 trials of 100 x 65: S = 1
    need = lib.vs_rrr_loss_grad_workspace_bytes(13, 100, 65, 5)
    assert need >= 8 * (100 * 7 * 65 + 100 * 6 * 65 + 7 * 65) and need % 256 == 0
    assert lib.vs_rrr_score_workspace_bytes(5, 65) >= 8 * 5 * 65
