"""The PCA video embedding without a GPU: the numpy restatement (tests/pca_ref.py) against the fixture
(tests/golden/pca.npz, scripts/gen_pca_fixture.py), the sign rule, and the library's host-side contract (version,
the counter group, argument rejections before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import pca_ref as pr

GEOMS = tuple(pr.GEOMETRIES)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("pca.npz")


@pytest.fixture(scope="module")
def restated(fx):
    """The restatement's fit of every geometry, computed once."""
    out = {}
    for g, (n, t, h, w) in pr.GEOMETRIES.items():
        out[g] = pr.subspace_pca(fx[f"{g}/video"].reshape(n * t, h * w))
    return out


@pytest.mark.parametrize("g", GEOMS)
def test_fixture_video_is_make_video(fx, g):
    assert np.array_equal(fx[f"{g}/video"], pr.make_video(g))
    n, t, h, w = pr.GEOMETRIES[g]
    assert max(n * t, h * w) > 500 and pr.K_COMP < 0.8 * min(n * t, h * w)     # sklearn's randomized branch


@pytest.mark.parametrize("g", GEOMS)
def test_exact_pca_is_sklearn_full(fx, g):
    n, t, h, w = pr.GEOMETRIES[g]
    ex = pr.exact_pca(fx[f"{g}/video"].reshape(n * t, h * w))
    Z = fx[f"{g}/scores"].reshape(n * t, -1)
    assert pr.score_distance(ex["scores"], Z) < 1e-11
    assert np.allclose(ex["components"], fx[f"{g}/components"], rtol=0, atol=1e-11)
    assert np.allclose(ex["singular_values"], fx[f"{g}/singular_values"], rtol=1e-12)
    assert np.allclose(ex["mean"], fx[f"{g}/mean"], rtol=1e-14)


@pytest.mark.parametrize("g", GEOMS)
def test_reference_spread_is_what_the_fixture_says(fx, g):
    n, t, h, w = pr.GEOMETRIES[g]
    Z = fx[f"{g}/scores"].reshape(n * t, -1)
    spread = max(pr.score_distance(z.reshape(n * t, -1), Z) for z in fx[f"{g}/ref_scores"])
    assert spread == float(fx[f"{g}/spread"])
    assert 1e-7 < spread < 1e-4          # the reference took its randomized solver, and it worked


@pytest.mark.parametrize("g", GEOMS)
def test_restatement_within_reference_spread(fx, restated, g):
    """The iteration with f32 products lands nearer to the exact scores than the reference's own solver does, so
    the reference's spread is a bar the design can meet."""
    n, t, h, w = pr.GEOMETRIES[g]
    r, spread = restated[g], float(fx[f"{g}/spread"])
    d = pr.score_distance(r["scores"], fx[f"{g}/scores"].reshape(n * t, -1))
    ds = pr.score_distance(r["singular_values"], fx[f"{g}/singular_values"])
    print(f"pca restatement {g}: scores {d:.3e}, singular values {ds:.3e}, reference spread {spread:.3e} "
          f"({d / spread:.2g} x), {r['n_iter']} steps, last residual {r['history'][-1]:.2e}")
    assert r["converged"]
    assert d <= spread and ds <= spread
    assert np.array_equal(np.sign(r["components"]), np.sign(pr.sign_flip(r["components"])))
    big = np.abs(fx[f"{g}/components"]).argmax(axis=1)
    rows = np.arange(pr.K_COMP)
    assert (r["components"][rows, big] > 0).all()             # the fixture's signs


def test_default_tol_is_four_times_the_stall_level(fx):
    """vspike.pca.DEFAULT_TOL comes from here, not from the GPU code: with f32 products the largest top-k residual
    stops falling at a level set by the products' rounding.  That level (the median of steps 10..14, well after the
    float64 iteration has passed it) times 4, over the three geometries, to within 10 %."""
    from vspike import pca
    stall = {}
    for g, (n, t, h, w) in pr.GEOMETRIES.items():
        X = fx[f"{g}/video"].reshape(n * t, h * w)
        h32 = pr.subspace_pca(X, tol=1e-30, max_iter=14)["history"]
        h64 = pr.subspace_pca(X, tol=1e-30, max_iter=14, products=np.float64)["history"]
        assert h64[-1] < 1e-3 * h32[-1]                       # f64 products go on falling: the stall is f32's
        stall[g] = float(np.median(h32[9:14]))
    print(f"pca residual stall levels {stall}")
    want = 4 * max(stall.values())
    assert 0.9 * want <= pca.DEFAULT_TOL <= 1.1 * want, (pca.DEFAULT_TOL, want)


def test_sign_rule():
    """svd_flip(u_based_decision=False): the entry of largest magnitude of every component is positive; numpy and
    torch statements agree."""
    from vspike import pca
    c = np.array([[0.1, -0.9, 0.3], [0.5, 0.2, -0.4], [-0.2, -0.3, 0.0], [0.0, 0.0, 0.0]])
    want = np.array([[-0.1, 0.9, -0.3], [0.5, 0.2, -0.4], [0.2, 0.3, 0.0], [0.0, 0.0, 0.0]])
    assert np.array_equal(pr.sign_flip(c), want)
    assert np.array_equal(pca.sign_flip(torch.from_numpy(c)).numpy(), want)
    assert np.allclose(pr.sign_margin(c[:2]), [(0.9 - 0.3) / 0.9, 0.1 / 0.5])


@pytest.mark.parametrize("g", GEOMS)
def test_fixture_signs_are_no_coin_toss(fx, g):
    assert (pr.sign_margin(fx[f"{g}/components"]) >= 1e-3).all()
    if g == "B":
        sv = fx["B/singular_values"]
        assert abs(sv[1] - sv[2]) / sv[1] < 0.04


def test_start_block_is_fixed():
    from vspike import pca
    state = torch.get_rng_state()
    a, b = pca.start_block(37, 6), pca.start_block(37, 6)
    assert torch.equal(a, b) and a.dtype == torch.float64 and a.shape == (37, 6)
    assert torch.equal(torch.get_rng_state(), state)          # the global generator is left alone


def test_version_and_counters():
    from vspike import _lib as L
    assert L.lib().vs_version() >= 10
    L.dispatch_reset()
    assert L.pca_dispatch_counts() == {"pca_colmean": 0, "pca_project": 0, "pca_gram_apply": 0}
    assert L.PCA_PATH_NAMES == ("pca_colmean", "pca_project", "pca_gram_apply")


def test_tiles_and_workspace_formulas():
    from vspike import ops
    t = ops.pca_tiles()
    assert t == {"rows": 128, "cols": 128, "chunk_rows": 512, "max_chunks": 16}

    def al(b):
        return (b + 255) // 256 * 256
    for M, D, L in ((2, 1, 1), (84, 572, 15), (513, 703, 32), (60000, 18260, 15)):
        chunks = min(-(-M // t["chunk_rows"]), t["max_chunks"])
        rows = -(-(-(-M // chunks)) // 128) * 128
        chunks = -(-M // rows)
        Dp, Mp = -(-D // 64) * 64, -(-M // 128) * 128
        assert ops.pca_colmean_workspace_bytes(M, D) == al(chunks * D * 8)
        assert ops.pca_project_workspace_bytes(M, D, L) == al(Dp * 32 * 4)
        assert ops.pca_gram_apply_workspace_bytes(M, D, L) == al(Dp * 32 * 4) + al(Mp * 32 * 4) + al(chunks * D * L * 8)
    # the session shape: well under the 1.1 GB of the uint8 pixels
    assert ops.pca_gram_apply_workspace_bytes(60000, 18260, 15) < 0.05 * 60000 * 18260


def test_rejections_without_a_device():
    """Bad arguments return VS_EINVAL before any launch (no GPU is touched: this runs without one)."""
    from vspike import _lib as L
    lib = L.lib()
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                            # 16-byte aligned, 56 doubles behind it
    L.dispatch_reset()
    U8, F32 = L.VS_U8, L.VS_F32
    assert lib.vs_pca_colmean(1, 8, p, U8, p, p, None) == -1               # M < 2
    assert lib.vs_pca_colmean(4, 0, p, U8, p, p, None) == -1               # D < 1
    assert lib.vs_pca_colmean(4, 8, p, L.VS_BF16, p, p, None) == -1        # dtype
    assert lib.vs_pca_colmean(4, 8, None, U8, p, p, None) == -1            # null
    assert lib.vs_pca_colmean(4, 8, p + 1, F32, p, p, None) == -1          # an f32 X off its alignment
    assert lib.vs_pca_project(4, 8, 0, p, U8, p, p, p, p, None) == -1      # L < 1
    assert lib.vs_pca_project(4, 8, 33, p, U8, p, p, p, p, None) == -1     # L > 32
    assert lib.vs_pca_project(4, 8, 2, p, U8, p, p, p, p + 8, None) == -1  # workspace alignment
    assert lib.vs_pca_gram_apply(4, 8, 33, p, F32, p, p, p, p, None) == -1
    assert lib.vs_pca_gram_apply(1, 8, 2, p, F32, p, p, p, p, None) == -1
    assert lib.vs_pca_gram_apply(4, 8, 2, p, F32, p, p, None, p, None) == -1
    assert b"vs_pca_gram_apply" in lib.vs_last_error()
    for fn, args in ((lib.vs_pca_colmean_workspace_bytes, (1, 8)), (lib.vs_pca_project_workspace_bytes, (4, 8, 33)),
                     (lib.vs_pca_gram_apply_workspace_bytes, (4, 8, 0))):
        assert fn(*args) == 0
    assert sum(L.pca_dispatch_counts().values()) == 0                      # nothing was counted as a call


def test_solver_rejections():
    from vspike import pca
    from vspike._lib import VsError
    for k in (0, 17):
        with pytest.raises(VsError, match="components"):
            pca.PCA(n_components=k)
    with pytest.raises(VsError, match="oversample"):
        pca.PCA(n_components=16, oversample=17)
    with pytest.raises(VsError, match="uint8 or float32"):
        pca._as_matrix(np.zeros((4, 4)), device="cpu")
    with pytest.raises(VsError, match=r"\(n, t, 1, h, w\)"):
        pca._as_video(np.zeros((2, 3, 2, 4, 4), np.uint8))
