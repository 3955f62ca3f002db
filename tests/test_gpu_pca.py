"""The PCA video embedding on the GPU (csrc/pca.hip, vspike/pca.py): the three kernels against float64 numpy under
the forward error bound of an f32 dot product, their memory hygiene and determinism, the solver against the fixture
(tests/golden/pca.npz) under the reference's own spread, and the RRR baseline end to end from raw video.

Every case prints its observed error-to-bound ratio before it asserts (run with -s); profiles/pca_tests.txt holds the
worst of a run on an MI355X."""
import numpy as np
import pytest
import torch

import pca_ref as pr
import rrr_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24            # unit roundoff of f32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("pca.npz")


def _tiles():
    from vspike import ops
    return ops.pca_tiles()


def _row_counts():
    """2 rows, under one row tile, one row tile + 1, and enough rows for a second reduction chunk."""
    t = _tiles()
    return (2, 84, t["rows"] + 1, t["chunk_rows"] + 1)


def _matrix(M, D, dtype, seed):
    rs = np.random.RandomState(seed)
    if dtype == np.uint8:
        return rs.randint(0, 256, size=(M, D)).astype(np.uint8)
    return (100.0 + 50.0 * rs.normal(size=(M, D))).astype(np.float32)


# M is taken from the kernels' own tile constants at run time; the ids name the role
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("D", [1, 3, 572, 703])
@pytest.mark.parametrize("mi", range(4), ids=["two_rows", "part_tile", "tile_plus_1", "two_chunks"])
def test_ops_against_float64(mi, D, dtype):
    """colmean to float64 rounding; project and gram_apply for L in {1, 15, 32} under
        |Y - Y64| <= (D + 2) u (|Xc| |Q|)                          (one f32 dot product of length D)
        |W - W64| <= ((D + 2) + (M + 2)) u |Xc|^T (|Xc| |Q|)      (its error carried through the second one)
    elementwise, u = 2^-24: K terms of accumulation + the rounding of the two operands to f32."""
    from vspike import ops
    M = _row_counts()[mi]
    X = _matrix(M, D, dtype, 1000 * mi + D)
    X64 = X.astype(np.float64)
    Xd = torch.from_numpy(X).to(DEV)
    mean = X64.mean(axis=0)
    mu = ops.pca_colmean(Xd)
    tol = 2.0 * M * 2.0 ** -53 * np.abs(X64).mean(axis=0) + 1e-300
    r_mean = float((np.abs(mu.cpu().numpy() - mean) / tol).max())
    # the products are tested on numpy's mean, so that each op stands alone
    mud = torch.from_numpy(mean).to(DEV)
    Xc = X64 - mean
    worst = {"project": 0.0, "gram_apply": 0.0}
    for L in (1, 15, 32):
        Q = np.random.RandomState(7 + L).normal(size=(D, L))
        Qd = torch.from_numpy(Q).to(DEV)
        A = np.abs(Xc) @ np.abs(Q)
        Y = ops.pca_project(Xd, mud, Qd).cpu().numpy()
        W = ops.pca_gram_apply(Xd, mud, Qd).cpu().numpy()
        assert Y.shape == (M, L) and W.shape == (D, L)
        by = (D + 2) * U * A
        bw = ((D + 2) + (M + 2)) * U * (np.abs(Xc).T @ A)
        ey, ew = np.abs(Y - Xc @ Q), np.abs(W - Xc.T @ (Xc @ Q))
        # a zero bound (a constant column: Xc = 0 exactly) admits a zero error only
        assert (ey[by == 0] == 0).all() and (ew[bw == 0] == 0).all()
        ry = float((ey[by > 0] / by[by > 0]).max()) if (by > 0).any() else 0.0
        rw = float((ew[bw > 0] / bw[bw > 0]).max()) if (bw > 0).any() else 0.0
        worst["project"], worst["gram_apply"] = max(worst["project"], ry), max(worst["gram_apply"], rw)
    print(f"pca ops M {M} D {D} {np.dtype(dtype).name}: error / bound colmean {r_mean:.3g}, "
          f"project {worst['project']:.3g}, gram_apply {worst['gram_apply']:.3g}")
    assert r_mean <= 1.0
    assert worst["project"] <= 1.0 and worst["gram_apply"] <= 1.0


def _guarded(n, dtype=torch.float64, guard=64):
    """A NaN-filled buffer and the view of its middle n elements (the guard is 512 bytes: alignment is kept)."""
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[guard:guard + n]


def _guards_intact(buf, n, guard=64):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("D,L", [(703, 15), (131, 32), (3, 1)])
def test_memory_hygiene_and_determinism(D, L, dtype):
    """X sits at an odd element offset inside a buffer whose other bytes are filled twice over (u8: 0 / 255, f32: NaN /
    3e4); outputs and workspace sit inside NaN-filled buffers.  The guard regions stay NaN, the results are finite and
    bitwise equal across fills and repeated calls, and the counter of each entry point moves by one per call."""
    from vspike import _lib as Lb, ops
    t = _tiles()
    M = t["chunk_rows"] + t["rows"] + 5                      # two chunks, a partial row tile
    rs = np.random.RandomState(D + L)
    if dtype == torch.uint8:
        X = torch.from_numpy(rs.randint(0, 256, size=(M, D)).astype(np.uint8))
        fills = (0, 255)
    else:
        X = torch.from_numpy((100.0 + 50.0 * rs.normal(size=(M, D))).astype(np.float32))
        fills = (float("nan"), 3.0e4)
    Q = torch.from_numpy(rs.normal(size=(D, L))).to(DEV)
    pad = 257                                                # odd: a uint8 X starts at an odd address
    outs = []
    for fill in fills:
        xbuf = torch.full((M * D + 2 * pad,), fill, dtype=dtype, device=DEV)
        xbuf[pad:pad + M * D].copy_(X.reshape(-1))
        Xd = xbuf[pad:pad + M * D].view(M, D)
        for _ in range(2):
            Lb.dispatch_reset()
            mbuf, mu = _guarded(D)
            ybuf, Y = _guarded(M * L)
            wbuf, W = _guarded(D * L)
            need = [ops.pca_colmean_workspace_bytes(M, D) // 8, ops.pca_project_workspace_bytes(M, D, L) // 8,
                    ops.pca_gram_apply_workspace_bytes(M, D, L) // 8]
            ws = [_guarded(n) for n in need]
            ops.pca_colmean(Xd, mu=mu, workspace=ws[0][1])
            assert Lb.pca_dispatch_counts() == {"pca_colmean": 1, "pca_project": 0, "pca_gram_apply": 0}
            ops.pca_project(Xd, mu, Q, Y=Y.view(M, L), workspace=ws[1][1])
            assert Lb.pca_dispatch_counts() == {"pca_colmean": 1, "pca_project": 1, "pca_gram_apply": 0}
            ops.pca_gram_apply(Xd, mu, Q, W=W.view(D, L), workspace=ws[2][1])
            assert Lb.pca_dispatch_counts() == {"pca_colmean": 1, "pca_project": 1, "pca_gram_apply": 1}
            torch.cuda.synchronize()
            for (buf, _), n in zip(ws, need):
                assert _guards_intact(buf, n), "a workspace guard was written"
            assert _guards_intact(mbuf, D) and _guards_intact(ybuf, M * L) and _guards_intact(wbuf, D * L)
            assert torch.equal(xbuf[pad:pad + M * D].cpu(), X.reshape(-1))      # X itself is read only
            outs.append((mu.clone(), Y.clone(), W.clone()))
    for o in outs[0]:
        assert torch.isfinite(o).all()
    for k, run in enumerate(outs[1:], 1):
        for name, a, b in zip(("mu", "Y", "W"), run, outs[0]):
            assert torch.equal(a, b), (name, k, float((a - b).abs().max()))


def _fit(fx, g, dtype):
    from vspike.pca import PCA
    n, t, h, w = pr.GEOMETRIES[g]
    X = torch.from_numpy(fx[f"{g}/video"].reshape(n * t, h * w)).to(DEV)
    p = PCA(n_components=pr.K_COMP)
    return p, p.fit_transform(X.to(dtype))


@pytest.mark.parametrize("g", tuple(pr.GEOMETRIES))
def test_fixture_scores_within_twice_the_reference_spread(fx, g):
    """PCA.fit_transform on the fixture's videos: scores and singular values within 2 x the reference's spread of the
    exact answer (both are f32 roundings of the same quantity; the factor 2 is for the MFMA's order of summation
    against numpy's), the fixture's signs, converged, and uint8 and float32 input alike."""
    n, t, h, w = pr.GEOMETRIES[g]
    spread = float(fx[f"{g}/spread"])
    Z = fx[f"{g}/scores"].reshape(n * t, -1)
    p8, z8 = _fit(fx, g, torch.uint8)
    p32, z32 = _fit(fx, g, torch.float32)
    d8, d32 = pr.score_distance(z8.cpu().numpy(), Z), pr.score_distance(z32.cpu().numpy(), Z)
    s8 = pr.score_distance(p8.singular_values_.cpu().numpy(), fx[f"{g}/singular_values"])
    s32 = pr.score_distance(p32.singular_values_.cpu().numpy(), fx[f"{g}/singular_values"])
    d_in = pr.score_distance(z32.cpu().numpy(), z8.cpu().numpy())
    print(f"pca fixture {g}: scores {d8:.3e} (u8) {d32:.3e} (f32), singular values {s8:.3e} {s32:.3e}, u8 against f32 "
          f"{d_in:.3e}, reference spread {spread:.3e} ({max(d8, d32) / spread:.2g} x), {p8.n_iter_} steps, residuals "
          f"{np.array2string(p8.residuals_, precision=2)}, small linear algebra on the {p8.timing_['linalg']}")
    assert z8.dtype == torch.float64 and z8.shape == (n * t, pr.K_COMP)
    assert p8.converged_ and p32.converged_
    assert max(d8, d32) <= 2 * spread and max(s8, s32) <= 2 * spread and d_in <= 2 * spread
    comps = p8.components_.cpu().numpy()
    want = fx[f"{g}/components"]
    assert comps.shape == want.shape
    assert ((comps * want).sum(axis=1) > 0).all()                              # the fixture's signs
    assert (comps[np.arange(pr.K_COMP), np.abs(comps).argmax(axis=1)] > 0).all()
    assert np.abs(comps - want).max() <= 1e-3                                  # and its directions
    mean = p8.mean_.cpu().numpy()
    assert np.abs(mean - fx[f"{g}/mean"]).max() <= 1e-12 * 255
    ev = p8.explained_variance_.cpu().numpy()
    sv = fx[f"{g}/singular_values"]
    assert np.abs(ev - sv ** 2 / (n * t - 1)).max() <= 5 * spread * sv[0] ** 2 / (n * t - 1)   # (s + 2 e s_1)^2


def test_embedding_and_transform_shapes(fx):
    """pca_embedding takes (n, t, 1, h, w) and (n, t, h, w), numpy and device tensors; transform of the fitted rows
    is fit_transform's result."""
    from vspike.pca import PCA, pca_embedding
    video = fx["A/video"]
    n, t = video.shape[:2]
    a = pca_embedding(video, out_dim=3)
    b = pca_embedding(torch.from_numpy(video[:, :, 0]).to(DEV), out_dim=3)
    assert a.shape == (n, t, 3) and a.dtype == torch.float64 and a.is_cuda and torch.equal(a, b)
    X = torch.from_numpy(video.reshape(n * t, -1)).to(DEV)
    p = PCA(3)
    assert torch.equal(p.fit_transform(X), p.transform(X))
    assert torch.equal(p.transform(X[:7]), p.transform(X)[:7])


def test_solver_rejections_on_device():
    from vspike._lib import VsError
    from vspike.pca import PCA
    X = torch.zeros(6, 9, dtype=torch.uint8, device=DEV) + 17
    with pytest.raises(VsError, match="zero total variance"):
        PCA(2).fit(X)
    with pytest.raises(VsError, match="components need"):
        PCA(6).fit(X)
    with pytest.raises(VsError, match="uint8 or float32"):
        PCA(2).fit(X.double())


def test_max_iter_warns():
    from vspike.pca import PCA
    X = torch.from_numpy(_matrix(40, 50, np.uint8, 3)).to(DEV)
    p = PCA(3, max_iter=1)
    with pytest.warns(RuntimeWarning, match="did not reach tol"):
        p.fit(X)
    assert not p.converged_ and p.n_iter_ == 1


def test_rrr_baseline_from_raw_video(fx):
    """pca_rrr_data + train_rrr_baseline(data, 'pca') on geometry C against the reference's scores sent through the
    restated baseline (fixture): co-bps and R^2 per neuron within 100 x the reference's spread over its 8 seeds."""
    from vspike.pca import pca_rrr_data
    from vspike.rrr import train_rrr_baseline
    video, spikes, idx = fx["C/video"], fx["C/spikes"], fx["C/idx"]
    kt = pr.C_TRAIN
    data = pca_rrr_data(video[:kt], spikes[:kt], video[kt:], spikes[kt:], out_dim=pr.K_COMP, eid="C")
    assert list(data) == ["C"] and data["C"]["X"][0].shape == (kt, video.shape[1], pr.K_COMP)
    assert data["C"]["X"][1].shape == (video.shape[0] - kt, video.shape[1], pr.K_COMP) and data["C"]["setup"] == {}
    result, mean_bps = train_rrr_baseline(data, "pca", idx=idx)
    got = {"bps": np.array(result["C"]["co_bps"]), "r2": np.array(result["C"]["r2"])}
    got["co_bps"] = np.nanmean(got["bps"])
    assert abs(mean_bps - got["co_bps"]) <= 1e-12 * abs(got["co_bps"])
    ratios = {}
    for key in ("bps", "r2"):
        ratios[key] = rr.dist(got[key], fx[f"C/e2e/{key}"]) / float(fx[f"C/e2e/spread/{key}"])
    ratios["co_bps"] = abs(got["co_bps"] - float(fx["C/e2e/co_bps"])) / abs(float(fx["C/e2e/co_bps"])) \
        / float(fx["C/e2e/spread/co_bps"])
    print(f"pca end to end C: co_bps {got['co_bps']:.6f} (fixture {float(fx['C/e2e/co_bps']):.6f}), distance / "
          f"reference seed spread: {', '.join(f'{k} {v:.3g}' for k, v in ratios.items())}")
    assert all(v <= 100.0 for v in ratios.values()), ratios
