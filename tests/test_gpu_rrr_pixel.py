"""The RRR baseline on raw pixels on the GPU: vs_rrr_pixel_stats, vs_rrr_pixel_loss_grad, vs_rrr_pixel_score
(csrc/rrr_pixel.hip) and vspike.rrr's PixelFeatures through RRRGD, prepare_rrr_inputs and train_rrr_baseline.

Kernel bars are those of tests/test_gpu_rrr_wide.py.  vs_rrr_pixel_loss_grad against float64 torch autograd on the
CPU over the numpy-standardised X: loss 1e-12 relative, each gradient 1e-12 of its norm (any float64 order passes,
any float32 shortcut fails: the note in test_gpu_rrr_wide.py).  vs_rrr_pixel_score against tests/rrr_ref.py: pred
1e-12, bps and R^2 per neuron 1e-10, NaN positions equal.  vs_rrr_pixel_stats against np.mean / np.std / np.clip on
the host: the same bits.  Every operand sits in a larger allocation whose margins hold NaN (X: 0xFF bytes, and a
uint8 X starts at an odd address) and the workspace is pre-filled with NaN: the results must be the bits of a run
on plain tensors, and of a second run.

Fit bars: the table above FIT_MEASURED.
"""
import numpy as np
import pytest
import torch

import rrr_pixel_ref as rp
import rrr_ref as rr
import test_gpu_rrr_wide as tw

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (K, F, T, N, C, r), idx: C + 1 = 34 no multiple of 4, C odd, under one MFMA tile in K and N | N crosses 64 and K
# crosses 16, with tails | two neuron tiles + a tail, five feature tiles (C + 1 = 258), r at its cap, C odd |
# C over the wide cap, 18 feature tiles, K under one MFMA k-step.  Every idx skips frames and is not 0..T-1.
SHAPES = [((5, 4, 3, 9, 33, 2), (1, 2, 3)), ((19, 6, 4, 70, 100, 3), (0, 2, 3, 5)),
          ((33, 3, 2, 130, 257, 4), (0, 2)), ((3, 3, 2, 17, 1100, 1), (1, 2))]
IDS = ["x".join(map(str, s)) for s, _ in SHAPES]
XDTYPES = [torch.uint8, torch.float32]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("rrr_pixel.npz")


def _guard_x(X):
    """tw._guard for the video: byte margins of 0xFF (NaN bits for float32), a uint8 X at an odd address."""
    if X.dtype != torch.uint8:
        return tw._guard(X)
    pad = 2049
    buf = torch.full((X.numel() + 2 * pad,), 255, dtype=torch.uint8, device=DEV)
    view = buf[pad:pad + X.numel()].view(X.shape)
    view.copy_(X)
    assert view.data_ptr() % 2 == 1
    return buf, view


def _margins_ok(buf, numel):
    if buf.dtype != torch.uint8:
        return tw._margins_nan(buf, numel)
    pad = (buf.numel() - numel) // 2
    return bool((buf[:pad] == 255).all() and (buf[pad + numel:] == 255).all())


def _video(K, F, C, xdtype, seed=0):
    """Pixels 0..255 (float32: + a fraction), column 1 constant over the trials (std clipped to 1e-8)."""
    g = torch.Generator().manual_seed(77 * seed + K * 131 + C)
    X = torch.randint(0, 256, (K, F, C), generator=g, dtype=torch.int64)
    X[:, :, 1 % C] = 7
    if xdtype == torch.uint8:
        return X.to(torch.uint8)
    X = X.float() + torch.rand(K, F, C, generator=g)
    X[:, :, 1 % C] = 7.25
    return X


def _np_stats(X):
    """utils.py:107-110 on the host, in numpy's dtypes: float64 for uint8, float32 for float32."""
    a = X.numpy()
    return np.mean(a, axis=0), np.clip(np.std(a, axis=0), 1e-8, None)


def _np_standardised(X, idx, mean, std):
    """The float64 X [K, T, C+1] the reference builds: (x - mean) / std in numpy's dtype, the bias column, the
    selected frames."""
    z = ((X.numpy() - mean) / std).astype(np.float64)
    return torch.from_numpy(np.concatenate([z, np.ones(z.shape[:2] + (1,))], axis=2)[:, list(idx)])


def _operands(shape, idx, xdtype, ydtype, seed=0):
    K, F, T, N, C, r = shape
    X = _video(K, F, C, xdtype, seed)
    mean, std = _np_stats(X)
    _, y, U, V, b = tw._inputs(K, T, N, C, r, ydtype, seed=seed)
    Xs = _np_standardised(X, idx, mean, std)
    return X, torch.tensor(idx, dtype=torch.int64), torch.from_numpy(mean), torch.from_numpy(std), Xs, y, U, V, b


def _call_loss_grad(X, idx, mean, std, y, U, V, b, l2, grad=True, guarded=True):
    """One vs_rrr_pixel_loss_grad call; with `guarded` every operand and output sits between margins and the
    workspace starts as NaN.  Returns (loss, dU, dV, db) on the host."""
    from vspike import ops
    K, T, N = y.shape
    C, r = X.shape[2], U.shape[2]
    bufs = []

    def put(t, guard=tw._guard):
        if not guarded:
            return t.to(DEV).contiguous()
        buf, view = guard(t)
        bufs.append((buf, t.numel()))
        return view
    dX = put(X, _guard_x)
    didx = idx.to(DEV)
    dm, ds, dy, dUp, dVp, dbp = (put(t) for t in (mean, std, y, U, V, b))
    outs = [put(torch.zeros_like(t)) for t in (U, V, b)] if grad else [None] * 3
    loss = put(torch.zeros(2, dtype=torch.float64))
    need = ops.rrr_pixel_loss_grad_workspace_bytes(K, T, N, C, r)
    ws = torch.full((need // 8 + 2,), float("nan"), dtype=torch.float64, device=DEV)
    ops.rrr_pixel_loss_grad(dX, didx, dm, ds, dy, dUp, dVp, dbp, l2, loss, dU=outs[0], dV=outs[1], db=outs[2],
                            workspace=ws)
    torch.cuda.synchronize()
    for buf, numel in bufs:
        assert _margins_ok(buf, numel), "a margin was written"
    return (loss[0].cpu().clone(),) + tuple(o.cpu().clone() if o is not None else None for o in outs)


@pytest.mark.parametrize("xdtype", XDTYPES, ids=["u8", "f32"])
def test_pixel_stats_are_numpys_bit_for_bit(xdtype):
    """np.mean / np.std / np.clip(., 1e-8) over the trials, the same bits: K = 19 (odd sums), K = 1 (std 0, clipped),
    a constant column, a float32 video whose float32 sums round at every step."""
    from vspike import _lib, ops
    for K, F, C in ((19, 3, 33), (1, 2, 5), (33, 2, 257)):
        X = _video(K, F, C, xdtype, seed=3)
        mean, std = _np_stats(X)
        before = _lib.rrr_pixel_dispatch_counts()["rrr_pixel_stats"]
        (xbuf, xv) = _guard_x(X)
        (mbuf, mv), (sbuf, sv) = tw._guard(torch.zeros_like(torch.from_numpy(mean))), \
            tw._guard(torch.zeros_like(torch.from_numpy(std)))
        ops.rrr_pixel_stats(xv, mean=mv, std=sv)
        torch.cuda.synchronize()
        assert _lib.rrr_pixel_dispatch_counts()["rrr_pixel_stats"] == before + 1
        assert _margins_ok(xbuf, X.numel()) and tw._margins_nan(mbuf, mean.size) and tw._margins_nan(sbuf, std.size)
        gm, gs = mv.cpu(), sv.cpu()
        print(f"\nrrr pixel stats {xdtype} K {K}: mean differs in {int((gm.numpy() != mean).sum())}, std in "
              f"{int((gs.numpy() != std).sum())} of {mean.size}")
        assert gm.dtype == torch.from_numpy(mean).dtype
        assert tw._same_bits(gm, torch.from_numpy(mean)) and tw._same_bits(gs, torch.from_numpy(std))
        assert float(gs[0, 1 % C]) == np.float64(1e-8).astype(std.dtype)
        if K == 1:
            assert bool((gs == gs[0, 0]).all())
        # plain tensors, allocated by the wrapper: the same bits
        pm, ps = ops.rrr_pixel_stats(X.to(DEV))
        assert tw._same_bits(pm.cpu(), gm) and tw._same_bits(ps.cpu(), gs)


@pytest.mark.parametrize("ydtype", [torch.float32, torch.float64], ids=["y32", "y64"])
@pytest.mark.parametrize("xdtype", XDTYPES, ids=["u8", "f32"])
@pytest.mark.parametrize("shape,idx", SHAPES, ids=IDS)
def test_pixel_loss_grad_matches_float64_autograd(shape, idx, xdtype, ydtype):
    from vspike import _lib
    assert list(idx) != list(range(shape[2])) and len(set(idx)) < shape[1]
    l2 = 100.0
    X, ix, mean, std, Xs, y, U, V, b = _operands(shape, idx, xdtype, ydtype)
    Ur, Vr, br = (t.clone().requires_grad_(True) for t in (U, V, b))
    want = rr.loss(Xs, y, Ur, Vr, br, l2)
    want.backward()
    before = _lib.rrr_pixel_dispatch_counts()["rrr_pixel"]
    got = _call_loss_grad(X, ix, mean, std, y, U, V, b, l2)
    assert _lib.rrr_pixel_dispatch_counts()["rrr_pixel"] == before + 1
    want = want.detach()
    rel = abs(float(got[0]) - float(want)) / abs(float(want))
    errs = [float((g - w.grad).norm() / w.grad.norm()) for g, w in zip(got[1:], (Ur, Vr, br))]
    print(f"\nrrr pixel loss_grad {shape} {xdtype} {ydtype}: loss rel {rel:.2e}, dU {errs[0]:.2e}, dV {errs[1]:.2e}, "
          f"db {errs[2]:.2e}")
    assert rel <= 1e-12 and max(errs) <= 1e-12
    assert all(torch.isfinite(g).all() for g in got[1:])
    # a second guarded run, and a run on plain tensors with an untouched workspace: the same bits
    again = _call_loss_grad(X, ix, mean, std, y, U, V, b, l2)
    plain = _call_loss_grad(X, ix, mean, std, y, U, V, b, l2, guarded=False)
    for a, c, d in zip(got, again, plain):
        assert torch.equal(a, c) and torch.equal(a, d)
    # loss-only mode: the same loss, bit for bit
    only = _call_loss_grad(X, ix, mean, std, y, U, V, b, l2, grad=False)
    assert torch.equal(only[0], got[0])
    # l2 = 0 (the reference's mses_val): the plain squared error
    mse = _call_loss_grad(X, ix, mean, std, y, U, V, b, 0.0, grad=False)[0]
    want0 = float(rr.loss(Xs, y, U, V, b, 0.0))
    assert abs(float(mse) - want0) <= 1e-12 * want0


@pytest.mark.parametrize("xdtype", XDTYPES, ids=["u8", "f32"])
@pytest.mark.parametrize("shape,idx", SHAPES[:3], ids=IDS[:3])
def test_pixel_agrees_with_wide(shape, idx, xdtype):
    """C <= 1024 runs on both entries: the pixel entry on the video and vs_rrr_wide_loss_grad on the materialised
    float64 X agree to 1e-12; one call moves the pixel counter by one and the wide counter not at all."""
    from vspike import _lib
    X, ix, mean, std, Xs, y, U, V, b = _operands(shape, idx, xdtype, torch.float32, seed=2)
    before_p, before_w = _lib.rrr_pixel_dispatch_counts()["rrr_pixel"], _lib.rrr_dispatch_counts()["rrr_wide"]
    pix = _call_loss_grad(X, ix, mean, std, y, U, V, b, 100.0)
    assert _lib.rrr_pixel_dispatch_counts()["rrr_pixel"] == before_p + 1
    assert _lib.rrr_dispatch_counts()["rrr_wide"] == before_w
    wide = tw._call_loss_grad(Xs, y, U, V, b, 100.0)
    assert _lib.rrr_pixel_dispatch_counts()["rrr_pixel"] == before_p + 1
    rel = abs(float(pix[0]) - float(wide[0])) / abs(float(wide[0]))
    errs = [float((g - w).norm() / w.norm()) for g, w in zip(pix[1:], wide[1:])]
    print(f"\nrrr pixel vs wide {shape} {xdtype}: loss rel {rel:.2e}, dU {errs[0]:.2e}, dV {errs[1]:.2e}, "
          f"db {errs[2]:.2e}")
    assert rel <= 1e-12 and max(errs) <= 1e-12


@pytest.mark.parametrize("gtdtype", [torch.float32, torch.float64], ids=["gt32", "gt64"])
@pytest.mark.parametrize("xdtype", XDTYPES, ids=["u8", "f32"])
@pytest.mark.parametrize("shape,idx", SHAPES[:2] + SHAPES[3:], ids=IDS[:2] + IDS[3:])
def test_pixel_score_matches_the_restatement(shape, idx, xdtype, gtdtype):
    from vspike import ops
    K, F, T, N, C, r = shape
    X = _video(K, F, C, xdtype, seed=5)
    mean, std = _np_stats(X)
    Xs = _np_standardised(X, idx, mean, std)
    _, U, V, b, mean_y, std_y, gt = tw._score_inputs(K, T, N, C, r, gtdtype)
    want = rr.score(Xs.numpy(), U, V, b, mean_y.numpy(), std_y.numpy(), gt.numpy())
    assert (want["pred"] == 1e-3).any() and (want["pred"] > 1e-3).any()          # the clip is reached, not everywhere
    ix = torch.tensor(idx, dtype=torch.int64, device=DEV)
    runs = []
    for _ in range(2):
        xb = _guard_x(X)
        bufs = [tw._guard(t) for t in (torch.from_numpy(mean), torch.from_numpy(std), U, V, b, mean_y, std_y, gt)]
        outs = [tw._guard(torch.zeros(n, dtype=torch.float64)) for n in (K * T * N, N, N, 2)]
        ws = torch.full((ops.rrr_pixel_score_workspace_bytes(K, T, N) // 8 + 2,), float("nan"), dtype=torch.float64,
                        device=DEV)
        a = [v for _, v in bufs]
        ops.rrr_pixel_score(xb[1], ix, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], outs[1][1], outs[2][1],
                            outs[3][1], pred=outs[0][1].view(K, T, N), workspace=ws)
        torch.cuda.synchronize()
        assert _margins_ok(xb[0], X.numel()) and all(tw._margins_nan(buf, v.numel()) for buf, v in bufs + outs)
        runs.append([v.cpu().clone() for _, v in outs])
    pred, bps, r2, out = (t.numpy() for t in runs[0])
    assert all(tw._same_bits(p, q) for p, q in zip(*runs))
    e_pred = np.abs(pred.reshape(K, T, N) - want["pred"]).max()
    assert np.array_equal(np.isnan(bps), np.isnan(want["bps"])) and np.isnan(bps[0]) and not np.isnan(r2).any()
    e_bps = np.nanmax(np.abs(bps - want["bps"]))
    e_r2 = np.abs(r2 - want["r2"]).max()
    print(f"\nrrr pixel score {shape} {xdtype} {gtdtype}: pred {e_pred:.2e}, bps {e_bps:.2e}, r2 {e_r2:.2e}")
    assert e_pred <= 1e-12 and e_bps <= 1e-10 and e_r2 <= 1e-10
    assert r2[0] == 0.0                                                        # silent trials score exactly 0
    assert abs(out[0] - want["co_bps"]) <= 1e-10 and abs(out[1] - want["r2_mean"]) <= 1e-10


def test_binding_rejects_unsupported_sizes():
    from vspike import ops
    from vspike._lib import VsError
    X, ix, mean, std, _, y, U, V, b = (t.to(DEV) for t in _operands((3, 3, 2, 4, 40, 5), (0, 2), torch.uint8,
                                                                     torch.float32))
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    with pytest.raises(VsError, match="r <= 4"):
        ops.rrr_pixel_loss_grad(X, ix, mean, std, y, U, V, b, 1.0, loss)
    X, ix, mean, std, _, y, U, V, b = (t.to(DEV) for t in _operands((3, 3, 2, 4, 40, 2), (0, 2), torch.uint8,
                                                                     torch.float32))
    with pytest.raises(VsError, match="float64"):
        ops.rrr_pixel_loss_grad(X, ix, mean.float(), std.float(), y, U, V, b, 1.0, loss)
    with pytest.raises(VsError, match="uint8 / float32"):
        ops.rrr_pixel_loss_grad(X.double(), ix, mean, std, y, U, V, b, 1.0, loss)
    with pytest.raises(VsError, match="int64"):
        ops.rrr_pixel_loss_grad(X, ix.int(), mean, std, y, U, V, b, 1.0, loss)


# ---- the fit ---------------------------------------------------------------------------------------------------
# Distances to tests/golden/rrr_pixel.npz in the units of rrr_ref.distances (max |a - b| / max |b|; b against
# max |U V|; pred absolute).  Each bar is min(8 x the distance measured on MI355X, CAP x the spread the fixture
# records for the reference itself: its second run, fed the standardised training trials in another order).
#
#   prepare_rrr_inputs + RRRGD.fit + score on the uint8 frames     measured      reference's spread
#     losses                                                       1.74e-14      4.83e-12
#     U                                                            4.69e-12      1.35e-9
#     V                                                            1.01e-11      3.16e-9
#     b (against max |U V|)                                        3.69e-10      1.00e-3
#     r2                                                           1.22e-12      5.71e-7
#     pred                                                         7.27e-12      4.93e-6
#     bps                                                          8.17e-8       5.09e-7
#     co_bps                                                       1.17e-7       4.20e-7
#
# Every bar here is 8 x measured; the cap is 12 x .. 1e7 x further out.  b, bps and co_bps are the CPU restatement's
# own distances to the same digits (3.691e-10, 8.173e-8, 1.169e-7, tests/test_cpu_rrr_pixel.py): b's master copy is
# float32, and bps is the reference's float32 null model against the float64 one of the scoring kernels (the notes
# above FIT_MEASURED in tests/test_gpu_rrr_wide.py and tests/test_gpu_rrr.py).
FIT_MEASURED = {"losses": 1.74e-14, "U": 4.69e-12, "V": 1.01e-11, "b": 3.69e-10, "bps": 8.17e-8, "r2": 1.22e-12,
                "co_bps": 1.17e-7, "pred": 7.27e-12}
CAP = 100.0
MARGIN_OVER_MEASURED = 8.0


def _assert_within(d, s, what):
    for k, v in d.items():
        bar = min(MARGIN_OVER_MEASURED * FIT_MEASURED[k], CAP * s[k])
        assert v <= bar, (what, k, f"distance {v:.3e}", f"bar {bar:.3e}", f"spread {s[k]:.3e}")


def _fit(prepared=None):
    """prepare_rrr_inputs on the fixture's uint8 frames (or sessions already prepared), RRRGD.fit, score."""
    from vspike.rrr import PixelFeatures, RRRGD, prepare_rrr_inputs
    gt = None
    if prepared is None:
        prepared, gt = prepare_rrr_inputs(rp.make_raw(), rp.INPUT_MOD, idx=rp.frame_idx())
        gt = gt[rp.EID]
    p = prepared[rp.EID]
    assert all(isinstance(x, PixelFeatures) and x.X.dtype == torch.uint8 for x in p["X"])
    m = RRRGD(n_comp=3, l2=rr.L2).fit({rp.EID: (p["X"][0], p["y"][0])})
    out = {"losses": m.losses, "n_iter": m.n_iter, "func_evals": m.func_evals, "V": m.V.cpu().numpy(),
           "U": m.U(rp.EID).cpu().numpy(), "b": m.b(rp.EID).cpu().numpy()}
    if gt is not None:
        sc = m.score(rp.EID, p["X"][1], p["setup"]["mean_y_TN"], p["setup"]["std_y_TN"], gt)
        out.update({k: v.cpu().numpy() for k, v in sc.items()})
        assert float(m.mse({rp.EID: (p["X"][1], p["y"][1])})) > 0
    torch.cuda.synchronize()
    return out, prepared


def test_pixel_fit_follows_the_reference(fixture):
    """The fixture geometry (uint8 frames (K, F, 1, 25, 44), C = 1100) through prepare_rrr_inputs, RRRGD.fit and
    score: 20 iterations and 20 evaluations; losses, U, V, b, pred, bps, r2 and co_bps within the bars above; NaN
    bps only at the silent neuron; a second fit gives the same bits; train_rrr_baseline returns those scores under
    the reference's keys."""
    from vspike.rrr import train_rrr_baseline
    out, prepared = _fit()
    assert out["n_iter"] == 20 and out["func_evals"] == 20 and len(out["losses"]) == 20
    assert out["n_iter"] == fixture["X/n_iter"] and out["func_evals"] == fixture["X/func_evals"]
    d, s = rp.distances(out, fixture, label="gpu fit")
    _assert_within(d, s, "fit")
    assert np.flatnonzero(np.isnan(out["bps"])).tolist() == [rp.SILENT]
    out2, _ = _fit()
    for k in ("losses", "U", "V", "b", "bps", "r2", "pred"):
        assert np.array_equal(out[k], out2[k], equal_nan=True), k
    # the statistics are numpy's, and the video was neither converted nor copied per bin
    x0 = rp.flatten(rp.make_raw())[rp.EID]["X"][0]
    mean, std = rp.stats_u8(x0)
    setup = prepared[rp.EID]["setup"]
    assert np.array_equal(setup["mean_X_Tv"].cpu().numpy(), mean) and np.array_equal(setup["std_X_Tv"].cpu().numpy(), std)
    assert prepared[rp.EID]["X"][0].X.shape == (rp.K_TRAIN, rp.F, rp.C)
    # end to end: the reference's keys, the same scores, the inputs left as they were
    data = rp.make_raw()
    raw = [a.copy() for a in data[rp.EID]["X"]]
    res, mean_bps = train_rrr_baseline(data, rp.INPUT_MOD, idx=rp.frame_idx())
    r = res[rp.EID]
    assert set(r) == {"gt", "pred", "co_bps", "r2", "eid"} and r["eid"] == rp.EID
    assert all(np.array_equal(a, b_) and b_.dtype == np.uint8 for a, b_ in zip(raw, data[rp.EID]["X"]))
    assert np.array_equal(np.array(r["co_bps"]), out["bps"], equal_nan=True) and np.array_equal(r["pred"], out["pred"])
    assert np.array_equal(np.array(r["r2"]), out["r2"]) and mean_bps == float(out["co_bps"])


def test_pixel_features_with_precomputed_statistics_give_the_same_bits():
    """The uint8 frames through prepare_rrr_inputs (device statistics) and the same integer values through
    PixelFeatures built by hand from numpy's statistics: the same fit, bit for bit."""
    from vspike.rrr import PixelFeatures
    out, prepared = _fit()
    x0 = rp.flatten(rp.make_raw())[rp.EID]["X"][0]
    mean, std = rp.stats_u8(x0)
    feats = PixelFeatures(torch.from_numpy(x0).to(DEV), rp.frame_idx(), torch.from_numpy(mean).to(DEV),
                          torch.from_numpy(std).to(DEV))
    by_hand = {rp.EID: {"X": [feats, feats], "y": prepared[rp.EID]["y"], "setup": prepared[rp.EID]["setup"]}}
    out2, _ = _fit(by_hand)
    for k in ("losses", "U", "V", "b"):
        assert np.array_equal(out[k], out2[k]), k
    # and the float64 tensor it stands for is the reference's input
    want = rp.prepare()[0][rp.EID]["X"][0]
    assert np.array_equal(feats.materialise().cpu().numpy(), want)


def test_mixed_pixel_and_narrow_fit_is_the_rrrgd_fit():
    """joint = True fits a pixel and a narrow session in one RRRGD sharing V: the prepared inputs go to the very fit
    RRRGD runs on them, so the scores are the same bits; the pixel counter moves, once per closure and score."""
    import rrr_baseline_ref as rb
    from vspike import _lib
    from vspike.rrr import PixelFeatures, RRRGD, prepare_rrr_inputs, train_rrr_baseline
    idx = rp.frame_idx()
    narrow = rb.make_raw("M")["M0"]                                               # C = 5, T = 20 frames = bins
    data = dict(rp.make_raw())
    data["A"] = {"X": [x[:, :rp.F] for x in narrow["X"]], "y": [v[:, :rp.T] for v in narrow["y"]], "setup": {}}
    before = _lib.rrr_pixel_dispatch_counts()["rrr_pixel"]
    res, mean_bps = train_rrr_baseline(data, rp.INPUT_MOD, idx=idx, joint=True)
    assert _lib.rrr_pixel_dispatch_counts()["rrr_pixel"] == before + 20 + 1
    prepared, gt = prepare_rrr_inputs(data, rp.INPUT_MOD, idx=idx)
    assert list(prepared) == ["A", rp.EID]
    assert isinstance(prepared[rp.EID]["X"][0], PixelFeatures) and torch.is_tensor(prepared["A"]["X"][0])
    m = RRRGD().fit({eid: (p["X"][0], p["y"][0]) for eid, p in prepared.items()})
    assert m.n_iter == 20 and m.V.shape == (3, rp.T)
    bps = []
    for eid, p in prepared.items():
        sc = m.score(eid, p["X"][1], p["setup"]["mean_y_TN"], p["setup"]["std_y_TN"], gt[eid])
        assert np.array_equal(np.array(res[eid]["co_bps"]), sc["bps"].cpu().numpy(), equal_nan=True)
        assert np.array_equal(res[eid]["pred"], sc["pred"].cpu().numpy())
        bps.append(float(sc["co_bps"]))
    assert mean_bps == float(np.mean(bps))
    _, separate = train_rrr_baseline(data, rp.INPUT_MOD, idx=idx, joint=False)
    assert separate != mean_bps
