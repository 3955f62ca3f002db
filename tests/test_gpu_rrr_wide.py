"""The RRR baseline on the GPU: vs_rrr_wide_loss_grad, vs_rrr_wide_score, vs_gauss_smooth_time (csrc/rrr_wide.hip)
and vspike.rrr's RRRGD, prepare_rrr_inputs and train_rrr_baseline.

Kernel bars are those of tests/test_gpu_rrr.py.  vs_rrr_wide_loss_grad against float64 torch autograd on the CPU,
same inputs: loss 1e-12 relative, each gradient 1e-12 of its norm.  Measured on the CPU at the four shapes below:
permuting trials, features and neurons moves these by <= 6e-16, forming the product from float32-rounded operands
moves yhat by 1e-7 .. 3e-7, so 1e-12 passes any float64 order and fails any float32 shortcut.  vs_rrr_wide_score
against tests/rrr_ref.py: pred 1e-12, bps and R^2 per neuron 1e-10, NaN positions equal, silent trials exactly 0.
vs_gauss_smooth_time against scipy's outputs stored in the fixture: the same bits.
Every operand sits in a larger allocation whose margins hold NaN and the workspace is pre-filled with NaN: the
results must be the bits of a run on plain tensors, and of a second run.

Fit bars: the table above FIT_MEASURED.
"""
import numpy as np
import pytest
import torch

import rrr_baseline_ref as rb
import rrr_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 256
# (K, T, N, C, r): the first C over the narrow cap, C + 1 = 34 no multiple of 4, under one MFMA tile in K and N |
# N crosses 64 and K crosses 16, both with tails | two neuron tiles + a tail, r at its cap, C + 1 = 258 |
# C at its cap, K under one MFMA k-step
SHAPES = [(5, 3, 9, 33, 2), (19, 4, 70, 100, 3), (33, 2, 130, 257, 8), (3, 2, 17, 1024, 1)]
NARROW_SHAPES = [(33, 100, 70, 5, 3), (3, 4, 64, 32, 8)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("rrr_baseline.npz")


def _guard(t):
    """A copy of t inside a larger allocation whose margins hold NaN: (buffer, view)."""
    t = t.contiguous()
    pad = MARGIN * 8 // t.element_size()
    buf = torch.full((t.numel() + 2 * pad,), float("nan"), dtype=t.dtype, device=DEV)
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _same_bits(a, b):
    """torch.equal on the bit patterns (NaN equals NaN)."""
    it = torch.int64 if a.element_size() == 8 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _margins_nan(buf, numel):
    pad = (buf.numel() - numel) // 2
    return bool(torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + numel:]).all())


def _inputs(K, T, N, C, r, ydtype, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + K * 131 + N)
    X = torch.randn(K, T, C + 1, generator=g, dtype=torch.float64)
    X[:, :, C] = 1.0
    y = torch.randn(K, T, N, generator=g, dtype=torch.float64).to(ydtype)
    U = torch.randn(N, C, r, generator=g, dtype=torch.float64) / (T * r) ** 0.5
    V = torch.randn(r, T, generator=g, dtype=torch.float64) / (T * r) ** 0.5
    b = 0.3 * torch.randn(N, 1, T, generator=g, dtype=torch.float64)            # non-zero: the b^2 term counts
    return X, y, U, V, b


def _call_loss_grad(X, y, U, V, b, l2, grad=True, guarded=True, wide=True):
    """One vs_rrr_wide_loss_grad (or, wide = False, vs_rrr_loss_grad) call; with `guarded` every operand and output
    sits between NaN margins and the workspace starts as NaN.  Returns (loss, dU, dV, db) on the host."""
    from vspike import ops
    K, T, N = y.shape
    C = X.shape[2] - 1
    bufs = []

    def put(t):
        if not guarded:
            return t.to(DEV).contiguous()
        buf, view = _guard(t)
        bufs.append((buf, t.numel()))
        return view
    dX, dy, dUp, dVp, dbp = (put(t) for t in (X, y, U, V, b))
    outs = [put(torch.zeros_like(t)) for t in (U, V, b)] if grad else [None] * 3
    loss = put(torch.zeros(2, dtype=torch.float64))
    need = (ops.rrr_wide_loss_grad_workspace_bytes if wide else ops.rrr_loss_grad_workspace_bytes)(K, T, N, C)
    ws = torch.full((need // 8 + 2,), float("nan"), dtype=torch.float64, device=DEV)
    fn = ops.rrr_wide_loss_grad if wide else ops.rrr_loss_grad
    fn(dX, dy, dUp, dVp, dbp, l2, loss, dU=outs[0], dV=outs[1], db=outs[2], workspace=ws)
    torch.cuda.synchronize()
    for buf, numel in bufs:
        assert _margins_nan(buf, numel), "a margin was written"
    return (loss[0].cpu().clone(),) + tuple(o.cpu().clone() if o is not None else None for o in outs)


@pytest.mark.parametrize("ydtype", [torch.float32, torch.float64], ids=["y32", "y64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wide_loss_grad_matches_float64_autograd(shape, ydtype):
    from vspike import _lib
    K, T, N, C, r = shape
    l2 = 100.0
    X, y, U, V, b = _inputs(K, T, N, C, r, ydtype)
    Ur, Vr, br = (t.clone().requires_grad_(True) for t in (U, V, b))
    want = rr.loss(X, y, Ur, Vr, br, l2)
    want.backward()
    before = _lib.rrr_dispatch_counts()["rrr_wide"]
    got = _call_loss_grad(X, y, U, V, b, l2)
    assert _lib.rrr_dispatch_counts()["rrr_wide"] == before + 1
    rel = abs(float(got[0]) - float(want)) / abs(float(want))
    errs = [float((g - w.grad).norm() / w.grad.norm()) for g, w in zip(got[1:], (Ur, Vr, br))]
    print(f"\nrrr wide loss_grad {shape} {ydtype}: loss rel {rel:.2e}, dU {errs[0]:.2e}, dV {errs[1]:.2e}, "
          f"db {errs[2]:.2e}")
    assert rel <= 1e-12 and max(errs) <= 1e-12
    assert all(torch.isfinite(g).all() for g in got[1:])
    # a second guarded run, and a run on plain tensors with an untouched workspace: the same bits
    again = _call_loss_grad(X, y, U, V, b, l2)
    plain = _call_loss_grad(X, y, U, V, b, l2, guarded=False)
    for a, c, d in zip(got, again, plain):
        assert torch.equal(a, c) and torch.equal(a, d)
    # loss-only mode: the same loss, bit for bit
    only = _call_loss_grad(X, y, U, V, b, l2, grad=False)
    assert torch.equal(only[0], got[0])
    # l2 = 0 (the reference's mses_val): the plain squared error
    mse = _call_loss_grad(X, y, U, V, b, 0.0, grad=False)[0]
    want0 = float(rr.loss(X, y, U, V, b, 0.0))
    assert abs(float(mse) - want0) <= 1e-12 * want0


@pytest.mark.parametrize("shape", NARROW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wide_agrees_with_narrow(shape):
    """C <= 32 runs on both entries: the MFMA products and the register kernel agree to 1e-12."""
    K, T, N, C, r = shape
    X, y, U, V, b = _inputs(K, T, N, C, r, torch.float32, seed=2)
    wide = _call_loss_grad(X, y, U, V, b, 100.0)
    narrow = _call_loss_grad(X, y, U, V, b, 100.0, wide=False)
    rel = abs(float(wide[0]) - float(narrow[0])) / abs(float(narrow[0]))
    errs = [float((g - w).norm() / w.norm()) for g, w in zip(wide[1:], narrow[1:])]
    print(f"\nrrr wide vs narrow {shape}: loss rel {rel:.2e}, dU {errs[0]:.2e}, dV {errs[1]:.2e}, db {errs[2]:.2e}")
    assert rel <= 1e-12 and max(errs) <= 1e-12


def test_binding_rejects_unsupported_sizes():
    from vspike import ops
    from vspike._lib import VsError
    X, y, U, V, b = (t.to(DEV) for t in _inputs(2, 2, 3, 1025, 2, torch.float32))
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    with pytest.raises(VsError, match="C <= 1024"):
        ops.rrr_wide_loss_grad(X, y, U, V, b, 1.0, loss)
    X, y, U, V, b = (t.to(DEV) for t in _inputs(3, 4, 5, 40, 9, torch.float32))
    with pytest.raises(VsError, match="r <= 8"):
        ops.rrr_wide_loss_grad(X, y, U, V, b, 1.0, loss)
    with pytest.raises(VsError, match="float64"):
        ops.rrr_wide_loss_grad(X.float(), y, U, V, b, 1.0, loss)
    with pytest.raises(VsError, match="radius"):
        ops.gauss_smooth_time(torch.zeros(2, 8, 3, device=DEV), 2)


def _score_inputs(K, T, N, C, r, gtdtype):
    g = torch.Generator().manual_seed(77 + N)
    X, _, U, V, _ = _inputs(K, T, N, C, r, torch.float32, seed=5)
    U = U * 8 / (C / 4.0) ** 0.5                  # yhat of order 1 whatever C, so that the clip is reached, not everywhere
    b = 0.2 * torch.randn(N, 1, T, generator=g, dtype=torch.float64)
    mean_y = 0.6 * torch.rand(T, N, generator=g, dtype=torch.float64) - 0.05
    std_y = 0.1 + torch.rand(T, N, generator=g, dtype=torch.float64)
    gt = torch.poisson(0.7 * torch.ones(K, T, N), generator=g)
    gt[:, :, 0] = 0                       # a silent neuron: NaN bps, R^2 exactly 0 in every trial
    gt[0, :, 1] = 0                       # a silent trial of an active neuron
    gt[:, :, 2] = 0
    gt[K - 1, T - 1, 2] = 3               # one spike train in one trial only
    std_y[:, 2] = 1e-8                    # the clipped standard deviation: pred = mean_y
    return X, U, V, b, mean_y, std_y, gt.to(gtdtype)


@pytest.mark.parametrize("gtdtype", [torch.float32, torch.float64], ids=["gt32", "gt64"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_wide_score_matches_the_restatement(shape, gtdtype):
    from vspike import ops
    K, T, N, C, r = shape
    X, U, V, b, mean_y, std_y, gt = _score_inputs(K, T, N, C, r, gtdtype)
    want = rr.score(X.numpy(), U, V, b, mean_y.numpy(), std_y.numpy(), gt.numpy())
    assert (want["pred"] == 1e-3).any() and (want["pred"] > 1e-3).any()          # the clip is reached, not everywhere
    runs = []
    for _ in range(2):
        bufs = [_guard(t) for t in (X, U, V, b, mean_y, std_y, gt)]
        outs = [_guard(torch.zeros(n, dtype=torch.float64)) for n in (K * T * N, N, N, 2)]
        ws = torch.full((ops.rrr_wide_score_workspace_bytes(K, T, N) // 8 + 2,), float("nan"), dtype=torch.float64,
                        device=DEV)
        a = [v for _, v in bufs]
        ops.rrr_wide_score(a[0], a[1], a[2], a[3], a[4], a[5], a[6], outs[1][1], outs[2][1], outs[3][1],
                           pred=outs[0][1].view(K, T, N), workspace=ws)
        torch.cuda.synchronize()
        assert all(_margins_nan(buf, v.numel()) for buf, v in bufs + outs)
        runs.append([v.cpu().clone() for _, v in outs])
    pred, bps, r2, out = (t.numpy() for t in runs[0])
    assert all(_same_bits(p, q) for p, q in zip(*runs))
    e_pred = np.abs(pred.reshape(K, T, N) - want["pred"]).max()
    assert np.array_equal(np.isnan(bps), np.isnan(want["bps"])) and np.isnan(bps[0]) and not np.isnan(r2).any()
    e_bps = np.nanmax(np.abs(bps - want["bps"]))
    e_r2 = np.abs(r2 - want["r2"]).max()
    print(f"\nrrr wide score {shape} {gtdtype}: pred {e_pred:.2e}, bps {e_bps:.2e}, r2 {e_r2:.2e}")
    assert e_pred <= 1e-12 and e_bps <= 1e-10 and e_r2 <= 1e-10
    assert r2[0] == 0.0                                                        # silent trials score exactly 0
    assert abs(out[0] - want["co_bps"]) <= 1e-10 and abs(out[1] - want["r2_mean"]) <= 1e-10
    # without pred: the same scores
    outs2 = [torch.zeros(n, dtype=torch.float64, device=DEV) for n in (N, N, 2)]
    ops.rrr_wide_score(*[t.to(DEV) for t in (X, U, V, b, mean_y, std_y, gt)], *outs2)
    assert all(_same_bits(o.cpu(), w) for o, w in zip(outs2, runs[0][1:]))


@pytest.mark.parametrize("name", list(rb.SMOOTH_INPUTS))
def test_gauss_smooth_time_is_scipy_bit_for_bit(fixture, name):
    """The fixture's scipy.ndimage.gaussian_filter1d(y, 2, axis=1) outputs, bit for bit, from plain tensors and
    from inside NaN margins.  Different bits mean contraction (an FMA) or another order of additions."""
    from vspike import _lib, ops
    y = torch.from_numpy(rb.smooth_input(name))
    want = torch.from_numpy(fixture[f"smooth/{name}"])
    assert want.dtype == y.dtype and want.shape == y.shape
    before = _lib.rrr_dispatch_counts()["gauss_smooth"]
    got = ops.gauss_smooth_time(y.to(DEV), rb.SMOOTH_W).cpu()
    assert _lib.rrr_dispatch_counts()["gauss_smooth"] == before + 1
    differ = int((got != want).sum())
    print(f"\ngauss_smooth_time {name}: {differ} of {want.numel()} elements differ from scipy's")
    assert _same_bits(got, want)
    (ybuf, yv), (obuf, ov) = _guard(y), _guard(torch.zeros_like(y))
    ops.gauss_smooth_time(yv, rb.SMOOTH_W, out=ov)
    torch.cuda.synchronize()
    assert _margins_nan(ybuf, y.numel()) and _margins_nan(obuf, y.numel())
    assert _same_bits(ov.cpu(), want)


# ---- the fits --------------------------------------------------------------------------------------------------
# Distances to tests/golden/rrr_baseline.npz in the units of rrr_ref.distances (max |a - b| / max |b|; b against
# max |U V|; pred absolute), measured on MI355X (run named in profiles/rrr_wide_tests.txt), the largest over the
# sessions of a geometry.  Each bar is 8 x the measured distance (the project's usual margin over one run) and
# never more than CAP x the spread the fixture records for the reference itself (its second run, fed the
# standardised training trials of every session in another order).  The cap is the binding condition.
#
#   RRRGD.fit + score on the host-standardised arrays   measured (W / M)      reference's spread (W / M)
#     losses                                            6.3e-13 / 3.2e-13     3.3e-9 / 9.5e-10
#     U (largest over the sessions)                     3.8e-14 / 1.1e-13     2.4e-10 / 4.9e-10
#     V                                                 3.8e-13 / 1.5e-13     1.2e-9 / 5.9e-10
#     b (against max |U V|)                             1.3e-8 / 5.8e-11      4.8e-4 / 3.3e-5
#     r2                                                2.6e-11 / 1.2e-12     2.6e-6 / 1.0e-6
#     pred (W only)                                     4.3e-10               2.4e-5
#     bps                                               9.4e-8 / 9.0e-8       8.3e-7 / 1.1e-7
#     co_bps                                            2.4e-8 / 2.0e-8       4.7e-7 / 6.6e-8
#   train_rrr_baseline end to end on P (device smoothing, one-hot, standardisation)
#     bps 7.96e-8, r2 2.0e-13, co_bps 1.24e-8           spread 8.7e-8, 1.8e-7, 8.5e-8
#
# Every bar here is 8 x measured: the cap is 12 x .. 1e6 x further out.  b, r2 and pred of W are the CPU
# restatement's own distances to the same digits (1.298e-8, 2.7e-11, 4.4e-10, tests/test_cpu_rrr_baseline.py): b's
# master copy is float32, so its last step is rounded to 6e-8 of its own size, and the scores inherit that.  bps and
# co_bps are the reference's float32 null model against the float64 one of vs_rrr_score / vs_rrr_wide_score (the
# note above FIT_MEASURED in tests/test_gpu_rrr.py), again the restatement's figures (9.394e-8, 9.011e-8, 7.957e-8).
FIT_MEASURED = {"W": {"losses": 6.3e-13, "U": 3.8e-14, "V": 3.8e-13, "b": 1.3e-8, "bps": 9.4e-8, "r2": 2.6e-11,
                      "co_bps": 2.4e-8, "pred": 4.3e-10},
                "M": {"losses": 3.2e-13, "U": 1.1e-13, "V": 1.5e-13, "b": 5.8e-11, "bps": 9.0e-8, "r2": 1.2e-12,
                      "co_bps": 2.0e-8}}
E2E_MEASURED = {"bps": 7.96e-8, "r2": 2.0e-13, "co_bps": 1.24e-8}
CAP = 100.0            # no bar may exceed 100 x the reference's spread
MARGIN_OVER_MEASURED = 8.0


def _assert_within(d, s, measured, what):
    for k, v in d.items():
        bar = min(MARGIN_OVER_MEASURED * measured[k], CAP * s[k])
        assert v <= bar, (what, k, f"distance {v:.3e}", f"bar {bar:.3e}", f"spread {s[k]:.3e}")


def _fit(geom):
    """RRRGD on a geometry's host-standardised sessions, then the scores per session."""
    from vspike.rrr import RRRGD
    sessions = rb.standardised(geom)
    m = RRRGD(n_comp=rb.N_COMP, l2=rr.L2).fit(
        {eid: (torch.from_numpy(s["X"][0]).to(DEV), torch.from_numpy(s["y"][0]).to(DEV)) for eid, s in sessions.items()})
    out = {"losses": m.losses, "n_iter": m.n_iter, "func_evals": m.func_evals, "V": m.V.cpu().numpy()}
    for eid, s in sessions.items():
        sc = m.score(eid, torch.from_numpy(s["X"][1]).to(DEV), torch.from_numpy(s["mean_y"]).to(DEV),
                     torch.from_numpy(s["std_y"]).to(DEV), torch.from_numpy(s["gt"]).to(DEV))
        out[eid] = {"U": m.U(eid).cpu().numpy(), "b": m.b(eid).cpu().numpy()}
        out[eid].update({k: v.cpu().numpy() for k, v in sc.items()})
    torch.cuda.synchronize()
    return out, m


@pytest.mark.parametrize("geom", ["W", "M"])
def test_rrrgd_fit_and_scoring_follow_the_reference(fixture, geom):
    """RRRGD.fit + score on the host-standardised arrays (bitwise the reference's inputs) against the fixture:
    n_iter and func_evals equal, the 20 losses, every session's U, b, pred, bps, r2, co_bps and the shared V within
    min(8 x measured, 100 x the reference's spread).  Measured figures: the table above FIT_MEASURED."""
    out, m = _fit(geom)
    assert out["n_iter"] == fixture[f"{geom}/n_iter"] and out["func_evals"] == fixture[f"{geom}/func_evals"]
    assert len(out["losses"]) == 20
    d, s = rb.distances(out, fixture, geom, label="gpu fit")
    _assert_within(d, s, FIT_MEASURED[geom], geom)
    # a second fit: the same bits
    out2, _ = _fit(geom)
    assert np.array_equal(out["losses"], out2["losses"]) and np.array_equal(out["V"], out2["V"])
    for eid in rb.GEOMETRIES[geom]["sessions"]:
        for k in ("U", "b", "bps", "r2", "pred"):
            assert np.array_equal(out[eid][k], out2[eid][k], equal_nan=True), (eid, k)
    sd = m.state_dict()
    eids = list(rb.GEOMETRIES[geom]["sessions"])
    assert list(sd["model"]) == [f"{e}_{p}" for e in eids for p in ("U", "b")] + ["V"]
    assert sd["eids"] == eids and sd["n_comp"] == 3 and sd["l2"] == rr.L2 and sd["T"] == rb.T
    assert sd["N"] == sum(g["N"] for g in rb.GEOMETRIES[geom]["sessions"].values())
    sessions = rb.standardised(geom)
    val = {eid: (torch.from_numpy(s_["X"][1]).to(DEV), torch.from_numpy(s_["y"][1]).to(DEV))
           for eid, s_ in sessions.items()}
    assert float(m.mse(val)) > 0


def test_train_rrr_baseline_end_to_end(fixture):
    """vspike.rrr.train_rrr_baseline on geometry P's raw inputs (smoothing, one-hot choice / block, device
    standardisation, frame selection, fit, scoring) against the fixture, within min(8 x measured, 100 x the
    reference's spread); the inputs are left as they were."""
    from vspike.rrr import train_rrr_baseline
    data = rb.make_raw("P")
    raw = {k: [a.copy() for a in data["P"][k]] for k in ("X", "y")}
    res, mean_bps = train_rrr_baseline(data, rb.GEOMETRIES["P"]["input_mod"], idx=rb.frame_idx("P"))
    r = res["P"]
    assert set(r) == {"gt", "pred", "co_bps", "r2", "eid"} and r["eid"] == "P"
    assert all(np.array_equal(a, b_) for k in raw for a, b_ in zip(raw[k], data["P"][k]))
    assert np.array_equal(r["gt"], raw["y"][1]) and r["pred"].dtype == np.float64
    assert set(data["P"]["setup"]) == {"mean_X_Tv", "std_X_Tv", "mean_y_TN", "std_y_TN"}
    got = {"P": {"bps": np.array(r["co_bps"]), "r2": np.array(r["r2"]), "co_bps": np.nanmean(r["co_bps"])}}
    assert abs(mean_bps - got["P"]["co_bps"]) <= 1e-12 * abs(mean_bps)
    d, s = rb.distances(got, fixture, "P", keys=("bps", "r2", "co_bps"), label="gpu train_rrr_baseline")
    _assert_within(d, s, E2E_MEASURED, "P")
    # the default frame draw is the reference's: numpy's global generator, sort(choice(F - 1, T))
    np.random.seed(rb.GEOMETRIES["P"]["idx_seed"])
    res2, mean2 = train_rrr_baseline(rb.make_raw("P"), rb.GEOMETRIES["P"]["input_mod"])
    assert mean2 == mean_bps and np.array_equal(res2["P"]["co_bps"], r["co_bps"], equal_nan=True)


def test_joint_fit_is_the_rrrgd_fit():
    """joint = True fits all sessions in one RRRGD: with the behaviour left alone ('me': no one-hot) the prepared
    inputs go to the very fit RRRGD runs on them, so the scores are the same bits; joint = False gives another
    model (each session its own V)."""
    from vspike.rrr import RRRGD, prepare_rrr_inputs, train_rrr_baseline
    data, idx = rb.make_raw("M"), rb.frame_idx("M")
    res, mean_bps = train_rrr_baseline(data, "me", idx=idx, joint=True)
    prepared, gt = prepare_rrr_inputs(data, "me", idx=idx)
    m = RRRGD().fit({eid: (p["X"][0], p["y"][0]) for eid, p in prepared.items()})
    assert list(prepared) == sorted(data) and m.n_iter == 20
    bps = []
    for eid, p in prepared.items():
        s = m.score(eid, p["X"][1], p["setup"]["mean_y_TN"], p["setup"]["std_y_TN"], gt[eid])
        assert np.array_equal(np.array(res[eid]["co_bps"]), s["bps"].cpu().numpy(), equal_nan=True)
        assert np.array_equal(res[eid]["pred"], s["pred"].cpu().numpy())
        bps.append(float(s["co_bps"]))
    assert mean_bps == float(np.mean(bps))
    _, separate = train_rrr_baseline(data, "me", idx=idx, joint=False)
    assert separate != mean_bps
