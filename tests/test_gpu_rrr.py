"""The reduced-rank regression validation on the GPU: vs_rrr_loss_grad, vs_rrr_score (csrc/rrr.hip), vspike.rrr
(RRR.fit, train_rrr) and ContrastTrainer.validate.

Kernel bars.  vs_rrr_loss_grad against float64 torch autograd on the CPU, same inputs: loss 1e-12 relative, each
gradient 1e-12 of its norm.  Measured on the CPU: another float64 summation order moves these by <= 4e-16, float32
accumulation by 5e-8 .. 3e-7, so 1e-12 passes any float64 order and fails any float32 shortcut.  vs_rrr_score
against tests/rrr_ref.py: pred 1e-12, bps and R^2 per neuron 1e-10, NaN positions equal, silent trials exactly 0.
Every operand sits in a larger allocation whose margins hold NaN and the workspace is pre-filled with NaN: the
results must be the bits of a run on plain tensors, and of a second run.

Fit bars: the table above FIT_MEASURED.
"""
import numpy as np
import pytest
import torch

import rrr_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 256
# (K, T, N, C, r): under one wave | N crosses a wave with a tail, the workload's T | two waves + a tail, minimal
# C and r | the caps
SHAPES = [(7, 5, 9, 3, 3), (33, 100, 70, 5, 3), (2, 3, 130, 1, 1), (3, 4, 64, 32, 8)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("rrr.npz")


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
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


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


def _call_loss_grad(X, y, U, V, b, l2, grad=True, guarded=True):
    """One vs_rrr_loss_grad call; with `guarded` every operand and output sits between NaN margins and the
    workspace starts as NaN.  Returns (loss, dU, dV, db) on the host."""
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
    need = ops.rrr_loss_grad_workspace_bytes(K, T, N, C)
    ws = torch.full((need // 8 + 2,), float("nan"), dtype=torch.float64, device=DEV)
    ops.rrr_loss_grad(dX, dy, dUp, dVp, dbp, l2, loss, dU=outs[0], dV=outs[1], db=outs[2], workspace=ws)
    torch.cuda.synchronize()
    for buf, numel in bufs:
        assert _margins_nan(buf, numel), "a margin was written"
    return (loss[0].cpu().clone(),) + tuple(o.cpu().clone() if o is not None else None for o in outs)


@pytest.mark.parametrize("ydtype", [torch.float32, torch.float64], ids=["y32", "y64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_grad_matches_float64_autograd(shape, ydtype):
    K, T, N, C, r = shape
    l2 = 100.0
    X, y, U, V, b = _inputs(K, T, N, C, r, ydtype)
    Ur, Vr, br = (t.clone().requires_grad_(True) for t in (U, V, b))
    want = rr.loss(X, y, Ur, Vr, br, l2)
    want.backward()
    got = _call_loss_grad(X, y, U, V, b, l2)
    rel = abs(float(got[0]) - float(want)) / abs(float(want))
    errs = [float((g - w.grad).norm() / w.grad.norm()) for g, w in zip(got[1:], (Ur, Vr, br))]
    print(f"\nrrr loss_grad {shape} {ydtype}: loss rel {rel:.2e}, dU {errs[0]:.2e}, dV {errs[1]:.2e}, db {errs[2]:.2e}")
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


def test_trial_split_over_blocks_is_ordered_and_exact():
    """A small grid (T ceil(N/64) < 512) with many trials splits the trials over several blocks per (t, neurons):
    the ordered partials give the same figures to 1e-12 and the same bits twice."""
    K, T, N, C, r = 70, 3, 9, 2, 2
    X, y, U, V, b = _inputs(K, T, N, C, r, torch.float32, seed=3)
    Ur, Vr, br = (t.clone().requires_grad_(True) for t in (U, V, b))
    want = rr.loss(X, y, Ur, Vr, br, 3.0)
    want.backward()
    got = _call_loss_grad(X, y, U, V, b, 3.0)
    assert abs(float(got[0]) - float(want)) <= 1e-12 * abs(float(want))
    for g, w in zip(got[1:], (Ur, Vr, br)):
        assert float((g - w.grad).norm() / w.grad.norm()) <= 1e-12
    again = _call_loss_grad(X, y, U, V, b, 3.0)
    assert all(torch.equal(a, c) for a, c in zip(got, again))


def test_binding_rejects_unsupported_sizes():
    from vspike import ops
    from vspike._lib import VsError
    X, y, U, V, b = (t.to(DEV) for t in _inputs(3, 4, 5, 33, 2, torch.float32))
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    with pytest.raises(VsError, match="C <= 32"):
        ops.rrr_loss_grad(X, y, U, V, b, 1.0, loss)
    X, y, U, V, b = (t.to(DEV) for t in _inputs(3, 4, 5, 2, 9, torch.float32))
    with pytest.raises(VsError, match="r <= 8"):
        ops.rrr_loss_grad(X, y, U, V, b, 1.0, loss)
    with pytest.raises(VsError, match="float64"):
        ops.rrr_loss_grad(X.float(), y, U, V, b, 1.0, loss)


def _score_inputs(K, T, N, C, r, gtdtype):
    g = torch.Generator().manual_seed(77 + N)
    X, _, U, V, _ = _inputs(K, T, N, C, r, torch.float32, seed=5)
    U = U * 8
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
def test_score_matches_the_restatement(shape, gtdtype):
    from vspike import ops
    K, T, N, C, r = shape
    X, U, V, b, mean_y, std_y, gt = _score_inputs(K, T, N, C, r, gtdtype)
    want = rr.score(X.numpy(), U, V, b, mean_y.numpy(), std_y.numpy(), gt.numpy())
    assert (want["pred"] == 1e-3).any() and (want["pred"] > 1e-3).any()          # the clip is reached, not everywhere
    runs = []
    for _ in range(2):
        bufs = [_guard(t) for t in (X, U, V, b, mean_y, std_y, gt)]
        outs = [_guard(torch.zeros(n, dtype=torch.float64)) for n in (K * T * N, N, N, 2)]
        ws = torch.full((ops.rrr_score_workspace_bytes(K, N) // 8 + 2,), float("nan"), dtype=torch.float64, device=DEV)
        a = [v for _, v in bufs]
        ops.rrr_score(a[0], a[1], a[2], a[3], a[4], a[5], a[6], outs[1][1], outs[2][1], outs[3][1],
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
    print(f"\nrrr score {shape} {gtdtype}: pred {e_pred:.2e}, bps {e_bps:.2e}, r2 {e_r2:.2e}")
    assert e_pred <= 1e-12 and e_bps <= 1e-10 and e_r2 <= 1e-10
    assert r2[0] == 0.0                                                        # silent trials score exactly 0
    assert abs(out[0] - want["co_bps"]) <= 1e-10 and abs(out[1] - want["r2_mean"]) <= 1e-10
    # without pred: the same scores
    outs2 = [torch.zeros(n, dtype=torch.float64, device=DEV) for n in (N, N, 2)]
    ops.rrr_score(*[t.to(DEV) for t in (X, U, V, b, mean_y, std_y, gt)], *outs2)
    assert all(_same_bits(o.cpu(), w) for o, w in zip(outs2, runs[0][1:]))


# ---- the fit ---------------------------------------------------------------------------------------------------
# Distances to tests/golden/rrr.npz in the units of rrr_ref.distances (max |a - b| / max |b|; b against max |U V|;
# pred absolute), measured on MI355X, the larger of geometries A and B.  Each bar is 8 x the measured distance (the
# project's usual margin over one run) and never more than CAP x the spread the fixture records for the reference
# itself (its second run, fed the standardised training trials in another order).
#
#   RRR.fit + score on the host-standardised arrays      measured    bar (A / B)           reference's spread (A / B)
#     losses                                             4.4e-15     3.5e-14               2.6e-9 / 7.1e-9
#     U                                                  1.3e-13     1.0e-12               1.7e-7 / 1.9e-7
#     V                                                  1.4e-13     1.1e-12               2.4e-7 / 2.0e-7
#     b (against max |U V|)                              1.7e-13     1.4e-12               1.8e-7 / 8.1e-8
#     r2                                                 2.0e-14     1.6e-13               1.9e-8 / 3.8e-8
#     pred (A only)                                      6.2e-14     5.0e-13               1.8e-7
#     bps                                                1.75e-7     2.2e-7 / 8.3e-7 (cap) 2.2e-9 / 8.3e-9
#     co_bps                                             3.6e-7      2.9e-6 / 2.4e-6 (cap) 3.9e-8 / 2.4e-8
#   train_rrr end to end (device standardisation)
#     bps, co_bps                                        as above (the same figures to three digits)
#     r2                                                 3.0e-14     2.4e-13
#     pred (A only)                                      7.4e-14     5.9e-13
#
# bps and co_bps sit at the cap, not at 8 x measured: their distance is not the fit's (pred agrees to 6e-14) but the
# reference's own float32 arithmetic.  Its held-out counts are float32, so `bits_per_spike` forms the null model's
# rates, their logarithms, gammaln and the sum of nll_null in float32 (metric_utils.py:97-101), a relative error
# of ~1e-7 that the float64 restatement on the CPU shows to the same digits (tests/test_cpu_rrr.py prints 1.745e-7
# and 6.531e-8).  vs_rrr_score computes the null model in float64, as the issue specifies; 79 x the spread at
# geometry A is that difference, under the 100 x cap.
# End to end was expected to be looser (the reference standardises y in float32); it is not, because
# vspike.rrr._std reproduces numpy's float32 statistics bit for bit (ascending sums, correctly rounded quotients).
CAP = 100.0            # no bar may exceed 100 x the reference's spread
MARGIN_OVER_MEASURED = 8.0
FIT_MEASURED = {"losses": 4.4e-15, "U": 1.3e-13, "V": 1.4e-13, "b": 1.7e-13, "bps": 1.75e-7, "r2": 2.0e-14,
                "co_bps": 3.6e-7, "pred": 6.2e-14}
E2E_MEASURED = {"bps": 1.75e-7, "r2": 3.0e-14, "co_bps": 3.6e-7, "pred": 7.4e-14}


def _fit(geom):
    from vspike.rrr import RRR
    g = rr.GEOMETRIES[geom]
    data = rr.make_data(geom)
    Xs, ys, mean_y, std_y = rr.standardise(data)
    m = RRR(n_comp=g["r"], l2=rr.L2).fit(torch.from_numpy(Xs[0]).to(DEV), torch.from_numpy(ys[0]).to(DEV))
    s = m.score(torch.from_numpy(Xs[1]).to(DEV), torch.from_numpy(mean_y).to(DEV), torch.from_numpy(std_y).to(DEV),
                torch.from_numpy(data["y"][1]).to(DEV))
    torch.cuda.synchronize()
    out = {"U": m.U.cpu().numpy(), "V": m.V.cpu().numpy(), "b": m.b.cpu().numpy(), "losses": m.losses,
           "n_iter": m.n_iter, "func_evals": m.func_evals}
    out.update({k: v.cpu().numpy() for k, v in s.items()})
    return out, m


def _assert_within(d, s, measured, what):
    for k, v in d.items():
        bar = min(MARGIN_OVER_MEASURED * measured[k], CAP * s[k])
        assert v <= bar, (what, k, f"distance {v:.3e}", f"bar {bar:.3e}", f"spread {s[k]:.3e}")


@pytest.mark.parametrize("geom", list(rr.GEOMETRIES))
def test_fit_and_scoring_follow_the_reference(fixture, geom):
    """RRR.fit + score on the host-standardised arrays (bitwise the reference's inputs) against the fixture: n_iter
    and func_evals equal, the 20 losses, U, V, b, pred, bps, r2 and co_bps within min(8 x measured, 100 x the
    reference's spread).  Measured on MI355X: losses 4.4e-15, U 1.3e-13, V 1.4e-13, b 1.7e-13, r2 2.0e-14, pred
    6.2e-14, bps 1.75e-7, co_bps 3.6e-7 (table and the reason for the last two above FIT_MEASURED)."""
    out, m = _fit(geom)
    assert out["n_iter"] == fixture[f"{geom}/n_iter"] and out["func_evals"] == fixture[f"{geom}/func_evals"]
    assert len(out["losses"]) == 20
    d, s = rr.distances(out, fixture, geom, label="gpu fit")
    _assert_within(d, s, FIT_MEASURED, geom)
    # a second fit: the same bits
    out2, _ = _fit(geom)
    for k in ("U", "V", "b", "losses", "bps", "r2", "pred"):
        assert np.array_equal(out[k], out2[k], equal_nan=True), k
    # mses_val (loss-only mode, l2 = 0) and the reference's state_dict layout
    sd = m.state_dict(geom)
    assert list(sd["model"]) == [f"{geom}_U", f"{geom}_b", "V"] and sd["n_comp"] == 3 and sd["l2"] == rr.L2
    Xs, ys, _, _ = rr.standardise(rr.make_data(geom))
    good = np.flatnonzero(np.arange(ys[1].shape[2]) != rr.SILENT_IN_TRAIN)   # its standardised validation y is ~1e8
    want = float(rr.loss(Xs[1], ys[1][:, :, good], out["U"][good], out["V"], out["b"][good], 0.0))
    Xv, yv = torch.from_numpy(Xs[1]).to(DEV), torch.from_numpy(np.ascontiguousarray(ys[1][:, :, good])).to(DEV)
    from vspike import ops
    sel = torch.from_numpy(good).to(DEV)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.rrr_loss_grad(Xv, yv, m.U.index_select(0, sel).contiguous(), m.V, m.b.index_select(0, sel).contiguous(), 0.0,
                      loss)
    assert abs(float(loss) - want) <= 1e-12 * want
    assert torch.isfinite(m.mse(Xv, torch.from_numpy(ys[1]).to(DEV)))


@pytest.mark.parametrize("geom", list(rr.GEOMETRIES))
@pytest.mark.parametrize("as_numpy", [True, False], ids=["numpy", "torch"])
def test_train_rrr_end_to_end(fixture, geom, as_numpy):
    """vspike.rrr.train_rrr (device standardisation, fit, scoring) on the raw inputs against the fixture's
    per-neuron lists and co_bps, within min(8 x measured, 100 x the reference's spread).  Measured on MI355X: r2
    3.0e-14, pred 7.4e-14, bps 1.75e-7, co_bps 3.6e-7 (table above FIT_MEASURED)."""
    from vspike.rrr import train_rrr
    data = rr.make_data(geom)
    raw = {k: [a.copy() for a in data[k]] for k in ("X", "y")}
    if not as_numpy:
        data = {"X": [torch.from_numpy(a).to(DEV) for a in data["X"]], "y": [torch.from_numpy(a) for a in data["y"]],
                "setup": {}}
    res = train_rrr({geom: data})[geom]
    assert set(res) == {"gt", "pred", "bps", "r2", "eid"} and res["eid"] == geom
    assert isinstance(res["bps"], list) and len(res["bps"]) == rr.GEOMETRIES[geom]["N"] == len(res["r2"])
    assert np.array_equal(res["gt"], raw["y"][1]) and res["pred"].dtype == np.float64
    if as_numpy:                                                       # the inputs are left as they were
        assert all(np.array_equal(a, b) for k in raw for a, b in zip(raw[k], data[k]))
    assert set(data["setup"]) == {"mean_X_Tv", "std_X_Tv", "mean_y_TN", "std_y_TN"}
    got = {"bps": np.array(res["bps"]), "r2": np.array(res["r2"]), "pred": res["pred"],
           "co_bps": np.nanmean(res["bps"])}
    d, s = rr.distances(got, fixture, geom, keys=("bps", "r2", "co_bps", "pred"), label="gpu train_rrr")
    _assert_within(d, s, E2E_MEASURED, geom)


# ---- ContrastTrainer.validate ----------------------------------------------------------------------------------
VAL = dict(train=6, val=4, F=6, T=5, N=9, E=3, image=32)


def _val_model():
    from vspike import ContrastViT
    torch.manual_seed(5)
    cfg = {"model_class": "ContrastViT", "compute_dtype": "fp32", "fix_temp": True, "image_size": VAL["image"],
           "patch_size": 16, "num_channels": 1, "hidden_size": 64, "num_hidden_layers": 1, "num_attention_heads": 1,
           "intermediate_size": 128, "layer_norm_eps": 1e-12, "embed_size": VAL["E"], "mask_ratio": 0.75,
           "decoder_hidden_size": 512}
    return ContrastViT(cfg).to(DEV)


def _val_batches(n_trials, seed, five_d):
    """One batch per trial, as the reference's loaders give them: 'ref' (F, 1, H, W), or 5-D with a leading 1."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_trials):
        ref = torch.rand(VAL["F"], 1, VAL["image"], VAL["image"], generator=g)
        lam = 0.3 + 1.5 * ref.mean((1, 2, 3))[:VAL["T"], None] * torch.rand(1, VAL["N"], generator=g)
        neural = torch.poisson(lam.expand(VAL["T"], VAL["N"]), generator=g)
        neural[:, 0] = 0
        out.append({"ref": (ref[None] if five_d else ref).to(DEV), "neural": neural[None].to(DEV)})
    return out


def test_validate_is_the_restatement_on_the_plugins_embeddings():
    """The glue of ContrastTrainer.validate (loader dict forms, reshape, frame index, mode restored) by equality with
    tests/rrr_ref.py run on the plugin's own z.  Measured on MI355X: val_bps 7.5e-14 from the restatement's, whose
    own spread on this problem is 7.1e-9 (bar: 100 x that spread)."""
    from vspike.trainer import ContrastTrainer
    m = _val_model()
    m.train()
    tr = ContrastTrainer(m, optimizer=None)
    train_b, val_b = _val_batches(VAL["train"], 1, five_d=True), _val_batches(VAL["val"], 2, five_d=False)
    idx = np.array([0, 1, 3, 4, 5])
    res = tr.validate(train_b, val_b, idx=idx)
    assert set(res) == {"val_bps"} and isinstance(res["val_bps"], float) and m.training
    # the restatement on the plugin's own z
    z = [tr.transform([b["ref"].squeeze(0) if b["ref"].dim() == 5 else b["ref"] for b in bs]) for bs in (train_b, val_b)]
    X = [t.view(-1, VAL["F"], VAL["E"])[:, idx].cpu().numpy() for t in z]
    y = [torch.cat([b["neural"] for b in bs]).cpu().numpy() for bs in (train_b, val_b)]
    assert X[0].shape == (VAL["train"], VAL["T"], VAL["E"]) and X[0].dtype == np.float32
    # the reference standardises the float32 embeddings in float32, then the bias column makes X float64
    Xs, ys, mean_y, std_y = rr.standardise({"X": X, "y": y})
    assert Xs[0].dtype == np.float64 and ys[0].dtype == np.float32
    fit = rr.fit(Xs[0], ys[0], 3, rr.L2)
    want = rr.score(Xs[1], fit["U"], fit["V"], fit["b"], mean_y, std_y, y[1])
    # the bar is the restatement's own spread on this very problem, as for the fixture: the same fit with the
    # standardised training trials in another order, x 100 (floor: 1e-12, float64 rounding of the scoring)
    perm = np.array([3, 0, 5, 1, 4, 2])
    fit2 = rr.fit(Xs[0][perm], ys[0][perm], 3, rr.L2)
    want2 = rr.score(Xs[1], fit2["U"], fit2["V"], fit2["b"], mean_y, std_y, y[1])
    spread = abs(want2["co_bps"] - want["co_bps"]) / abs(want["co_bps"])
    d = abs(res["val_bps"] - want["co_bps"]) / abs(want["co_bps"])
    print(f"\nrrr validate: val_bps {res['val_bps']:.12g}, restatement {want['co_bps']:.12g}, distance {d:.3e}, "
          f"restatement's spread {spread:.3e}")
    assert d <= max(100.0 * spread, 1e-12)
    # another frame selection gives another number: idx is used
    other = tr.validate(train_b, val_b, idx=np.array([0, 1, 2, 3, 4]))
    assert abs(other["val_bps"] - res["val_bps"]) > 1e-6 * abs(res["val_bps"])
    with pytest.raises(ValueError, match="frame indices"):
        tr.validate(train_b, val_b, idx=np.array([0, 1, 2]))


def test_validate_default_draw_is_the_references():
    """idx = None draws sort(choice(F - 1, T, replace=False)) from numpy's global generator, as contrast.py:141
    does with (119, 100): the result equals the explicit call with that draw, and the generator has advanced."""
    from vspike.trainer import ContrastTrainer
    tr = ContrastTrainer(_val_model(), optimizer=None)
    train_b, val_b = _val_batches(VAL["train"], 1, five_d=False), _val_batches(VAL["val"], 2, five_d=False)
    np.random.seed(11)
    idx = np.sort(np.random.choice(VAL["F"] - 1, VAL["T"], replace=False))
    after = np.random.rand()
    assert idx.max() < VAL["F"] - 1                                     # the last frame is never used
    want = tr.validate(train_b, val_b, idx=idx)
    np.random.seed(11)
    got = tr.validate(train_b, val_b)
    assert got == want and np.random.rand() == after
