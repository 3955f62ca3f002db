"""The masked-autoencoder kernels of csrc/mae.hip, each alone against torch indexing.

The gathers copy f32 values (or round them once to bf16), so they must equal torch's indexing bit for bit; the
in-order sums and the loss are compared with float64 sums at 1e-6 relative (f32 sums of at most a few hundred
terms; the loss itself is accumulated in f64 and rounded once).  Cases: one kept patch, every patch kept, the
fixture geometries (9 patches / 2 kept, 81 / 32) and a channel count that is not a multiple of the 256-lane block.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (G, P, Lk, D)
CASES = [(4, 9, 2, 64), (3, 81, 32, 96), (2, 9, 1, 128), (2, 9, 9, 64), (5, 16, 7, 520)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ids(G, P, Lk, seed):
    g = torch.Generator().manual_seed(seed)
    noise = torch.rand(G, P, generator=g)
    shuffle = torch.argsort(noise, dim=1)
    restore = torch.argsort(shuffle, dim=1)
    return shuffle[:, :Lk].contiguous(), restore


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _i32(t):
    return t.to(torch.int32).to(DEV).contiguous()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_mae_embed_fwd_bwd(case):
    from vspike import ops
    G, P, Lk, D = case
    keep, restore = _ids(G, P, Lk, 3)
    patches, cls, table = _rand(G * P, D, seed=4), _rand(D, seed=5), _rand(P + 1, D, seed=6)
    x0 = torch.full((G, Lk + 1, D), float("nan"), device=DEV)
    ops.mae_embed_fwd(patches.to(DEV), _i32(keep), cls.to(DEV), table.to(DEV), x0)
    ref = torch.cat([(cls + table[0]).expand(G, 1, D),
                     torch.gather(patches.view(G, P, D), 1, keep[:, :, None].expand(G, Lk, D))], dim=1)
    assert torch.equal(x0.cpu(), ref)
    dx = _rand(G, Lk + 1, D, seed=7)
    mask = restore >= Lk
    ref_dp = torch.zeros(G, P, D)
    ref_dp.scatter_(1, keep[:, :, None].expand(G, Lk, D), dx[:, 1:])
    assert not ref_dp[mask].any()
    for dt in (torch.float32, torch.bfloat16):
        d_cls = torch.full((D,), float("nan"), device=DEV)
        dp = torch.full((G * P, D), float("nan"), dtype=dt, device=DEV)
        ops.mae_embed_bwd(dx.to(DEV), _i32(restore), d_cls, dp)
        assert torch.equal(dp.cpu().view(G, P, D), ref_dp.to(dt))
        want = dx[:, 0].double().sum(0)
        assert (d_cls.cpu().double() - want).abs().max() <= 1e-6 * want.abs().max()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_mae_dec_assemble_fwd_bwd(case):
    from vspike import ops
    G, P, Lk, D = case
    keep, restore = _ids(G, P, Lk, 8)
    e, tok, tabd = _rand(G, Lk + 1, D, seed=9), _rand(D, seed=10), _rand(P + 1, D, seed=11)
    xd = torch.full((G, P + 1, D), float("nan"), device=DEV)
    ops.mae_dec_assemble_fwd(e.to(DEV), _i32(restore), tok.to(DEV), tabd.to(DEV), xd)
    # HF ViTMAEDecoder.forward: append mask tokens, unshuffle with ids_restore, prepend the CLS row, add the table
    full = torch.cat([e[:, 1:], tok.expand(G, P - Lk, D)], dim=1)
    full = torch.gather(full, 1, restore[:, :, None].expand(G, P, D))
    ref = torch.cat([e[:, :1], full], dim=1) + tabd
    assert torch.equal(xd.cpu(), ref)
    dxd = _rand(G, P + 1, D, seed=12)
    mask = restore >= Lk
    ref_de = torch.cat([dxd[:, :1], torch.gather(dxd[:, 1:], 1, keep[:, :, None].expand(G, Lk, D))], dim=1)
    want = (dxd[:, 1:].double() * mask[:, :, None]).sum((0, 1))
    ws = torch.full((ops.mae_dec_assemble_bwd_workspace_bytes(G, D) // 4,), float("nan"), device=DEV)
    for dt in (torch.float32, torch.bfloat16):
        de = torch.full((G, Lk + 1, D), float("nan"), dtype=dt, device=DEV)
        d_tok = torch.full((D,), float("nan"), device=DEV)
        ops.mae_dec_assemble_bwd(dxd.to(DEV), _i32(keep), _i32(restore), de, d_tok, ws)
        assert torch.equal(de.cpu(), ref_de.to(dt))
        if Lk == P:
            assert not d_tok.cpu().any()
        else:
            assert (d_tok.cpu().double() - want).abs().max() <= 1e-6 * want.abs().max()


@pytest.mark.parametrize("geom", [(4, 1, 48, 16, 2), (3, 1, 144, 16, 32), (2, 3, 32, 8, 1), (2, 1, 48, 16, 8)],
                         ids=lambda g: "x".join(map(str, g)))
def test_mae_recon_loss(geom):
    from vspike import ops
    G, C, S, patch, Lk = geom
    w = S // patch
    P, K = w * w, patch * patch * C
    _, restore = _ids(G, P, Lk, 13)
    pixels, pred = _rand(G, C, S, S, seed=14), _rand(G, P + 1, K, seed=15)
    # HF patchify: nchpwq -> n (hw) (pqc)
    target = pixels.double().view(G, C, w, patch, w, patch).permute(0, 2, 4, 3, 5, 1).reshape(G, P, K)
    mask = (restore >= Lk).double()
    p64 = pred.double().requires_grad_()
    loss_ref = (((p64[:, 1:] - target) ** 2).mean(-1) * mask).sum() / mask.sum()
    (g_ref,) = torch.autograd.grad(loss_ref, p64)
    ws = torch.full((ops.mae_recon_loss_workspace_bytes(G, P) // 4,), float("nan"), device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    d_pred = torch.full((G, P + 1, K), float("nan"), device=DEV)
    ops.mae_recon_loss(pred.to(DEV), pixels.to(DEV), _i32(restore), Lk, patch, loss, d_pred, ws)
    assert abs(loss.item() - loss_ref.item()) <= 1e-6 * abs(loss_ref.item())
    got = d_pred.cpu().double()
    assert not got[:, 0].any() and not got[:, 1:][mask == 0].any()
    assert (got - g_ref).abs().max() <= 1e-6 * g_ref.abs().max()
    d16 = torch.full((G, P + 1, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    loss2 = torch.full((1,), float("nan"), device=DEV)
    ops.mae_recon_loss(pred.to(DEV), pixels.to(DEV), _i32(restore), Lk, patch, loss2, d16, ws)
    assert torch.equal(loss2, loss)                                   # equal bits on a second call
    assert torch.equal(d16.cpu(), d_pred.cpu().to(torch.bfloat16))


def test_mae_ops_refuse_bad_arguments():
    from vspike import ops
    from vspike._lib import VsError
    G, P, Lk, D = 2, 9, 2, 64
    keep, restore = _ids(G, P, Lk, 3)
    x0 = torch.zeros(G, Lk + 1, D, device=DEV)
    with pytest.raises(VsError, match="int32"):
        ops.mae_embed_fwd(torch.zeros(G * P, D, device=DEV), keep.to(DEV), torch.zeros(D, device=DEV),
                          torch.zeros(P + 1, D, device=DEV), x0)
    pix = torch.zeros(G, 1, 48, 48, device=DEV)
    pred = torch.zeros(G, P + 1, 256, device=DEV)
    ws = torch.zeros(ops.mae_recon_loss_workspace_bytes(G, P) // 4, device=DEV)
    with pytest.raises(VsError, match="at least one masked"):      # every patch kept: HF's 0 / 0
        ops.mae_recon_loss(pred, pix, _i32(restore), P, 16, torch.zeros(1, device=DEV), torch.zeros_like(pred), ws)


# ------------------------------------------------------------------------------------------------------------
# the plugin (vspike/mae.py) against tests/golden/mae.npz and the restatement tests/mae_ref.py
# ------------------------------------------------------------------------------------------------------------
import numpy as np                      # noqa: E402

import mae_ref as mr                    # noqa: E402
from oracle import cpu_ref              # noqa: E402


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("mae.npz")


def _model(geom, dtype="fp32"):
    from vspike import MAE
    m = MAE(mr.model_config(geom, dtype)).to(DEV)
    m.load_reference_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in mr.make_params(geom).items()})
    return m


def _inputs(geom):
    return torch.from_numpy(mr.make_images(geom)).to(DEV), torch.from_numpy(mr.make_noise(geom)).to(DEV)


def _named_grads(m):
    out = {}
    for name, which, slot, rows, _ in m.hf_items():
        flat, lay = m._flat(which)
        t = lay.view(flat.grad, slot)
        out[name] = (t if rows is None else t[rows]).detach().cpu().numpy().copy()
    return out


def _distances(m, geom, fx):
    """(z, loss, {gradient: norm-relative}) distances of one forward + backward to the float64 fixture."""
    x, noise = _inputs(geom)
    m.zero_grad(set_to_none=True)
    out = m(x, noise)
    out["recon_loss"].backward()
    torch.cuda.synchronize()
    zr = fx[f"{geom}/z"]
    ez = float(np.abs(out["z"].cpu().numpy() - zr).max() / np.abs(zr).max())
    want = fx[f"{geom}/recon_loss"][0]
    el = abs(out["recon_loss"].item() - want) / want
    sub = {k[len(geom) + 1:]: v for k, v in fx.items() if k.startswith(geom + "/")}
    eg = {n: cpu_ref.summary_rel_error(n, g, sub) for n, g in _named_grads(m).items()}
    return ez, el, eg, out


@pytest.mark.parametrize("geom", sorted(mr.GEOMETRIES))
def test_plugin_fp32_parity_with_the_fixture(fixture, geom):
    """The project's fp32 bars (test_gpu_contrast.py:7): z 1e-4 of max|ref|, loss 1e-5 relative, every gradient 1e-3
    norm-relative; z at mask_ratio 0 at the same bar, with a NaN loss (HF's 0 / 0)."""
    m = _model(geom)
    ez, el, eg, out = _distances(m, geom, fixture)
    worst = max(eg, key=eg.get)
    print(f"\n[mae fp32 {geom}] z {ez:.2e}, loss {el:.2e}, worst gradient {worst} {eg[worst]:.2e}")
    assert not out["z"].requires_grad and out["recon_loss"].requires_grad
    assert ez <= 1e-4 and el <= 1e-5
    assert eg[worst] <= 1e-3, sorted(eg.items(), key=lambda kv: -kv[1])[:4]
    assert set(eg) == {n for n in mr.param_shapes(geom) if mr.trainable(n)}
    m.config.mask_ratio = 0.0
    out0 = m(_inputs(geom)[0])
    z0 = fixture[f"{geom}/z_mask0"]
    assert np.abs(out0["z"].cpu().numpy() - z0).max() <= 1e-4 * np.abs(z0).max()
    assert torch.isnan(out0["recon_loss"])


@pytest.mark.parametrize("geom", sorted(mr.GEOMETRIES))
def test_plugin_bf16_against_the_rounding_model(fixture, geom):
    """compute_dtype bf16 against the float64 fixture.  The yardstick is the model of rounding, not the plugin: the
    restatement with bf16-rounded matmul operands (contrast_ref.bf16_matmul, mae_ref.forward(bf16=True)) is run here
    and each of the plugin's distances (z, loss, the worst gradient) must stay within twice the model's.
    Measured on an MI355X, plugin | model: g1 z 7.9e-3 | 7.0e-3, loss 5.6e-5 | 2.9e-5, worst gradient 5.2e-2 | 4.9e-2;
    g2 z 6.4e-3 | 7.0e-3, loss 7.0e-6 | 8.3e-5, worst gradient 2.8e-2 | 2.4e-2.  The bar is twice the model's figure
    and not twice the measured one because the loss distances are cancellations far below bf16's 2^-9 (at g2 the
    plugin's is 12 times under the model's), so a constant taken from one measurement would pin an accident."""
    P = mr.to_torch(mr.make_params(geom), torch.float32)
    x, noise = torch.from_numpy(mr.make_images(geom)), torch.from_numpy(mr.make_noise(geom))
    ref = mr.forward(x, noise, P, geom, bf16=True)
    ref["recon_loss"].backward()
    sub = {k[len(geom) + 1:]: v for k, v in fixture.items() if k.startswith(geom + "/")}
    zr, want = fixture[f"{geom}/z"], fixture[f"{geom}/recon_loss"][0]
    mz = float(np.abs(ref["z"].detach().numpy() - zr).max() / np.abs(zr).max())
    ml = abs(ref["recon_loss"].item() - want) / want
    mg = max(cpu_ref.summary_rel_error(n, p.grad.numpy(), sub) for n, p in P.items() if mr.trainable(n))
    ez, el, eg, _ = _distances(_model(geom, "bf16"), geom, fixture)
    worst = max(eg, key=eg.get)
    print(f"\n[mae bf16 {geom}] plugin z {ez:.2e} loss {el:.2e} worst gradient {worst} {eg[worst]:.2e}; "
          f"model z {mz:.2e} loss {ml:.2e} worst gradient {mg:.2e}")
    assert ez <= 2 * mz and el <= 2 * ml and eg[worst] <= 2 * mg


def _trainer(m, lr=1e-3):
    from vspike import FusedAdamW
    from vspike.trainer import ContrastTrainer
    return ContrastTrainer(m, FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=lr))


def test_bf16_steps_are_bitwise_repeatable_for_equal_noise():
    runs = []
    for _ in range(2):
        m = _model("g2", "bf16")
        tr = _trainer(m)
        torch.manual_seed(7)                    # the plugin draws its noise from torch's device generator
        losses = [tr.step_recon(_inputs("g2")[0])["loss"] for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), m.enc_flat.detach().cpu().clone(), m.dec_flat.detach().cpu().clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0][0], runs[0][0][1])          # the model moved


def test_step_recon_equals_the_manual_sequence():
    from vspike import FusedAdamW
    x = _inputs("g1")[0]
    a, b = _model("g1"), _model("g1")
    tr = _trainer(a)
    torch.manual_seed(3)
    res = tr.step_recon(x)
    opt = FusedAdamW([p for p in b.parameters() if p.requires_grad], lr=1e-3)
    torch.manual_seed(3)
    loss = b(x)["recon_loss"]
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert set(res) == {"loss"} and not res["loss"].requires_grad and torch.equal(res["loss"], loss.detach())
    assert torch.equal(a.enc_flat, b.enc_flat) and torch.equal(a.dec_flat, b.dec_flat)
    assert a.enc_flat.grad is None


def test_transform_sets_mask_ratio_to_zero_and_restores_it(fixture):
    m = _model("g1")
    tr = _trainer(m)
    x = _inputs("g1")[0]
    z = tr.transform([x[:2], {"ref": x[2:]}])
    assert m.config.mask_ratio == 0.75 and m.training
    z0 = fixture["g1/z_mask0"]
    assert np.abs(z.cpu().numpy() - z0).max() <= 1e-4 * np.abs(z0).max()


def test_validate_on_a_128_wide_embedding_runs_the_wide_rrr_entries():
    from vspike import _lib as L
    m = _model("g1")
    tr = _trainer(m)
    g = torch.Generator().manual_seed(11)
    F, T, N = 5, 4, 3

    def batches(k):
        return [{"ref": torch.randn(F, 1, 48, 48, generator=g).to(DEV), "neural": torch.rand(1, T, N, generator=g) * 3}
                for _ in range(k)]
    L.dispatch_reset()
    res = tr.validate(batches(6), batches(3), idx=[0, 1, 2, 3])
    assert L.rrr_dispatch_counts()["rrr_wide"] > 0
    assert set(res) == {"val_bps"} and m.config.mask_ratio == 0.75


def test_training_curve_follows_the_restatement():
    """Five AdamW + OneCycleLR steps at g1 (fp32) with given noise against mae_ref driven through cpu_ref.train_curve,
    to 1e-3 (test_gpu_contrast.py's curve test)."""
    from vspike import FusedAdamW
    geom, steps, lr = "g1", 5, 1e-3
    P = cpu_ref.to_torch(mr.make_params(geom))
    batches = [((torch.from_numpy(mr.make_images(geom, mr.SEED + 100 + s)),
                 torch.from_numpy(mr.make_noise(geom, mr.SEED + 100 + s))), None) for s in range(steps)]
    want = cpu_ref.train_curve(lambda xn, prm: mr.forward(xn[0], xn[1], prm, geom)["recon_loss"], P, batches, lr=lr,
                               trainable=mr.trainable, criterion=lambda out, _y: out)
    m = _model(geom)
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=lr, weight_decay=0.01, eps=1e-8)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, total_steps=steps, max_lr=lr, pct_start=0.15, div_factor=10.0)
    got = []
    for (x, noise), _ in batches:
        loss = m(x.to(DEV), noise.to(DEV))["recon_loss"]
        loss.backward()
        opt.step()
        sched.step()
        opt.zero_grad(set_to_none=True)
        got.append(float(loss))
    print(f"\n[mae curve] got {got}\n            want {want}")
    assert max(abs(w - want[0]) for w in want) > 1e-2
    np.testing.assert_allclose(got, want, rtol=1e-3)
