"""The ContrastViT plugin and its InfoNCE step on the GPU, against tests/golden/contrast_vit.npz (HF ViTMAEModel +
the reference's loss_fn_, scripts/gen_contrast_fixture.py) and the CPU restatement tests/contrast_ref.py.

Geometries (contrast_ref.GEOMETRIES): g1 = 10 tokens (under one key tile), g2 = 82 tokens (64 + an 18-row tail);
D = 128, 2 heads, F = 256, 2 layers.

fp32 bars are the project's (test_gpu_models.py): z within 1e-4 of max|ref|, losses 1e-5 relative, every gradient
1e-3 norm-relative; the reference's own patch-shuffle noise is 30x below them.

bf16 bars are 2x the distance to the fixture measured on MI355X (test_bf16_against_the_fixture's docstring).
"""
import numpy as np
import pytest
import torch

import contrast_ref as cr
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_KEYS = ("loss", "pos_loss", "neg_loss")
# bf16 bars per geometry (z, losses, gradients) = 2x the larger of the fix / tau distances measured on MI355X:
# see test_bf16_against_the_fixture
BF16_BARS = {"g1": (4.1e-2, 3.8e-2, 1.72e-1), "g2": (2.0e-2, 6.5e-3, 1.55e-1)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("contrast_vit.npz")


def _sub(fx, prefix):
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


def _model(geom, dtype="fp32", fix_temp=True, seed=cr.SEED):
    from vspike import ContrastViT
    m = ContrastViT(cr.model_config(geom, dtype, fix_temp)).to(DEV)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in cr.make_params(geom, seed).items()}
    if not fix_temp:
        sd["temperature"] = torch.tensor(cr.TEMPERATURE)
    m.load_reference_state_dict(sd)
    return m


def _views(geom, seed=cr.SEED):
    return [torch.from_numpy(cr.make_images(geom, w, seed)).to(DEV) for w in ("ref", "pos", "neg")]


def _named_grads(m):
    """reference parameter name -> gradient (numpy), the q / k / v rows cut out of the fused slots."""
    out = {}
    for name, which, slot, rows in m.layout.hf_items():
        t = m._flat_layout(which).view(m._flat(which).grad, slot)
        out[name] = (t if rows is None else t[rows]).detach().cpu().numpy().copy()
    if m.temperature.grad is not None:
        out["temperature"] = m.temperature.grad.detach().cpu().numpy().copy()
    return out


def _three_calls(m, views, fix_temp):
    """The reference trainer's literal step up to the backward (src/trainer/contrast.py:80-88, 100-118)."""
    from vspike import InfoNCE
    m.zero_grad(set_to_none=True)
    outs = [m(v) for v in views]
    res = InfoNCE(fix_temp=fix_temp)(*outs)
    res["loss"].backward()
    torch.cuda.synchronize()
    return res, torch.cat([o["z"] for o in outs]).detach()


def _distances(m, res, z, fx, geom, tag):
    zr = fx[f"{geom}/z"]
    ez = float(np.abs(z.cpu().numpy() - zr).max() / np.abs(zr).max())
    want = fx[f"{geom}/{tag}/losses"]
    got = np.array([float(res[k].detach()) for k in LOSS_KEYS])
    el = float((np.abs(got - want) / np.abs(want)).max())
    sub = _sub(fx, f"{geom}/{tag}/")
    eg = {n: cpu_ref.summary_rel_error(n, g, sub) for n, g in _named_grads(m).items()}
    return ez, el, eg, got, want


@pytest.mark.parametrize("tag", ["fix", "tau"])
@pytest.mark.parametrize("geom", sorted(cr.GEOMETRIES))
def test_fp32_parity_with_the_fixture(fixture, geom, tag):
    fix_temp = tag == "fix"
    m = _model(geom, "fp32", fix_temp)
    res, z = _three_calls(m, _views(geom), fix_temp)
    ez, el, eg, got, want = _distances(m, res, z, fixture, geom, tag)
    worst = max(eg, key=eg.get)
    print(f"\n[fp32 {geom} {tag}] z {ez:.2e}, losses {el:.2e} ({got} vs {want}), worst gradient {worst} {eg[worst]:.2e}")
    assert ez <= 1e-4 and el <= 1e-5
    assert eg[worst] <= 1e-3, sorted(eg.items(), key=lambda kv: -kv[1])[:4]
    assert set(eg) == {n for n in cr.param_shapes(cr.vit_cfg(geom), 3) if cr.trainable(n, fix_temp)}
    if fix_temp:
        assert m.temperature.grad is None
    else:
        assert "temperature" in eg


@pytest.mark.parametrize("tag", ["fix", "tau"])
@pytest.mark.parametrize("geom", sorted(cr.GEOMETRIES))
def test_bf16_against_the_fixture(fixture, geom, tag):
    """bf16 activations / weights against the fp32 HF fixture.  Measured on MI355X (z relative to max|z|, worst
    loss relative, worst gradient norm-relative):
        g1 fix: z 2.05e-2, losses 1.87e-2, gradient 8.56e-2      g1 tau: z 2.05e-2, losses 1.87e-2, gradient 8.29e-2
        g2 fix: z 9.97e-3, losses 3.23e-3, gradient 7.74e-2      g2 tau: z 9.97e-3, losses 3.23e-3, gradient 6.93e-2
    Bars = 2x the larger value of each geometry.  z at g1 and the gradients are above 3x smoke()'s bf16 bars
    (1.8e-2 / 4.5e-2), so a bug was looked for first: the fixture's weights are drawn with std 0.1 (5x HF's, so
    that z is not degenerate), and the CPU restatement with nothing but bf16 rounding of the products' operands
    and stored outputs (contrast_ref.bf16_matmul) moves by the same amounts: z 1.33e-2 / 1.43e-2, worst gradient
    7.65e-2 / 1.08e-1 (g1 / g2), asserted to lie within a factor 2 of the figures above by
    test_cpu_contrast.py::test_bf16_rounding_alone_accounts_for_the_gpu_bf16_distances; the fp32 run of the same
    code path is within 1.2e-6 / 8e-6.  Rounding, no bug."""
    fix_temp = tag == "fix"
    m = _model(geom, "bf16", fix_temp)
    res, z = _three_calls(m, _views(geom), fix_temp)
    ez, el, eg, got, want = _distances(m, res, z, fixture, geom, tag)
    worst = max(eg, key=eg.get)
    print(f"\n[bf16 {geom} {tag}] z {ez:.2e}, losses {el:.2e} ({got} vs {want}), worst gradient {worst} {eg[worst]:.2e}")
    z_bar, loss_bar, grad_bar = BF16_BARS[geom]
    assert ez <= z_bar and el <= loss_bar
    assert eg[worst] <= grad_bar, sorted(eg.items(), key=lambda kv: -kv[1])[:4]


@pytest.mark.parametrize("geom,fix_temp", [("g1", True), ("g2", False)])
def test_fused_step_equals_the_three_call_form(geom, fix_temp):
    """ContrastTrainer.step (one 3n forward, one vs_info_nce, one backward) against the three-call form: losses and
    every gradient to 1e-5 in fp32; the three-call form is refused while a gradient sink is attached."""
    from vspike import FusedAdamW
    from vspike.dp import GradExchange
    from vspike.trainer import ContrastTrainer
    views = _views(geom)
    a = _model(geom, "fp32", fix_temp)
    res_a, _ = _three_calls(a, views, fix_temp)
    ga = _named_grads(a)
    b = _model(geom, "fp32", fix_temp)
    grads = {}

    class _Peek(FusedAdamW):               # the fused step's gradients, seen just before the update
        def step(self, closure=None):
            grads.update(_named_grads(b))
            return super().step(closure)

    tr = ContrastTrainer(b, _Peek([p for p in b.parameters() if p.requires_grad], lr=1e-4))
    res_b = tr.step(*views)
    torch.cuda.synchronize()
    for k in LOSS_KEYS:
        x, y = float(res_a[k].detach()), float(res_b[k])
        assert abs(x - y) <= 1e-5 * abs(x), (k, x, y)
    assert set(grads) == set(ga)
    errs = {n: float(np.linalg.norm((grads[n] - ga[n]).ravel()) / max(np.linalg.norm(ga[n].ravel()), 1e-30)) for n in ga}
    worst = max(errs, key=errs.get)
    print(f"\n[fused vs three calls {geom}] worst gradient {worst} {errs[worst]:.2e}")
    assert errs[worst] <= 1e-5
    assert all(p.grad is None for p in b.parameters())          # the step zeroes the gradients
    # with a sink attached the three-call form raises; the fused step goes through the sink
    c = _model(geom, "fp32", fix_temp)
    ex = GradExchange(c)
    trc = ContrastTrainer(c, FusedAdamW([p for p in c.parameters() if p.requires_grad], lr=1e-4), exchange=ex)
    with pytest.raises(RuntimeError, match="second forward"):
        trc.step_three_calls(*views)
    del trc
    c2 = _model(geom, "fp32", fix_temp)
    trc2 = ContrastTrainer(c2, FusedAdamW([p for p in c2.parameters() if p.requires_grad], lr=1e-4),
                           exchange=GradExchange(c2))
    res_c = trc2.step(*views)
    torch.cuda.synchronize()
    # the same update as without the sink, to the bar above (fp32 products sum some split partials with f32
    # atomics, so fp32 steps are not bitwise reproducible; the bf16 step is, see the test below)
    assert abs(float(res_c["loss"]) - float(res_b["loss"])) <= 1e-5 * abs(float(res_b["loss"]))
    for got, want in ((c2.enc_flat.detach(), b.enc_flat.detach()), (c2.head_flat.detach(), b.head_flat.detach())):
        assert float((got - want).norm() / want.norm()) <= 1e-5


def test_transform_stacks_z_without_grad():
    from vspike.trainer import ContrastTrainer
    m = _model("g1")
    views = _views("g1")
    z = ContrastTrainer(m, optimizer=None).transform([views[0], {"ref": views[1]}])
    assert z.shape == (8, 3) and not z.requires_grad
    with torch.no_grad():
        want = torch.cat([m(views[0])["z"], m(views[1])["z"]])
    assert torch.equal(z, want)


@pytest.mark.parametrize("geom", ["g1", "g2"])
def test_bf16_fused_steps_are_bitwise_reproducible(geom):
    """Two bf16 fused steps from the same state: bit-identical losses and parameters.  The plugin runs the blocks'
    weight-gradient products in order on the main stream; the side stream is not offered for it (it raises): with
    it on, about 1 backward in 100 differed at g2, so that variant of this check is left
    out together with the path."""
    from vspike import FusedAdamW
    from vspike.trainer import ContrastTrainer
    runs = []
    for _ in range(2):
        m = _model(geom, "bf16", fix_temp=False)
        with pytest.raises(ValueError, match="side stream"):
            m.set_side_stream(True)
        m.set_side_stream(False)
        assert m.__dict__["_side"] is False
        tr = ContrastTrainer(m, FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3))
        losses = [tr.step(*_views(geom, seed=cr.SEED + s)) for s in range(2)]
        torch.cuda.synchronize()
        runs.append((torch.stack([l[k] for l in losses for k in LOSS_KEYS]).cpu(), m.enc_flat.detach().cpu().clone(),
                     m.head_flat.detach().cpu().clone(), m.temperature.detach().cpu().clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][3]) != cr.TEMPERATURE                  # the temperature trained


def test_training_curve_follows_the_restatement():
    """Five AdamW + OneCycleLR steps at g1 (fp32) against contrast_ref driven through cpu_ref.train_curve, to 1e-3."""
    from vspike import FusedAdamW
    from vspike.trainer import ContrastTrainer
    geom, steps, lr = "g1", 5, 1e-3
    cfg = cr.vit_cfg(geom)
    P = cpu_ref.to_torch(cr.make_params(geom))
    batches = [([torch.from_numpy(cr.make_images(geom, w, cr.SEED + 100 + s)) for w in ("ref", "pos", "neg")], None)
               for s in range(steps)]
    want = cpu_ref.train_curve(lambda views, prm: cr.step_losses(views, prm, cfg)[0]["loss"], P, batches, lr=lr,
                               trainable=lambda n: cr.trainable(n, True), criterion=lambda out, _y: out)
    m = _model(geom, "fp32")
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=lr, weight_decay=0.01, eps=1e-8)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, total_steps=steps, max_lr=lr, pct_start=0.15, div_factor=10.0)
    tr = ContrastTrainer(m, opt, sched)
    got = [float(tr.step(*[v.to(DEV) for v in views])["loss"]) for views, _ in batches]
    print(f"\n[curve] got {got}\n        want {want}")
    assert max(abs(w - want[0]) for w in want) > 1e-2            # the curve moves: the comparison means something
    np.testing.assert_allclose(got, want, rtol=1e-3)


# ------------------------------------------------------------------------------------------------
# data parallel: two gloo ranks on one GPU (test_gpu_dp.py's pattern), each on its half of the views
# ------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out):
    import os
    import torch.distributed as dist
    from vspike import InfoNCE
    from vspike.dp import GradExchange
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = _model("g1", "fp32", fix_temp=False)
    if rank == 1:
        with torch.no_grad():
            m.head_flat.add_(0.5)                   # replicas built differently: the broadcast aligns them
    from vspike import FusedAdamW
    from vspike.trainer import ContrastTrainer
    ex = GradExchange(m, bucket_mb=0.25)
    per = cr.GEOMETRIES["g1"]["n"] // world
    views = [v[rank * per:(rank + 1) * per] for v in _views("g1")]
    seen = {}

    class _Peek(FusedAdamW):               # the exchanged (summed) gradients, seen just before the update
        def step(self, closure=None):
            torch.cuda.synchronize()
            seen.update({k: v / world for k, v in _named_grads(m).items()})
            return super().step(closure)

    opt = _Peek([p for p in m.parameters() if p.requires_grad], lr=1e-4, grad_scale=1.0 / world)
    # the documented entry point: the fused step with the exchange (finish() runs inside it)
    ContrastTrainer(m, opt, criterion=InfoNCE(fix_temp=False), exchange=ex).step(*views)
    torch.cuda.synchronize()
    out[rank] = seen
    dist.destroy_process_group()


def test_two_ranks_average_the_half_batch_gradients():
    """Each rank's loss uses its own n / 2 negatives (as the reference under DDP); the exchanged gradient / world
    equals the restatement's average of the two half-batches' gradients (fp32 bar, 1e-3 norm-relative)."""
    import socket
    import torch.multiprocessing as mp
    world, geom = 2, "g1"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(world, port, out), nprocs=world, join=True)
    cfg, per = cr.vit_cfg(geom), cr.GEOMETRIES[geom]["n"] // world
    want = {}
    for r in range(world):
        params = cr.make_params(geom)
        params["temperature"] = np.float32(cr.TEMPERATURE)
        P = cpu_ref.to_torch(params)
        views = [torch.from_numpy(cr.make_images(geom, w))[r * per:(r + 1) * per] for w in ("ref", "pos", "neg")]
        cr.step_losses(views, P, cfg, fix_temp=False)[0]["loss"].backward()
        for n, t in P.items():
            if cr.trainable(n, False):
                want[n] = want.get(n, 0) + t.grad.numpy() / world
    assert set(out[0]) == set(want)
    for r in range(world):
        errs = {n: float(np.linalg.norm((out[r][n] - want[n].reshape(out[r][n].shape)).ravel()) /
                         max(np.linalg.norm(want[n].ravel()), 1e-30)) for n in want}
        worst = max(errs, key=errs.get)
        print(f"\n[dp rank {r}] worst gradient {worst} {errs[worst]:.2e}")
        assert errs[worst] <= 1e-3, sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    assert all(np.array_equal(out[0][n], out[1][n]) for n in want)
