"""vs_info_nce, vs_embed_head_fwd / _bwd and vs_cls_embed_fwd / _bwd (csrc/contrast.hip) on the GPU, against
float64 torch.

Bars: the three losses 1e-6 relative; gradients 1e-5 norm-relative (||got - ref|| / ||ref||).  The head's
forward outputs (h, z_raw, z) take the gradients' bar: they are f32 LayerNorm sums and dot products over D <= 768
terms, whose rounding is ~sqrt(D) 2^-24 = 1.7e-6 of the operands' norms.  vs_cls_embed_fwd and the compact patch
rows of vs_cls_embed_bwd are copies (plus one f32 add / one bf16 rounding) and must match bit for bit; d_cls must
equal the ascending f32 sum over images bit for bit.

Every operand sits in a larger allocation whose margins hold NaN: a kernel that read them would produce NaN, one
that wrote them is caught by the margin check, and the results must be the bits of a run on plain tensors."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 256
NCE_CASES = [(1, 1, 3), (2, 2, 1), (5, 5, 8), (5, 7, 3), (64, 64, 64), (65, 65, 3), (130, 130, 8)]
HEAD_CASES = [(1, 9, 128, 3), (15, 81, 128, 8), (3, 81, 768, 64)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _guard(t):
    """A copy of t inside a larger allocation whose margins hold NaN: (buffer, view)."""
    t = t.contiguous()
    pad = MARGIN * 8 // t.element_size()                      # a multiple of 16 bytes: the view stays aligned
    buf = torch.full((t.numel() + 2 * pad,), float("nan"), dtype=t.dtype, device=DEV)
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _margins_nan(buf, numel):
    pad = (buf.numel() - numel) // 2
    return bool(torch.isnan(buf[:pad]).all() and torch.isnan(buf[-pad:]).all())


def _relnorm(got, ref):
    ref = ref.double()
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------
# InfoNCE
# ------------------------------------------------------------------------------------------------
def _nce_reference(ref, pos, neg, log_inv_tau):
    r, p, q = (t.double().cpu().requires_grad_(True) for t in (ref, pos, neg))
    t = torch.tensor(0.0 if log_inv_tau is None else log_inv_tau, dtype=torch.float64, requires_grad=True)
    inv_tau = torch.exp(t)
    pd = (r * p).sum(-1) * inv_tau
    nd = r @ q.T * inv_tau
    c = nd.max(dim=1, keepdim=True)[0].detach()
    pos_loss = -(pd - c.squeeze(1)).mean()
    neg_loss = torch.logsumexp(nd - c, dim=1).mean()
    loss = pos_loss + neg_loss
    loss.backward()
    return torch.stack([loss, pos_loss, neg_loss]).detach(), r.grad, p.grad, q.grad, t.grad


def _nce_run(ops, ref, pos, neg, tau, guarded, grad_scale=1.0):
    n, E = ref.shape
    m = neg.shape[0]
    ws_n = ops.info_nce_workspace_bytes(n, m) // 4
    outs = [torch.zeros(3), torch.zeros(n, E), torch.zeros(n, E), torch.zeros(m, E), torch.zeros(1), torch.zeros(ws_n)]
    ins = [ref, pos, neg] + ([tau] if tau is not None else [])
    if guarded:
        gi, go = [_guard(t) for t in ins], [_guard(t) for t in outs]
        ins, outs = [v for _, v in gi], [v for _, v in go]
    else:
        ins, outs = [t.to(DEV) for t in ins], [t.to(DEV) for t in outs]
    out, dr, dp, dq, dt, ws = outs
    ops.info_nce(ins[0], ins[1], ins[2], out, log_inv_tau=ins[3] if tau is not None else None, d_ref=dr, d_pos=dp,
                 d_neg=dq, grad_scale=grad_scale, d_log_inv_tau=dt if tau is not None else None, workspace=ws)
    torch.cuda.synchronize()
    if guarded:
        for (buf, v) in gi + go[:5]:
            assert _margins_nan(buf, v.numel())
    return out, dr, dp, dq, dt


@pytest.mark.parametrize("with_tau", [False, True], ids=["tau1", "tau"])
@pytest.mark.parametrize("n,m,E", NCE_CASES)
def test_info_nce_matches_f64_and_ignores_its_surroundings(n, m, E, with_tau):
    from vspike import ops
    g = torch.Generator().manual_seed(100 * n + 10 * m + E)
    ref, pos, neg = (torch.nn.functional.normalize(torch.randn(k, E, generator=g), dim=-1) * 1.5 for k in (n, n, m))
    tau = torch.tensor([0.3]) if with_tau else None
    want, wr, wp, wq, wt = _nce_reference(ref, pos, neg, 0.3 if with_tau else None)
    out, dr, dp, dq, dt = _nce_run(ops, ref, pos, neg, tau, guarded=False)
    got = out.double().cpu()
    print(f"\n[info_nce n={n} m={m} E={E} tau={with_tau}] losses {got.tolist()} f64 {want.tolist()}")
    assert bool(((got - want).abs() <= 1e-6 * want.abs()).all()), (got, want)
    errs = {"d_ref": _relnorm(dr.cpu(), wr), "d_pos": _relnorm(dp.cpu(), wp), "d_neg": _relnorm(dq.cpu(), wq)}
    if with_tau:
        errs["d_log_inv_tau"] = abs(float(dt) - float(wt)) / max(abs(float(wt)), 1e-300)
    print("   gradient errors", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-5, errs
    # the same bits with NaN around every operand, and with the gradients scaled on the host side
    out2, dr2, dp2, dq2, dt2 = _nce_run(ops, ref, pos, neg, tau, guarded=True)
    for a, b in ((out, out2), (dr, dr2), (dp, dp2), (dq, dq2)) + (((dt, dt2),) if with_tau else ()):
        assert torch.equal(a, b)
    _, dr3, dp3, dq3, _ = _nce_run(ops, ref, pos, neg, tau, guarded=False, grad_scale=0.5)
    assert max(_relnorm(dr3.cpu(), 0.5 * wr), _relnorm(dp3.cpu(), 0.5 * wp), _relnorm(dq3.cpu(), 0.5 * wq)) <= 1e-5


def test_info_nce_forward_only_and_counter():
    from vspike import _lib as L, ops
    g = torch.Generator().manual_seed(3)
    ref, pos, neg = (torch.randn(k, 3, generator=g).to(DEV) for k in (5, 5, 7))
    want = _nce_reference(ref, pos, neg, None)[0]
    out = torch.zeros(3, device=DEV)
    L.dispatch_reset()
    ops.info_nce(ref, pos, neg, out)
    assert L.dispatch_counts()["info_nce"] == 1
    assert bool(((out.double().cpu() - want).abs() <= 1e-6 * want.abs()).all())
    with pytest.raises(L.VsError):
        ops.info_nce(ref, pos[:4], neg, out)                   # shapes are checked before any launch
    with pytest.raises(L.VsError):
        ops.info_nce(ref, pos, neg, out, workspace=torch.zeros(4, device=DEV))
    assert L.dispatch_counts()["info_nce"] == 1


# ------------------------------------------------------------------------------------------------
# embedding head
# ------------------------------------------------------------------------------------------------
def _head_inputs(G, P, D, E):
    g = torch.Generator().manual_seed(G + 3 * P + D + 7 * E)
    x = torch.randn(G, P + 1, D, generator=g) * 1.5 + 0.3
    gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    w = torch.randn(E, D, generator=g) / math.sqrt(D)
    b = 0.1 * torch.randn(E, generator=g)
    dz = torch.randn(G, E, generator=g)
    return x, gamma, beta, w, b, dz


def _head_reference(x, gamma, beta, w, b, dz, eps):
    xr, ga, be, wd, bd = (t.double().requires_grad_(True) for t in (x[:, 0], gamma, beta, w, b))
    h = torch.nn.functional.layer_norm(xr, (xr.shape[-1],), ga, be, eps)
    z_raw = h @ wd.T + bd
    z = z_raw / z_raw.norm(dim=-1, keepdim=True)
    (z * dz.double()).sum().backward()
    return h.detach(), z_raw.detach(), z.detach(), xr.grad, ga.grad, be.grad, wd.grad, bd.grad


@pytest.mark.parametrize("with_lp", [True, False], ids=["bf16copy", "f32only"])
@pytest.mark.parametrize("G,P,D,E", HEAD_CASES)
def test_embed_head_forward_and_backward(G, P, D, E, with_lp):
    from vspike import _lib as L, ops
    eps = 1e-12
    x, gamma, beta, w, b, dz = _head_inputs(G, P, D, E)
    h_ref, zraw_ref, z_ref, dx_ref, dg_ref, db_ref, dw_ref, dbp_ref = _head_reference(x, gamma, beta, w, b, dz, eps)
    xn = x.clone()
    xn[:, 1:] = float("nan")                                     # only the CLS row may be read
    gx, xd = _guard(xn)
    (gg, ga), (gb, be), (gw, wd), (gbp, bd), (gdz, dzd) = (_guard(t) for t in (gamma, beta, w, b, dz))
    outs = {k: _guard(torch.zeros(s)) for k, s in (("h", (G, D)), ("mean", (G,)), ("rstd", (G,)), ("z_raw", (G, E)),
                                                   ("nrm", (G,)), ("z", (G, E)))}
    o = {k: v for k, (_, v) in outs.items()}
    L.dispatch_reset()
    ops.embed_head_fwd(xd, (P + 1) * D, ga, be, eps, wd, bd, o["h"], o["mean"], o["rstd"], o["z_raw"], o["nrm"], o["z"])
    torch.cuda.synchronize()
    errs = {"h": _relnorm(o["h"].cpu(), h_ref), "z_raw": _relnorm(o["z_raw"].cpu(), zraw_ref),
            "z": _relnorm(o["z"].cpu(), z_ref), "nrm": _relnorm(o["nrm"].cpu(), zraw_ref.norm(dim=-1))}
    print(f"\n[embed_head G={G} P={P} D={D} E={E}] forward errors", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-5, errs
    assert float((o["z"].double().norm(dim=-1) - 1).abs().max()) <= 1e-6
    # backward
    gdx, dx = _guard(torch.full((G, P + 1, D), 7.0))
    gdl, dx_lp = _guard(torch.full((G, P + 1, D), 7.0, dtype=torch.bfloat16))
    grads = {k: _guard(torch.full(s, 7.0)) for k, s in (("dw", (E, D)), ("db", (E,)), ("dgamma", (D,)), ("dbeta", (D,)))}
    gr = {k: v for k, (_, v) in grads.items()}
    ops.embed_head_bwd(dzd, xd, (P + 1) * D, o["h"], o["mean"], o["rstd"], o["z_raw"], o["nrm"], ga, wd, dx,
                       dx_lp=dx_lp if with_lp else None, dw=gr["dw"], db=gr["db"], dgamma=gr["dgamma"], dbeta=gr["dbeta"])
    torch.cuda.synchronize()
    assert L.dispatch_counts()["embed_head"] == 2
    berrs = {"dx": _relnorm(dx[:, 0].cpu(), dx_ref), "dgamma": _relnorm(gr["dgamma"].cpu(), dg_ref),
             "dbeta": _relnorm(gr["dbeta"].cpu(), db_ref), "dw": _relnorm(gr["dw"].cpu(), dw_ref),
             "db": _relnorm(gr["db"].cpu(), dbp_ref)}
    print("   backward errors", {k: f"{v:.2e}" for k, v in berrs.items()})
    assert max(berrs.values()) <= 1e-5, berrs
    assert not bool(dx[:, 1:].any())                             # the other P rows: exactly 0
    if with_lp:
        assert torch.equal(dx_lp, dx.to(torch.bfloat16))         # the bf16 copy is the rounding of the f32 rows
    else:
        assert bool((dx_lp == 7.0).all())
    for buf, v in [(gx, xd), (gg, ga), (gb, be), (gw, wd), (gbp, bd), (gdz, dzd), (gdx, dx), (gdl, dx_lp)] + \
            list(outs.values()) + list(grads.values()):
        assert _margins_nan(buf, v.numel())
    # dx only (no parameter gradients, no workspace), and a rerun: the same bits
    dx2 = torch.full((G, P + 1, D), 7.0, device=DEV)
    ops.embed_head_bwd(dzd, xd, (P + 1) * D, o["h"], o["mean"], o["rstd"], o["z_raw"], o["nrm"], ga, wd, dx2)
    assert torch.equal(dx2, dx)
    dw2 = {k: torch.full_like(v, 3.0) for k, v in gr.items()}
    ops.embed_head_bwd(dzd, xd, (P + 1) * D, o["h"], o["mean"], o["rstd"], o["z_raw"], o["nrm"], ga, wd, dx2, **dw2)
    assert all(torch.equal(dw2[k], gr[k]) for k in gr)


def test_embed_head_image_alone_gives_the_same_bits():
    """Image g computed alone (G = 1) has the bits it has inside the batch: no sum depends on G."""
    from vspike import ops
    G, P, D, E = 15, 81, 128, 8
    x, gamma, beta, w, b, _ = (t.to(DEV) for t in _head_inputs(G, P, D, E))
    mk = lambda G: [torch.zeros(s, device=DEV) for s in ((G, D), (G,), (G,), (G, E), (G,), (G, E))]  # noqa: E731
    full = mk(G)
    ops.embed_head_fwd(x, (P + 1) * D, gamma, beta, 1e-12, w, b, *full)
    for g in (0, 7, 14):
        one = mk(1)
        ops.embed_head_fwd(x[g:g + 1], (P + 1) * D, gamma, beta, 1e-12, w, b, *one)
        assert all(torch.equal(a[0], f[g]) for a, f in zip(one, full)), g


# ------------------------------------------------------------------------------------------------
# CLS assembly
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,P,D,E", HEAD_CASES)
def test_cls_embed_forward_and_backward(G, P, D, E):
    from vspike import _lib as L, ops
    g = torch.Generator().manual_seed(G + P + D)
    patches, cls, table = torch.randn(G * P, D, generator=g), torch.randn(D, generator=g), torch.randn(P + 1, D, generator=g)
    (gp, pd), (gc, cd), (gt, td) = (_guard(t) for t in (patches, cls, table))
    gx, x = _guard(torch.full((G, P + 1, D), 7.0))
    L.dispatch_reset()
    ops.cls_embed_fwd(pd, cd, td, x)
    torch.cuda.synchronize()
    want = torch.cat([(cls + table[0]).expand(G, 1, D), patches.view(G, P, D)], dim=1)
    assert torch.equal(x.cpu(), want)
    # backward
    dx = torch.randn(G, P + 1, D, generator=g)
    gdx, dxd = _guard(dx)
    gdc, d_cls = _guard(torch.full((D,), 7.0))
    seq = torch.zeros(D)
    for i in range(G):
        seq = seq + dx[i, 0]                                    # ascending g, f32
    for dt in (torch.float32, torch.bfloat16):
        gdp, d_p = _guard(torch.full((G * P, D), 7.0, dtype=dt))
        ops.cls_embed_bwd(dxd, d_cls, d_p)
        torch.cuda.synchronize()
        assert torch.equal(d_p.cpu(), dx[:, 1:].reshape(G * P, D).to(dt))
        assert torch.equal(d_cls.cpu(), seq)
        assert _relnorm(d_cls.cpu(), dx[:, 0].double().sum(0)) <= 1e-5
        assert _margins_nan(gdp, d_p.numel())
    assert L.dispatch_counts()["cls_embed"] == 3
    for buf, v in ((gp, pd), (gc, cd), (gt, td), (gx, x), (gdx, dxd), (gdc, d_cls)):
        assert _margins_nan(buf, v.numel())


def test_wrappers_refuse_bad_shapes_without_launching():
    from vspike import _lib as L, ops
    L.dispatch_reset()
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    with pytest.raises(L.VsError):
        ops.cls_embed_fwd(z(8, 128), z(128), z(10, 128), z(1, 10, 128))          # 8 patch rows for P = 9
    with pytest.raises(L.VsError):
        ops.cls_embed_bwd(z(1, 10, 128), z(64), z(9, 128))
    with pytest.raises(L.VsError):
        ops.cls_embed_fwd(z(9, 100), z(100), z(10, 100), z(1, 10, 100))          # D % 8
    with pytest.raises(L.VsError):
        ops.embed_head_fwd(z(1, 10, 128), 1280, z(128), z(128), 1e-12, z(300, 128), z(300), z(1, 128), z(1), z(1),
                           z(1, 300), z(1), z(1, 300))                           # E > 256
    assert set(L.dispatch_counts().values()) == {0}
