"""vs_token_pool_fwd / vs_token_pool_bwd (csrc/token_pool.hip) on the GPU: the per-time-step mean of the
encoder's tokens (+ position table, + bf16 copy) and its backward.

Shapes (G, S, D) are the smallest that reach every path: one row (S = 1), fewer rows than the 32 row
lanes, S = 49 / 196 (one and two passes of the 4-row unrolled loop plus a tail), one to twelve
64-channel tiles (D = 320 is no multiple of 128 or 256), more than one group.

Forward bound, from the f32 arithmetic alone: the lane / LDS sums of S terms carry at most
(S-1) u sum|x_i| (u = 2^-24), i.e. (S-1) u max|x| on the mean; the division by S and the addition of
the position value (|pos| <= 1) add one rounding each of a value <= max|x| + 1:
|err| <= (S+2) 2^-24 (max|x| + 1).  The backward is one correctly rounded division."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1, 64), (3, 3, 64), (6, 5, 128), (2, 49, 128), (5, 196, 192), (4, 7, 320), (2, 196, 768)]
SENTINEL = -12288.0      # exact in bf16 too
MARGIN = 512


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _guarded(shape, dtype):
    """A tensor of `shape` inside a larger allocation whose margins hold a sentinel."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * MARGIN,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[MARGIN:MARGIN + n].view(shape)


def _margins_intact(buf):
    return bool((buf[:MARGIN] == SENTINEL).all() and (buf[-MARGIN:] == SENTINEL).all())


def _x(G, S, D, ldx=None, seed=5):
    g = torch.Generator().manual_seed(seed + G + 7 * S + D)
    ldx = ldx or D
    full = (torch.randn(G * S, ldx, generator=g) * 3.0 + 0.5).to(DEV)
    return full[:, :D]            # row stride ldx


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("G,S,D", SHAPES)
def test_forward_matches_f64_mean(G, S, D, with_pos):
    from vspike import ops
    x = _x(G, S, D)
    pos_rows = 3 if G == 6 else G          # G = 6: g % pos_rows is not the identity
    pos = ops.sinusoid_table(pos_rows, D, DEV) if with_pos else None
    obuf, out = _guarded((G, D), torch.float32)
    lbuf, out_lp = _guarded((G, D), torch.bfloat16)
    ops.token_pool_fwd(x, S, out, pos=pos, out_lp=out_lp)
    torch.cuda.synchronize()
    ref = x.double().view(G, S, D).mean(dim=1)
    if with_pos:
        ref = ref + pos.double()[torch.arange(G, device=DEV) % pos_rows]
    err = float((out.double() - ref).abs().max())
    bound = (S + 2) * 2.0 ** -24 * (float(x.abs().max()) + 1.0)
    print(f"\n[pool fwd G={G} S={S} D={D} pos={with_pos}] max err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(out_lp, out.to(torch.bfloat16))
    assert _margins_intact(obuf) and _margins_intact(lbuf)


@pytest.mark.parametrize("G,S,D", [(6, 5, 128), (4, 7, 320), (2, 196, 768)])
def test_forward_strided_input_and_no_bf16_copy(G, S, D):
    """ldx > D: the columns past D (never read) hold NaN; out_lp = NULL writes the f32 result only."""
    from vspike import ops
    x = _x(G, S, D, ldx=D + 12)               # a view of a [G*S, D + 12] tensor
    x._base[:, D:] = float("nan")
    obuf, out = _guarded((G, D), torch.float32)
    ops.token_pool_fwd(x, S, out)
    dense = torch.empty(G, D, device=DEV)
    ops.token_pool_fwd(x.contiguous(), S, dense)
    torch.cuda.synchronize()
    ref = x.double().reshape(G, S, D).mean(dim=1)
    assert float((out.double() - ref).abs().max()) <= (S + 2) * 2.0 ** -24 * (float(x.abs().max()) + 1.0)
    assert torch.equal(out, dense)             # the row stride does not change a bit
    assert _margins_intact(obuf)


@pytest.mark.parametrize("with_lp", [True, False])
@pytest.mark.parametrize("G,S,D", SHAPES)
def test_backward_broadcasts_dpool_over_s(G, S, D, with_lp):
    from vspike import ops
    g = torch.Generator().manual_seed(11 + G + S + D)
    dpool = (torch.randn(G, D, generator=g) * 2.0).to(DEV)
    xbuf, dx = _guarded((G * S, D), torch.float32)
    lbuf, dx_lp = _guarded((G * S, D), torch.bfloat16)
    ops.token_pool_bwd(dpool, S, dx, dx_lp if with_lp else None)
    torch.cuda.synchronize()
    ref = (dpool.double() / S).float()[:, None, :].expand(G, S, D).reshape(G * S, D)
    torch.testing.assert_close(dx, ref, rtol=2.0 ** -23, atol=0)
    rows = dx.view(G, S, D)
    assert torch.equal(rows, rows[:, :1].expand(G, S, D))      # all S rows of a group bitwise equal
    if with_lp:
        assert torch.equal(dx_lp, dx.to(torch.bfloat16))
    else:
        assert bool((dx_lp == SENTINEL).all())
    assert _margins_intact(xbuf) and _margins_intact(lbuf)


def test_fixed_order_reruns_and_group_alone_bitwise():
    """Two calls give the same bits; group g computed alone (G = 1) gives the bits it has inside G = 5:
    the summation order depends on (S, D) only."""
    from vspike import ops
    G, S, D = 5, 196, 192
    x = _x(G, S, D)
    pos = ops.sinusoid_table(G, D, DEV)
    a, b = torch.empty(G, D, device=DEV), torch.empty(G, D, device=DEV)
    ops.token_pool_fwd(x, S, a, pos=pos)
    ops.token_pool_fwd(x, S, b, pos=pos)
    assert torch.equal(a, b)
    for g in range(G):
        one = torch.empty(1, D, device=DEV)
        ops.token_pool_fwd(x[g * S:(g + 1) * S], S, one, pos=pos[g:g + 1])
        assert torch.equal(one[0], a[g]), g
    dpool = torch.randn(G, D, device=DEV)
    d1, d2 = torch.empty(G * S, D, device=DEV), torch.empty(G * S, D, device=DEV)
    ops.token_pool_bwd(dpool, S, d1)
    ops.token_pool_bwd(dpool, S, d2)
    assert torch.equal(d1, d2)


def test_dispatch_counter_counts_each_call():
    from vspike import _lib as L, ops
    G, S, D = 3, 3, 64
    x = _x(G, S, D)
    out, dx = torch.empty(G, D, device=DEV), torch.empty(G * S, D, device=DEV)
    L.dispatch_reset()
    assert L.dispatch_counts()["token_pool"] == 0
    ops.token_pool_fwd(x, S, out)
    assert L.dispatch_counts()["token_pool"] == 1
    ops.token_pool_bwd(out, S, dx)
    ops.token_pool_bwd(out, S, dx)
    assert L.dispatch_counts()["token_pool"] == 3
    torch.cuda.synchronize()
