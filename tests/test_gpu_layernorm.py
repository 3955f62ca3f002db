"""vs_layernorm_fwd / vs_layernorm_bwd on every kernel instantiation of csrc/norm.hip.

Six scalar kernels (2, 3, 4, 8, 12, 16 values per lane: cols <= 128, 192, 256, 512, 768, 1024) and three
vectorised ones (cols = 192, 384, 768 with 16-byte aligned rows), each with a grid-stride row loop.  The
reference is fp64 torch.nn.functional.layer_norm and its autograd on the same f32 inputs; the bound is
1e-5 of max |reference| (test_gpu_ops.py's), except where a test states another.  Every call asserts
through the LayerNorm counters (vs_ln_dispatch_counts) which instantiation ran.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-12          # the reference model's nn.LayerNorm eps
SENTINEL = -777.0
# cols -> the instantiation vs_layernorm_* picks for dense, aligned rows
KERNEL = {1: "vpl2", 64: "vpl2", 100: "vpl2", 160: "vpl3", 256: "vpl4", 320: "vpl8", 512: "vpl8", 640: "vpl12",
          1000: "vpl16", 1024: "vpl16", 192: "vec192", 384: "vec384", 768: "vec768"}
SCALAR_OF = {192: "vpl3", 384: "vpl8", 768: "vpl12"}     # where the vectorised widths fall without aligned rows


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vspike import _lib as L
    L.lib()


def rel(a, b):
    """max |a - b| / max |b|; 0 when both are exactly zero (cols = 1: every gradient but dbeta vanishes)."""
    a, b = a.double().cpu(), b.double().cpu()
    d = (a - b).abs().max().item()
    return d / max(b.abs().max().item(), 1e-30) if d else 0.0


def _rand(*shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


class _Buf:
    """[R, C] device tensor `t` with row stride ld inside an allocation filled with `fill` (NaN around
    inputs, a sentinel around outputs)."""

    def __init__(self, R, C, ld, dtype, fill, vals=None):
        self.buf = torch.full((R * ld + 8,), fill, dtype=dtype, device=DEV)
        self.full = self.buf[:R * ld].view(R, ld)
        self.t, self.C = self.full[:, :C], C
        if vals is not None:
            self.t.copy_(vals.to(dtype))
        self.snap = self.buf.clone()

    def outside_untouched(self):
        a, b = self.buf.clone(), self.snap.clone()
        for x in (a, b):
            x[:self.full.numel()].view_as(self.full)[:, :self.C] = 0
        return torch.equal(a, b)


class Problem:
    """Inputs of one LayerNorm (f32, on the CPU) and their fp64 forward / backward."""

    def __init__(self, rows, cols, seed=0, shift=1.0, device="cpu"):
        self.rows, self.cols = rows, cols
        self.x = _rand(rows, cols, seed=seed + 1, scale=3.0 if shift == 1.0 else 1.0, shift=shift)
        self.g = 1 + 0.1 * _rand(cols, seed=seed + 2)
        self.b = 0.1 * _rand(cols, seed=seed + 3)
        self.dy = _rand(rows, cols, seed=seed + 4)
        self.dres = _rand(rows, cols, seed=seed + 5)
        self.device = device
        self._bwd = {}

    def fwd_ref(self, wd=torch.float64):
        """(y, mean, rstd) of torch's layer_norm in `wd` (native_layer_norm: the same op with its statistics)."""
        y, mean, rstd = torch.native_layer_norm(self.x.to(self.device, wd), (self.cols,), self.g.to(self.device, wd),
                                                self.b.to(self.device, wd), EPS)
        return y, mean.reshape(-1), rstd.reshape(-1)

    def bwd_ref(self, dy_dtype=F32, wd=torch.float64):
        """(dx without dres, dgamma, dbeta) for dy rounded to dy_dtype; computed once per dtype."""
        key = (dy_dtype, wd)
        if key not in self._bwd:
            x = self.x.to(self.device, wd).requires_grad_()
            g = self.g.to(self.device, wd).requires_grad_()
            b = self.b.to(self.device, wd).requires_grad_()
            y = torch.nn.functional.layer_norm(x, (self.cols,), g, b, EPS)
            self._bwd[key] = torch.autograd.grad(y, (x, g, b), self.dy.to(dy_dtype).to(self.device, wd))
        return self._bwd[key]


def _ln_counts():
    from vspike import _lib as L
    return {k: v for k, v in L.ln_dispatch_counts().items() if v}


def _forward(p, y_dtype=F32, pad=0, kernel=None):
    from vspike import ops, _lib as L
    nan = float("nan")
    x = _Buf(p.rows, p.cols, p.cols + pad, F32, nan, p.x)
    y = _Buf(p.rows, p.cols, p.cols + pad, y_dtype, SENTINEL)
    mean = torch.full((p.rows + 8,), SENTINEL, device=DEV)
    rstd = torch.full((p.rows + 8,), SENTINEL, device=DEV)
    L.dispatch_reset()
    ops.layernorm_fwd(x.t, p.g.to(DEV), p.b.to(DEV), EPS, y.t, mean, rstd)
    torch.cuda.synchronize()
    if kernel:
        assert _ln_counts() == {"fwd_" + kernel: 1}, (_ln_counts(), kernel)
    assert y.outside_untouched() and (mean[p.rows:] == SENTINEL).all() and (rstd[p.rows:] == SENTINEL).all()
    return y.t.clone(), mean[:p.rows].clone(), rstd[:p.rows].clone()


def _backward(p, mean, rstd, *, dy_dtype=F32, dres=True, lp=True, ws=True, pad=0, kernel=None, dg0=None, db0=None):
    """One vs_layernorm_bwd call: returns dx, dx_lp (or None), dgamma, dbeta."""
    from vspike import ops, _lib as L
    nan = float("nan")
    ld = p.cols + pad
    x = _Buf(p.rows, p.cols, ld, F32, nan, p.x)
    dy = _Buf(p.rows, p.cols, ld, dy_dtype, nan, p.dy)
    dr = _Buf(p.rows, p.cols, ld, F32, nan, p.dres) if dres else None
    dx = _Buf(p.rows, p.cols, ld, F32, SENTINEL)
    dx_lp = _Buf(p.rows, p.cols, ld, BF, SENTINEL) if lp else None      # dx's row stride (the ABI's)
    dg = torch.full((p.cols + 8,), SENTINEL, device=DEV)
    db = torch.full((p.cols + 8,), SENTINEL, device=DEV)
    dg[:p.cols] = 0 if dg0 is None else dg0.to(DEV)
    db[:p.cols] = 0 if db0 is None else db0.to(DEV)
    L.dispatch_reset()
    ops.layernorm_bwd(dy.t, x.t, mean, rstd, p.g.to(DEV), dx.t, dg, db, dres=dr.t if dres else None,
                      dx_lp=dx_lp.t if lp else None, workspace=None if ws else False)
    torch.cuda.synchronize()
    if kernel:
        assert _ln_counts() == {"bwd_" + kernel: 1}, (_ln_counts(), kernel)
    assert dx.outside_untouched() and (dx_lp is None or dx_lp.outside_untouched())
    assert (dg[p.cols:] == SENTINEL).all() and (db[p.cols:] == SENTINEL).all()
    return dx.t.clone(), (dx_lp.t.clone() if lp else None), dg[:p.cols].clone(), db[:p.cols].clone()


def _check_backward(p, out, dy_dtype, dres, tol=1e-5):
    dx, dx_lp, dg, db = out
    gx, gg, gb = p.bwd_ref(dy_dtype)
    gx = gx.cpu() + (p.dres.double() if dres else 0)
    assert rel(dx, gx) < tol, rel(dx, gx)
    assert rel(dg, gg) < tol and rel(db, gb) < tol, (rel(dg, gg), rel(db, gb))
    if dx_lp is not None:
        assert torch.equal(dx_lp, dx.to(BF))          # the bf16 copy is the rounded f32 result


# --------------------------------------------------------------------------------- every instantiation
@pytest.mark.parametrize("rows", [1, 3, 333])
@pytest.mark.parametrize("cols", sorted(KERNEL))
def test_every_instantiation(rows, cols):
    """Forward (f32 and bf16 y) and backward (f32 and bf16 dy, with and without dres, dx_lp and the
    workspace) on each of the nine kernels, at 1, 3 and 333 rows: ragged widths (1, 100, 160, 320, 640,
    1000) exercise the scalar kernels' column predicates, 333 rows their partial last row group."""
    p = Problem(rows, cols, seed=10 * cols)
    k = KERNEL[cols]
    yr, mr, rr = p.fwd_ref()
    y, mean, rstd = _forward(p, F32, kernel=k)
    assert rel(y, yr) < 1e-5 and rel(mean, mr) < 1e-5 and rel(rstd, rr) < 1e-5, (rel(y, yr), rel(mean, mr), rel(rstd, rr))
    yb, mean_b, rstd_b = _forward(p, BF, kernel=k)
    assert rel(yb, yr) < 5e-3 and torch.equal(mean_b, mean) and torch.equal(rstd_b, rstd)
    for dy_dtype, dres, lp, ws in ((F32, True, True, True), (F32, False, False, False), (BF, True, True, False),
                                   (BF, False, False, True)):
        out = _backward(p, mean, rstd, dy_dtype=dy_dtype, dres=dres, lp=lp, ws=ws, kernel=k)
        _check_backward(p, out, dy_dtype, dres)


def test_cols_out_of_range_is_rejected():
    from vspike import _lib as L
    for cols in (1025, 0):
        y = torch.full((3, 1032), SENTINEL, device=DEV)
        mean, rstd = torch.zeros(3, device=DEV), torch.ones(3, device=DEV)
        x = torch.zeros(3, 1032, device=DEV)
        g = torch.ones(1032, device=DEV)
        L.dispatch_reset()
        with pytest.raises(L.VsError):
            rc = L.lib().vs_layernorm_fwd(L.VS_F32, 3, cols, x.data_ptr(), 1032, g.data_ptr(), g.data_ptr(), EPS,
                                          y.data_ptr(), 1032, mean.data_ptr(), rstd.data_ptr(), L.stream())
            L.check(rc, "vs_layernorm_fwd")
        with pytest.raises(L.VsError):
            rc = L.lib().vs_layernorm_bwd(3, cols, x.data_ptr(), 1032, x.data_ptr(), 1032, mean.data_ptr(),
                                          rstd.data_ptr(), g.data_ptr(), None, 0, y.data_ptr(), 1032, None,
                                          mean.data_ptr(), rstd.data_ptr(), None, L.stream())
            L.check(rc, "vs_layernorm_bwd")
        torch.cuda.synchronize()
        assert not _ln_counts() and (y == SENTINEL).all()


# --------------------------------------------------------------------------------- strides
@pytest.mark.parametrize("cols", [192, 384, 768])
def test_strided_rows(cols):
    """x, y, dy, dres, dx (and dx_lp, on dx's row stride) as column slices of wider tensors.  ld = cols + 4
    keeps rows 16-byte aligned and must stay on the vectorised kernel; ld = cols + 1 must fall back to the
    scalar kernel of that width and agree with the vectorised result to 1e-6 (the same f32 arithmetic per
    row, another summation order).  Pad columns of inputs hold NaN; those of outputs a sentinel that must
    survive (_forward / _backward)."""
    p = Problem(333, cols, seed=7)
    yr, mr, rr = p.fwd_ref()
    res = {}
    for pad, k in ((4, KERNEL[cols]), (1, SCALAR_OF[cols])):
        y, mean, rstd = _forward(p, F32, pad=pad, kernel=k)
        assert rel(y, yr) < 1e-5 and rel(mean, mr) < 1e-5 and rel(rstd, rr) < 1e-5
        yb, _, _ = _forward(p, BF, pad=pad, kernel=k)
        assert rel(yb, yr) < 5e-3
        outs = []
        for dy_dtype, dres, lp in ((F32, True, True), (BF, False, False)):
            out = _backward(p, mean, rstd, dy_dtype=dy_dtype, dres=dres, lp=lp, pad=pad, kernel=k)
            _check_backward(p, out, dy_dtype, dres)
            outs.append(out)
        res[pad] = (y, mean, rstd, outs)
    (y4, m4, r4, o4), (y1, m1, r1, o1) = res[4], res[1]
    assert rel(y1, y4) < 1e-6 and rel(m1, m4) < 1e-6 and rel(r1, r4) < 1e-6
    for a, b in zip(o1, o4):
        assert rel(a[0], b[0]) < 1e-6 and rel(a[2], b[2]) < 1e-6 and rel(a[3], b[3]) < 1e-6


def test_strided_rows_scalar_width():
    """The same slices on a width that has scalar kernels only (cols = 160, ld = 161 and 164)."""
    p = Problem(37, 160, seed=8)
    yr, mr, rr = p.fwd_ref()
    for pad in (1, 4):
        y, mean, rstd = _forward(p, F32, pad=pad, kernel="vpl3")
        assert rel(y, yr) < 1e-5 and rel(mean, mr) < 1e-5 and rel(rstd, rr) < 1e-5
        _check_backward(p, _backward(p, mean, rstd, pad=pad, kernel="vpl3"), F32, True)


# --------------------------------------------------------------------------------- grid-stride loops
@pytest.mark.parametrize("cols", [192, 384, 768])
def test_vectorised_grid_stride_and_prefetch(cols, knobs):
    """Grid caps of 2 blocks (knobs ln_fwd_blocks / ln_blocks) at 333 rows: every lane group walks many
    trips of the row loop (16, 8, 4 rows per block pass at 192, 384, 768) and ends on a partial one, where
    the backward's prefetch of row + stride must not run.  The work is per row, so y, mean, rstd, dx and
    dx_lp are bitwise those of the default grid; dgamma / dbeta (another partial-sum split) stay within 1e-5
    of fp64, and two runs at the same cap are bitwise equal (fixed-order partial sums)."""
    p = Problem(333, cols, seed=9)
    k = KERNEL[cols]
    y0, m0, r0 = _forward(p, kernel=k)
    b0 = {(d, ws): _backward(p, m0, r0, dy_dtype=d, ws=ws, kernel=k) for d in (F32, BF) for ws in (True, False)}
    knobs("ln_fwd_blocks", 2)
    knobs("ln_blocks", 2)
    y, mean, rstd = _forward(p, kernel=k)
    assert torch.equal(y, y0) and torch.equal(mean, m0) and torch.equal(rstd, r0)
    for (d, ws), ref in b0.items():
        out = _backward(p, mean, rstd, dy_dtype=d, ws=ws, kernel=k)
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
        _check_backward(p, out, d, True)
        if ws:
            again = _backward(p, mean, rstd, dy_dtype=d, ws=ws, kernel=k)
            assert all(torch.equal(a, b) for a, b in zip(out, again))


@pytest.mark.parametrize("rows,cols", [(40000, 128), (9000, 1024)])
def test_scalar_backward_second_trip(rows, cols):
    """The scalar backward's row loop takes a second trip only past its cap of 1,024 blocks with the
    workspace: 40,000 rows at 32 per block (cols 128) and 9,000 rows at 8 per block (cols 1,024)."""
    p = Problem(rows, cols, seed=11, device=DEV)
    yr, mr, rr = p.fwd_ref()
    y, mean, rstd = _forward(p, kernel=KERNEL.get(cols, "vpl2"))
    assert rel(y, yr) < 1e-5 and rel(rstd, rr) < 1e-5
    out = _backward(p, mean, rstd, ws=True, kernel=KERNEL.get(cols, "vpl2"))
    _check_backward(p, out, F32, True)
    again = _backward(p, mean, rstd, ws=True)
    assert all(torch.equal(a, b) for a, b in zip(out, again))


# --------------------------------------------------------------------------------- accumulation
@pytest.mark.parametrize("ws", [True, False], ids=["workspace", "atomics"])
@pytest.mark.parametrize("cols", [128, 192, 640])
def test_dgamma_dbeta_accumulate(cols, ws):
    """dgamma / dbeta are added to, by ln_partsum_kernel as by the per-block atomics: from a start of the
    gradient's own magnitude the result is the start plus the fp64 gradient."""
    p = Problem(333, cols, seed=12)
    _, mean, rstd = _forward(p)
    gx, gg, gb = p.bwd_ref()
    dg0 = _rand(cols, seed=13, scale=gg.abs().max().item())
    db0 = _rand(cols, seed=14, scale=gb.abs().max().item())
    _, _, dg, db = _backward(p, mean, rstd, ws=ws, dg0=dg0, db0=db0)
    assert rel(dg, dg0.double() + gg) < 1e-5 and rel(db, db0.double() + gb) < 1e-5


# --------------------------------------------------------------------------------- large mean
@pytest.mark.parametrize("cols", [192, 768])
def test_large_mean(cols):
    """x = randn + 1000: the variance must not be computed as E[x^2] - mean^2.  The bound on y, rstd and dx
    is 3 x the distance of torch's own f32 CPU layer_norm (another implementation, hence the factor) from
    the fp64 result on the same input.  Measured on the CPU, as max |error| / max |reference|:
    cols 192: y 3.0e-5, rstd 1.2e-5, dx 1.5e-5;  cols 768: y 3.1e-5, rstd 7.4e-6, dx 1.6e-5 (the bounds are
    three times these)."""
    p = Problem(333, cols, seed=15, shift=1000.0)
    yr, mr, rr = p.fwd_ref()
    gx = p.bwd_ref()[0] + p.dres.double()
    y32, _, r32 = p.fwd_ref(F32)
    gx32 = p.bwd_ref(F32, F32)[0] + p.dres
    ty, tr, tdx = 3 * rel(y32, yr), 3 * rel(r32, rr), 3 * rel(gx32, gx)
    y, mean, rstd = _forward(p, kernel=KERNEL[cols])
    dx = _backward(p, mean, rstd, kernel=KERNEL[cols])[0]
    print(f"\ncols {cols}: y {rel(y, yr):.2e} / {ty:.2e}, rstd {rel(rstd, rr):.2e} / {tr:.2e}, "
          f"dx {rel(dx, gx):.2e} / {tdx:.2e}, mean {rel(mean, mr):.2e}")
    assert rel(mean, mr) < 1e-5
    assert rel(y, yr) < ty and rel(rstd, rr) < tr and rel(dx, gx) < tdx
