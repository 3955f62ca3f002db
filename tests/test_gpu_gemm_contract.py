"""vs_gemm's documented contract (include/vspike.h) on every dispatch path.

C = epilogue(alpha * A B) with the eleven VS_EPI_* bits, free leading dimensions for C and every
epilogue operand, f32 or bf16 C and a_rowsum, checked against ONE fp64 reference of the epilogue written
from the header's text (`_epi_ref`), at the smallest shape that reaches each of vs_gemm's dispatch paths.
Every call asserts through the dispatch counters which path ran, so a later change of the dispatch
conditions fails here instead of silently testing another kernel.

Operands are rounded to the operand dtype first and the reference works on those values (the convention
of test_gpu_ops.py).  Bounds, as max |error| / max |reference|: 1e-5 for an f32 C (f32 accumulation),
2e-5 for split-K accumulation (ATOMIC), 8e-3 for a bf16 C or a bf16 aux_out (one rounding), 1.5e-2 for
the GELU' product into a bf16 C: the bounds test_gpu_ops.py applies to the same epilogues.  The one
combination without a precedent there (bf16 operands, GELU, f32 C) takes its bound from the reference
itself, see test_scalar_epilogue.
"""
import math
from dataclasses import dataclass

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32

BIAS, GELU, RELU, RESIDUAL, POS = 0x1, 0x2, 0x4, 0x8, 0x10
GELU_BWD, RELU_BWD, ATOMIC, ACCUM, GELU_GRAD, MUL_AUX = 0x20, 0x40, 0x80, 0x100, 0x200, 0x400
AUX_IN = GELU_BWD | RELU_BWD | MUL_AUX
SENTINEL = -777.0


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vspike import _lib as L
    L.lib()
    assert (L.EPI_BIAS, L.EPI_GELU, L.EPI_RELU, L.EPI_RESIDUAL, L.EPI_POS, L.EPI_GELU_BWD, L.EPI_RELU_BWD, L.EPI_ATOMIC,
            L.EPI_ACCUM, L.EPI_GELU_GRAD, L.EPI_MUL_AUX) == (BIAS, GELU, RELU, RESIDUAL, POS, GELU_BWD, RELU_BWD, ATOMIC,
                                                            ACCUM, GELU_GRAD, MUL_AUX)


# --------------------------------------------------------------------------------- the reference
def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _epi_ref(A, B, flags, *, op_dtype, alpha=1.0, bias=None, pos=None, aux_in=None, residual=None, c_prev=None,
             wd=torch.float64):
    """The epilogue of include/vspike.h in the header's order, in the working dtype `wd` (fp64: the
    reference; f32: the second evaluation a derived bound is taken from).  A [M, K], B [K, N] and every
    operand hold values already rounded to their storage dtype.  Returns (C, aux_out) before the rounding
    of the store.
      1. alpha * (A B)   2. + bias[n]   3. + pos[m % pos_rows, n]
      4. GELU_BWD: * gelu'(aux_in);  RELU_BWD: aux_in > 0 ? v : 0;  MUL_AUX: * aux_in
      5. GELU: aux_out = v (GELU_GRAD: gelu'(x)), v = gelu(x), x = v rounded to bf16 for bf16 operands
         ("the value the backward will see")
      6. RELU   7. + residual   8. ACCUM: + the previous C
      9. ATOMIC: C += v, the bias added once; with RELU, C = relu(C + v)."""
    c = lambda t: t.to(wd)  # noqa: E731
    v = alpha * (c(A) @ c(B))
    aux_out = None
    if flags & BIAS:
        v = v + c(bias)
    if flags & POS:
        v = v + c(pos)[torch.arange(v.shape[0], device=v.device) % pos.shape[0]]
    if flags & GELU_BWD:
        v = v * _gelu_grad(c(aux_in))
    if flags & RELU_BWD:
        v = torch.where(c(aux_in) > 0, v, torch.zeros_like(v))
    if flags & MUL_AUX:
        v = v * c(aux_in)
    if flags & GELU:
        x = v.to(F32).to(BF).to(wd) if op_dtype == BF else v
        aux_out = _gelu_grad(x) if flags & GELU_GRAD else v
        v = _gelu(x)
    if flags & ATOMIC:
        v = c(c_prev) + v
        return (v.clamp_min(0) if flags & RELU else v), None
    if flags & RELU:
        v = v.clamp_min(0)
    if flags & RESIDUAL:
        v = v + c(residual)
    if flags & ACCUM:
        v = v + c(c_prev)
    return v, aux_out


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _tol(flags, op_dtype, out_dtype):
    """The precedent bounds of test_gpu_ops.py (module docstring); None where there is none."""
    if flags & ATOMIC:
        return 2e-5
    if out_dtype == BF:
        return 1.5e-2 if flags & GELU_BWD else 8e-3
    if flags & GELU and op_dtype == BF:
        return None
    return 1e-5


# --------------------------------------------------------------------------------- operands
def _vals(shape, seed, dtype=F32, scale=1.0, grid=0):
    """Random values rounded to `dtype`, as f32 on the CPU.  grid > 0: multiples of 1 / grid in [-1, 1]
    (exact in bf16, and their K-term dot products are exact in f32 in any order)."""
    g = torch.Generator().manual_seed(seed)
    if grid:
        return torch.randint(-grid, grid + 1, shape, generator=g).float() * (scale / grid)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).float()


class _Buf:
    """A [R, C] device tensor `t` with row stride ld >= C that starts `offset` elements into a 16-byte
    aligned allocation; everything around the values holds `fill` (NaN for inputs, a sentinel for outputs).
    `slack` elements follow, so that a kernel that mixed two leading dimensions up stays inside."""

    def __init__(self, vals, ld, dtype, fill, offset=0, slack=0):
        R, C = vals.shape
        self.buf = torch.full((offset + R * ld + slack + 8,), fill, dtype=dtype, device=DEV)
        self.full = self.buf[offset:offset + R * ld].view(R, ld)
        self.t = self.full[:, :C]
        self.vals, self.ld, self.C = vals.to(dtype), ld, C
        self.reset()

    def reset(self):
        self.t.copy_(self.vals)
        self.snap = self.buf.clone()

    def outside_untouched(self):
        a, b = self.buf.clone(), self.snap.clone()
        for x in (a, b):
            x[self.full.storage_offset():self.full.storage_offset() + self.full.numel()].view_as(self.full)[:, :self.C] = 0
        return torch.equal(a, b)


@dataclass
class Pads:
    ab: int = 0          # lda, ldb above the contiguous extent
    c: int = 0           # ldc - N
    res: int = 0
    aux_in: int = 0
    aux_out: int = 0
    misalign: int = 0    # bias, residual, aux_in and aux_out start this many elements past a 16-byte boundary


class Case:
    """One vs_gemm problem: operands on the device (padded as asked), run() and the fp64 reference."""

    def __init__(self, M, N, K, dtype, flags=0, *, out_dtype=F32, akc=True, bkc=True, pads=Pads(), pos_rows=0,
                 rowsum=False, workspace=False, seed=0, grid=0):
        from vspike import ops
        self.M, self.N, self.K, self.dtype, self.out_dtype, self.flags = M, N, K, dtype, out_dtype, flags
        self.akc, self.bkc, self.pos_rows = akc, bkc, pos_rows
        s = 100 * seed
        self.A = _vals((M, K), s + 1, dtype, grid=grid).to(DEV)
        self.B = _vals((K, N), s + 2, dtype, scale=0.5 if grid else K ** -0.5, grid=2 * grid).to(DEV)
        nan = float("nan")
        slack = M * 32
        self.a = _Buf(self.A if akc else self.A.t(), (K if akc else M) + pads.ab, dtype, nan)
        self.b = _Buf(self.B.t() if bkc else self.B, (K if bkc else N) + pads.ab, dtype, nan)
        prev = flags & (ACCUM | ATOMIC)
        self.C0 = _vals((M, N), s + 3).to(DEV) if prev else None
        self.c = _Buf(self.C0 if prev else torch.full((M, N), nan), N + pads.c, out_dtype, SENTINEL, slack=slack)
        self.kw = {}
        self.bias = self.pos = self.aux_in = self.residual = self.aux_out = self.rowsum = None
        if flags & BIAS:        # the magnitude of the product: an alpha applied to it would show
            self.bias = _vals((1, N), s + 4).to(DEV)
            self.kw["bias"] = _Buf(self.bias, N, F32, nan, offset=pads.misalign).t[0]
        if flags & POS:
            self.pos = _vals((pos_rows, N), s + 5).to(DEV)
            self.kw.update(pos=_Buf(self.pos, N, F32, nan).t, pos_rows=pos_rows)
        if flags & AUX_IN:
            self.aux_in = _vals((M, N), s + 6, dtype).to(DEV)
            self._aux_in = _Buf(self.aux_in, N + pads.aux_in, dtype, nan, offset=pads.misalign, slack=slack)
            self.kw.update(aux_in=self._aux_in.t, ld_aux_in=self._aux_in.ld)
        if flags & RESIDUAL:
            self.residual = _vals((M, N), s + 7).to(DEV)
            self._res = _Buf(self.residual, N + pads.res, F32, nan, offset=pads.misalign, slack=slack)
            self.kw.update(residual=self._res.t, ld_residual=self._res.ld)
        if flags & GELU:
            self.aux_out = _Buf(torch.full((M, N), nan), N + pads.aux_out, dtype, SENTINEL, offset=pads.misalign,
                                slack=slack)
            self.kw.update(aux_out=self.aux_out.t, ld_aux_out=self.aux_out.ld)
        if rowsum:
            self.RS0 = _vals((1, M), s + 8).to(DEV)
            self.rowsum = _Buf(self.RS0, M, F32, SENTINEL)
            self.kw["a_rowsum"] = self.rowsum.t[0]
        if workspace:
            nb = ops.splitk_workspace_bytes(dtype, M, N, K)
            assert nb > 0
            self.kw["workspace"] = torch.empty(nb // 4 + 64, device=DEV)

    def run(self, alpha=1.0, path=None, **over):
        """One vs_gemm call on freshly initialised outputs.  `path`: the dispatch counter that must read 1
        (every other one 0); a callable gets the non-zero counters instead."""
        from vspike import ops, _lib as L
        for buf in (self.c, self.aux_out, self.rowsum):
            if buf is not None:
                buf.reset()
        L.dispatch_reset()
        kw = dict(M=self.M, N=self.N, K=self.K, a_kcontig=self.akc, b_kcontig=self.bkc, lda=self.a.ld, ldb=self.b.ld,
                  ldc=self.c.ld, epilogue=self.flags, alpha=alpha, **self.kw)
        kw.update(over)
        ops.gemm(self.a.t, self.b.t, self.c.t, **kw)
        torch.cuda.synchronize()
        counts = {k: v for k, v in L.dispatch_counts().items() if v}
        if callable(path):
            path(counts)
        elif path is not None:
            assert counts == {path: 1}, (counts, path)
        for buf in (self.c, self.aux_out, self.rowsum):   # pad columns and surroundings bit-identical
            assert buf is None or buf.outside_untouched(), "a store outside the [M, N] extent"
        return self.c.t.clone()

    def ref(self, alpha=1.0, wd=torch.float64, device=DEV):
        mv = lambda t: None if t is None else t.to(device)  # noqa: E731
        return _epi_ref(mv(self.A), mv(self.B), self.flags, op_dtype=self.dtype, alpha=alpha, bias=mv(self.bias),
                        pos=mv(self.pos), aux_in=mv(self.aux_in), residual=mv(self.residual), c_prev=mv(self.C0), wd=wd)

    def check(self, out, alpha=1.0, tol=None):
        ref, aux_ref = self.ref(alpha)
        tol = _tol(self.flags, self.dtype, self.out_dtype) if tol is None else tol
        err = rel(out, ref)
        assert err < tol, (err, tol)
        if aux_ref is not None:
            aerr = rel(self.aux_out.t, aux_ref)
            assert aerr < (1e-5 if self.dtype == F32 else 8e-3), aerr
        if self.rowsum is not None:      # += sum_k A(m, k): not scaled by alpha
            rerr = rel(self.rowsum.t[0], self.RS0[0].double() + self.A.double().sum(1))
            assert rerr < 2e-5, rerr
        return err


# --------------------------------------------------------------------------------- the dispatch paths
@dataclass
class Path:
    name: str                 # dispatch counter
    shape: tuple              # the smallest (M, N, K) that reaches it
    dtype: torch.dtype = BF
    akc: bool = True
    bkc: bool = True
    knob: tuple = None
    base: tuple = (0, F32)    # (epilogue, C dtype) of the alpha-scaling check
    epis: tuple = ()          # (epilogue, C dtype) the dispatcher admits here, checked against _epi_ref
    special: bool = True      # needs 16-byte aligned rows of C (an unaligned ldc leaves the path)
    dense_c: bool = False     # needs ldc == N
    workspace: bool = False
    rowsum: bool = False

    @property
    def id(self):
        lay = "" if (self.akc and self.bkc) else f"-{'k' if self.akc else 'm'}{'k' if self.bkc else 'n'}"
        return f"{self.name}-{'x'.join(map(str, self.shape))}-{'bf16' if self.dtype == BF else 'f32'}{lay}"

    def case(self, epi=None, **kw):
        flags, out_dtype = self.base if epi is None else epi
        kw.setdefault("pos_rows", 7 if flags & POS else 0)
        return Case(*self.shape, self.dtype, flags, out_dtype=out_dtype, akc=self.akc, bkc=self.bkc,
                    workspace=self.workspace, rowsum=self.rowsum, **kw)


GENERIC = ((BIAS | RESIDUAL, F32), (BIAS | GELU, BF), (MUL_AUX, BF))
_tile = dict(special=False, epis=GENERIC + ((GELU_BWD, F32),))
PATHS = (
    [Path("gemm_f32", (200, 136, 72), F32, akc, bkc, special=False,
          epis=((BIAS | RESIDUAL, F32), (BIAS | GELU, F32), (GELU_BWD, F32)))
     for akc in (True, False) for bkc in (True, False)] +
    # K % 64 != 0: the register-staged tiles, BM x BN = 64 x 64, 64 x 128, 128 x 64, 128 x 128
    [Path("gemm_tile", s, **_tile) for s in ((40, 64, 72), (40, 136, 72), (200, 64, 72), (200, 136, 72))] +
    [Path("gemm_fullk", (300, 192, K), special=False, epis=GENERIC) for K in (64, 128, 192)] +
    [Path("gemm_ring", s, **_tile) for s in ((200, 136, 256), (40, 72, 256))] +
    [Path("gemm_panel", (300, 192, 128), base=(GELU_BWD, F32), epis=((GELU_BWD, F32), (GELU_BWD, BF)))] +
    [Path("gemm_slab", (8192, N, 192), epis=((BIAS, BF), (BIAS | RESIDUAL, F32), (BIAS | POS, F32)))
     for N in (64, 128, 192)] +
    [Path("gemm_wslab", (8192, 256, K), base=(MUL_AUX, F32), epis=((GELU_BWD, BF), (MUL_AUX, BF), (MUL_AUX, F32)))
     for K in (64, 128, 192)] +
    [Path("gemm_wres", (8192, 384, 192), base=(0, BF),
          epis=((BIAS, BF), (BIAS | GELU, BF), (BIAS | GELU | GELU_GRAD, BF)))] +
    [Path("gemm_big", (4096, 512, 512), epis=((BIAS | RESIDUAL, F32), (BIAS | GELU, BF), (BIAS | POS, F32)))] +
    [Path("gemm_g256", (16384, 256, 256), knob=("g256", 1),
          epis=((BIAS | RESIDUAL, F32), (BIAS | GELU | GELU_GRAD, BF), (MUL_AUX, BF), (GELU_BWD, BF)))] +
    [Path("gemm_skinny", s, base=(ATOMIC, F32), epis=((ATOMIC | BIAS, F32), (ATOMIC | BIAS | RELU, F32)),
          dense_c=True, workspace=True) for s in ((5, 48, 3200), (40, 16, 2144))] +
    [Path("gemm_dw", (104, 40, 5000), akc=False, bkc=False, base=(ATOMIC, F32), epis=((ATOMIC, F32),), special=False,
          workspace=True, rowsum=True)] +
    [Path("gemm_dw256", (256, 256, 4096), akc=False, bkc=False, knob=("dw256_all", 1), base=(ATOMIC, F32),
          epis=((ATOMIC, F32),), workspace=True, rowsum=True)])
UNIT_ALPHA_ONLY = ("gemm_skinny", "gemm_dw", "gemm_dw256")   # kernels without an alpha: the dispatcher keeps them for 1.0
_paths = pytest.mark.parametrize("p", PATHS, ids=[p.id for p in PATHS])


def _generic_only(p):
    """The call left path p for a generic kernel (the 256 x 256 dW product may land on the dW tiles)."""
    allowed = {"gemm_tile", "gemm_ring", "gemm_fullk", "gemm_f32"} | ({"gemm_dw"} if p.name == "gemm_dw256" else set())

    def check(counts):
        assert sum(counts.values()) == 1 and set(counts) <= allowed, (counts, p.name)
    return check


def test_every_path_is_in_the_table():
    names = {p.name for p in PATHS}
    assert names == {"gemm_f32", "gemm_tile", "gemm_fullk", "gemm_ring", "gemm_panel", "gemm_slab", "gemm_wslab",
                     "gemm_wres", "gemm_big", "gemm_g256", "gemm_skinny", "gemm_dw", "gemm_dw256"}
    assert sum(p.name == "gemm_tile" for p in PATHS) == 4 and sum(p.name == "gemm_f32" for p in PATHS) == 4


# --------------------------------------------------------------------------------- 1. alpha
@_paths
def test_alpha_power_of_two_is_exact(p, knobs):
    """C(alpha) == alpha * C(1) bitwise for alpha in {0.5, -2}: scaling by a power of two is exact in f32
    and in bf16, through the linear epilogues too (MUL_AUX / GELU_BWD where a path admits nothing else).
    The split-K kernels that carry no alpha (skinny, dW, dW 256 x 256) must hand another alpha to the
    generic tiles: there C is C0 + alpha A B within the split-K bound, and a_rowsum stays unscaled."""
    if p.knob:
        knobs(*p.knob)
    case = p.case()
    c1 = case.run(1.0, path=p.name)
    case.check(c1)
    for alpha in (0.5, -2.0):
        if p.name in UNIT_ALPHA_ONLY:
            ca = case.run(alpha, path=_generic_only(p))
            case.check(ca, alpha)
        else:
            ca = case.run(alpha, path=p.name)
            assert torch.equal(ca.float(), alpha * c1.float()), (alpha, rel(ca.float(), alpha * c1.float()))


@_paths
def test_alpha_with_epilogue(p, knobs):
    """alpha = 0.3 under every epilogue the path admits, against _epi_ref: alpha scales the product only
    (the bias has the product's magnitude, so a scaled bias is an error of order one); the ATOMIC paths
    start from a non-zero C and give C0 + alpha A B (+ bias once) through the workspace."""
    if p.knob:
        knobs(*p.knob)
    for epi in p.epis:
        case = p.case(epi, seed=1)
        if p.name in UNIT_ALPHA_ONLY:
            if epi[0] & RELU:      # ATOMIC | RELU exists on the skinny kernel only: rejected with another alpha
                from vspike import _lib as L
                with pytest.raises(L.VsError):
                    case.run(0.3)
                assert torch.equal(case.c.t, case.C0)
                case.check(case.run(1.0, path=p.name))
                continue
            case.check(case.run(0.3, path=_generic_only(p)), 0.3)
        else:
            case.check(case.run(0.3, path=p.name), 0.3)


# --------------------------------------------------------------------------------- 2. leading dimensions
@_paths
def test_padded_leading_dimensions(p, knobs):
    """C, residual, aux_in and aux_out as column slices of wider tensors (each with its own leading
    dimension), lda / ldb above the contiguous extent.  A pad that keeps rows 16-byte aligned must stay on
    the path; ldc = N + 1 must leave the vector paths for a generic one and still be right.  Input pads
    hold NaN; output pads hold a sentinel and must be bit-identical afterwards (Case.run).  The skinny kernel
    takes a dense C only (padded A and B stay on it); ATOMIC | RELU, which no other kernel has, is then
    rejected."""
    if p.knob:
        knobs(*p.knob)
    N = p.shape[1]
    for epi in p.epis:
        cpad = 0 if p.dense_c else 8
        case = p.case(epi, seed=2, pads=Pads(ab=8, c=cpad, res=16, aux_in=24, aux_out=16))
        case.check(case.run(path=p.name))
        case = p.case(epi, seed=2, pads=Pads(ab=8, c=1, res=16, aux_in=24, aux_out=16))
        assert case.c.ld == N + 1
        if epi[0] & ATOMIC and epi[0] & RELU:    # only the skinny kernel has ATOMIC | RELU, and it needs a dense C
            _rejected(case)
            continue
        case.check(case.run(path=_generic_only(p) if (p.special or p.dense_c) else p.name))


# --------------------------------------------------------------------------------- 3. the scalar epilogue
SCALAR_FLAGS = [0, BIAS, BIAS | POS, BIAS | GELU, BIAS | GELU | GELU_GRAD, RELU, BIAS | RESIDUAL, GELU_BWD, RELU_BWD,
                MUL_AUX, BIAS | RELU | RESIDUAL, ACCUM, ACCUM | BIAS | RESIDUAL]


SCALAR_CASES = [(o, f) for f in SCALAR_FLAGS for o in (F32, BF) if not (f & ACCUM and o == BF)]


@pytest.mark.parametrize("out_dtype,flags", SCALAR_CASES,
                         ids=[f"c_{'f32' if o == F32 else 'bf16'}-epi{f:#05x}" for o, f in SCALAR_CASES])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(200, 100, 72), (72, 36, 128)], ids=["N100", "N36"])
def test_scalar_epilogue(shape, dtype, out_dtype, flags):
    """store_tile's per-element epilogue (epi_one), which runs when an operand is not 16-byte aligned and on
    a ragged last column group (N % 8 != 0): N in {100, 36} with K-contiguous B, bias, residual, aux_in and
    aux_out one element past a 16-byte boundary (C stays aligned: an epilogue without operands then mixes
    vector groups with the scalar last one), every flag of the header, f32 and bf16 operands and C, against the
    reference the vector path is held to.  (200, 100, 72) runs gemm_tile / gemm_f32, (72, 36, 128)
    gemm_fullk / gemm_f32.

    A and B are multiples of 1/4 and 1/8 here: A B is then exact in f32 in any summation order, so the
    second, f32 evaluation of _epi_ref rounds the same pre-activation to bf16 as the kernel does.
    bf16 operands with GELU into an f32 C have no bound in test_gpu_ops.py; theirs is 3 x the distance of
    that f32 CPU evaluation (f32 accumulation, the documented bf16 rounding of the GELU argument) from the
    fp64 one.  Measured on the CPU: distance 5.0e-8 (N100) and 4.4e-8 (N36) of max |ref| for BIAS|GELU and
    the same with GELU_GRAD, so the bounds are 1.5e-7 and 1.3e-7: no pre-activation of these inputs lies
    within f32 rounding of a bf16 tie, and what remains is the f32 rounding of the GELU itself.
    ACCUM with a bf16 C is not a case here: vs_gemm rejects it (test_accum_needs_f32_c)."""
    M, N, K = shape
    case = Case(M, N, K, dtype, flags, out_dtype=out_dtype, pads=Pads(misalign=1), pos_rows=7 if flags & POS else 0,
                seed=3, grid=4)
    path = "gemm_f32" if dtype == F32 else ("gemm_tile" if K % 64 else "gemm_fullk")
    out = case.run(path=path)
    tol = _tol(flags, dtype, out_dtype)
    if tol is None:
        r64, _ = case.ref(device="cpu")
        r32, _ = case.ref(wd=F32, device="cpu")
        tol = 3 * rel(r32, r64)
        print(f"\nderived bound {tol:.3e} (3 x f32-CPU distance)")
    print(f"\nerr {case.check(out, tol=tol):.3e} tol {tol:.1e}")


# --------------------------------------------------------------------------------- 4. ACCUM
ACCUM_PATHS = [p for p in PATHS if p.name in ("gemm_tile", "gemm_fullk", "gemm_ring") or
               (p.name == "gemm_f32" and p.akc and p.bkc)]


@pytest.mark.parametrize("flags", [ACCUM, ACCUM | BIAS | RESIDUAL, ACCUM | RELU], ids=["accum", "bias_res", "relu"])
@pytest.mark.parametrize("p", ACCUM_PATHS, ids=[p.id for p in ACCUM_PATHS])
def test_accum(p, flags):
    """VS_EPI_ACCUM (C += v, plain read-modify-write) on the four kinds of kernel the dispatcher lets it
    reach, alone, after RELU and with BIAS | RESIDUAL; C starts from values of the product's magnitude."""
    case = p.case((flags, F32), seed=4)
    case.check(case.run(path=p.name))
    case.check(case.run(0.3, path=p.name), 0.3)


def _rejected(case, **over):
    from vspike import _lib as L
    before = case.c.buf.clone()
    with pytest.raises(L.VsError):
        case.run(path={}, **over)
    torch.cuda.synchronize()
    assert not any(L.dispatch_counts().values()), L.dispatch_counts()
    assert torch.equal(case.c.buf.view(torch.int32 if case.out_dtype == F32 else torch.int16),
                       before.view(torch.int32 if case.out_dtype == F32 else torch.int16))


def test_accum_needs_f32_c():
    _rejected(Case(200, 136, 72, BF, ACCUM, out_dtype=BF))


# --------------------------------------------------------------------------------- 5. every flag on tile / ring
TILE_RING = [p for p in PATHS if p.name in ("gemm_tile", "gemm_ring")]
ALL_FLAGS = {"bias": (BIAS, F32), "pos": (BIAS | POS, F32), "gelu": (BIAS | GELU, BF),
             "gelu_grad": (BIAS | GELU | GELU_GRAD, BF), "relu": (BIAS | RELU, F32), "residual": (RESIDUAL, F32),
             "gelu_bwd": (GELU_BWD, F32), "gelu_bwd_bf16": (GELU_BWD, BF), "relu_bwd": (RELU_BWD, F32),
             "mul_aux": (MUL_AUX, F32), "relu_res_bf16": (BIAS | RELU | RESIDUAL, BF), "rowsum": (0, F32)}


@pytest.mark.parametrize("epi", sorted(ALL_FLAGS))
@pytest.mark.parametrize("layout", ["kk", "mn"])
@pytest.mark.parametrize("p", TILE_RING, ids=[p.id for p in TILE_RING])
def test_every_flag_on_tile_and_ring(p, layout, epi):
    """Each epilogue bit on the vector epilogue (epi_eight) of gemm_tile in its four BM x BN instantiations
    and of gemm_ring in both, which test_gpu_ops.py reaches with epilogue 0 only: POS with pos_rows = 7
    (not a divisor of M), GELU with both aux_out contents, both masks, MUL_AUX, and a_rowsum accumulating
    onto a non-zero start.  Both operand layouts: K-contiguous (forward) and M / N-contiguous (dW)."""
    M, N, K = p.shape      # every extent of these shapes is a multiple of 8: both layouts are legal
    kc = layout == "kk"
    flags, out_dtype = ALL_FLAGS[epi]
    case = Case(M, N, K, BF, flags, out_dtype=out_dtype, akc=kc, bkc=kc, pos_rows=7 if flags & POS else 0,
                rowsum=epi == "rowsum", seed=5)
    case.check(case.run(path=p.name))


# --------------------------------------------------------------------------------- 6. rejections
def test_rejections_launch_nothing():
    """Argument errors vs_gemm must refuse with VS_EINVAL before any launch: no dispatch counter moves and C
    keeps its bits."""
    _rejected(Case(40, 64, 4096, BF, ATOMIC | GELU))                        # ATOMIC combines with BIAS (RELU) only
    _rejected(Case(200, 136, 256, BF, 0), split_k=4)                        # split_k > 1 without ATOMIC
    _rejected(Case(200, 136, 72, BF, 0), ldc=128)                           # ldc < N
    _rejected(Case(200, 136, 72, BF, 0, pads=Pads(ab=4)))                   # lda = 76 bf16: not 16 bytes
    _rejected(Case(200, 136, 72, F32, 0, pads=Pads(ab=2)))                  # lda = 74 f32
    _rejected(Case(200, 136, 256, BF, ATOMIC | RELU))                       # ATOMIC | RELU off the skinny path
    _rejected(Case(200, 136, 72, BF, MUL_AUX), aux_in=None)                 # MUL_AUX reads aux_in
