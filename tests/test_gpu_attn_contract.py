"""The contract of the head-dim-64 attention entries vs_attn_fwd / vs_attn_bwd (csrc/attn_fwd.hip, attn_bwd.hip), at op level.

Reference and bars.  tests/attn_ref.py holds the float64 reference and a rounding model of the bf16 kernels (the
same float64 arithmetic with the kernels' documented bf16 roundings); tests/test_cpu_attn_contract.py checks both
without a GPU.  Every statistic here is per (batch, head): the worst row's max-abs error over that head's own
max|ref|, for each of o, lse, dQ, dK, dV.
  f32 kernels: at most 1e-5 (o, lse) / 2e-5 (gradients), the bars of tests/test_gpu_ops.py, now per head.
  bf16 kernels: at most TWICE what the rounding model itself gives for the same head and tensor (the margin the
    project uses for its rounding models), and, as a second, looser assertion, the whole-tensor
    bars of tests/test_gpu_ops.py (1.5e-2 o, 3e-3 lse, 3e-2 gradients).
  One head can have a reference that is exactly zero: dQ and dK at N = 1 (dS = 0).  The model gives exactly zero
    there too, the kernels what two differently ordered f32 sums of the same products leave; those heads (and only
    those) are held to attn_ref.cancel_floor, a bound on that remainder from the f32 format alone.
No number here was taken from the kernels.  Each case prints its kernel / model ratios ("attn-contract ..." lines;
the ladder's are recorded in profiles/attn_contract_ratios.txt).

Frames.  Every operand is a view into a larger buffer of NaN or 3.0e4: 8 rows before and after, pad columns to the
right, each operand with its own pad so that ld_qkv, ld_o, ld_do, ld_dqkv all differ from each other and from the
contiguous 3D / D (bf16: the smallest increments the entries admit, +8, +8 -> +16 for dout to differ from o, +4 for
dqkv; f32: odd ones, 3D + 1).  lse sits inside a filled buffer and the workspace is exactly
vs_attn_bwd_workspace_bytes long between two filled guards.  After a forward + backward the fill is intact, the
inputs (and o, lse across the backward) are bit-identical, and the outputs are bit-identical to the same call on
contiguous tensors (which keep the pad rows, lse edges and workspace guards, checked the same way, and drop only
the pad columns).  With B = 2, H = 2 the rows "past N" of batch 0 are batch 1's rows and every head has a
neighbour's columns beside it.

Knob values (VS_KNOB_ATTN_VARIANT = backward << 4 | forward): 0x00 default forward + the backward's own pick, 0x96
forward 6 + backward 9, 0x67 forward 7 + backward 6, 0x98 forward 8 + backward 9 -- every forward (0, 6, 7, 8) and
backward (6, 9) variant meets every shape.
"""
import math

import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
FILLS = (NAN, 3.0e4)
CONFIGS = [(BF16, 0x00), (BF16, 0x96), (BF16, 0x67), (BF16, 0x98), (F32, 0)]
FORCED = [(BF16, 0x66), (BF16, 0x96), (BF16, 0x67), (BF16, 0x98), (F32, 0)]      # no pick left to the grid size
cfg_id = lambda c: ("bf16-%02x" % c[1]) if c[0] == BF16 else "f32"      # noqa: E731
PADS = {BF16: dict(qkv=8, o=8, do=16, dqkv=4), F32: dict(qkv=1, o=1, do=2, dqkv=3)}
PAD_ROWS, LSE_EDGE, WS_GUARD = 8, 256, 64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------------------
# cases: inputs, float64 reference and rounding model, computed once and shared
# ------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, B, N, H, dtype, scale, seed, extreme=False):
        self.B, self.N, self.H, self.dtype, self.scale = B, N, H, dtype, scale
        if extreme:
            self.qkv, self.dout = R.make_extreme_inputs(B, N, H, seed, dtype)
        else:
            self.qkv, self.dout = R.make_inputs(B, N, H, seed, dtype, scale)
        self.ref = R.reference(self.qkv, self.dout, B, N, H, scale)
        self.model = None
        if dtype == BF16:       # the backward model consumes the forward model's O and f32 lse, as training does
            o_m, lse_m = R.model_fwd(self.qkv, B, N, H, scale, safe=extreme)
            self.model = (o_m, lse_m, R.model_bwd(self.qkv, o_m, lse_m.float(), self.dout, B, N, H, scale))


_CASES = {}


def case(B, N, H, dtype, scale=0.125, seed=None, extreme=False):
    key = (B, N, H, dtype, scale, seed, extreme)
    if key not in _CASES:
        _CASES[key] = Case(B, N, H, dtype, scale, N if seed is None else seed, extreme)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------------------
def framed(rows, cols, dtype, fill, pad_cols, pad_rows, src=None):
    """A [rows, cols] view (leading dimension cols + pad_cols) inside a buffer of `fill`; (view, buffer)."""
    buf = torch.full((rows + 2 * pad_rows, cols + pad_cols), fill, dtype=dtype, device=DEV)
    view = buf[pad_rows:pad_rows + rows, :cols]
    if src is not None:
        view.copy_(src)
    return view, buf


def is_fill(t, fill):
    want = torch.tensor(fill, dtype=t.dtype).item()           # 3.0e4 is 29952 in bf16
    return bool(torch.isnan(t).all()) if math.isnan(fill) else bool((t == want).all())


def frame_untouched(buf, rows, cols, fill, pad_rows):
    m = torch.ones_like(buf, dtype=torch.bool)
    m[pad_rows:pad_rows + rows, :cols] = False
    return is_fill(buf[m], fill)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


class Buffers:
    """The operands of one forward + backward inside filled surroundings; frame=False keeps the pad rows, the lse
    edges and the workspace guards but drops the pad columns: contiguous operands, minimal leading dimensions."""

    def __init__(self, c, fill=NAN, frame=True):
        from vspike import ops
        self.c, self.fill, self.frame = c, fill, frame
        B, N, H, dt = c.B, c.N, c.H, c.dtype
        M, D = B * N, H * R.DH
        self.M, self.D = M, D
        pads = PADS[dt] if frame else dict.fromkeys(PADS[dt], 0)
        self.pr = pr = PAD_ROWS
        self.edge = edge = LSE_EDGE
        self.qkv, self.qkv_buf = framed(M, 3 * D, dt, fill, pads["qkv"], pr, c.qkv)
        self.dout, self.dout_buf = framed(M, D, dt, fill, pads["do"], pr, c.dout)
        self.o, self.o_buf = framed(M, D, dt, fill, pads["o"], pr)
        self.dqkv, self.dqkv_buf = framed(M, 3 * D, dt, fill, pads["dqkv"], pr)
        self.lse_buf = torch.full((B * H * N + 2 * edge,), fill, device=DEV)
        self.lse = self.lse_buf[edge:edge + B * H * N].view(B, H, N)
        self.ws_n = ops.attn_bwd_workspace_bytes(B, N, H) // 4            # exactly that long: no slack
        self.ws_buf = torch.full((self.ws_n + 2 * WS_GUARD,), NAN, device=DEV)
        self.ws_buf[:WS_GUARD] = fill
        self.ws_buf[WS_GUARD + self.ws_n:] = fill
        self.ws = self.ws_buf[WS_GUARD:WS_GUARD + self.ws_n]
        if frame:
            lds = (self.qkv.stride(0), self.o.stride(0), self.dout.stride(0), self.dqkv.stride(0))
            assert len(set(lds) | {D, 3 * D}) == 6, lds

    def fwd(self):
        from vspike import ops
        c = self.c
        ops.attn_fwd(self.qkv, self.o, self.lse, c.B, c.N, c.H, c.scale)

    def bwd(self):
        from vspike import ops
        c = self.c
        ops.attn_bwd(self.qkv, self.o, self.dout, self.lse, self.dqkv, self.ws, c.B, c.N, c.H, c.scale)

    def outputs_untouched_outside(self):
        return {"o": frame_untouched(self.o_buf, self.M, self.D, self.fill, self.pr),
                "dqkv": frame_untouched(self.dqkv_buf, self.M, 3 * self.D, self.fill, self.pr),
                "lse": is_fill(torch.cat([self.lse_buf[:self.edge], self.lse_buf[self.edge + self.lse.numel():]]), self.fill),
                "ws": is_fill(torch.cat([self.ws_buf[:WS_GUARD], self.ws_buf[WS_GUARD + self.ws_n:]]), self.fill)}

    def outputs_all_fill(self):
        return is_fill(self.o_buf, self.fill) and is_fill(self.dqkv_buf, self.fill) and is_fill(self.lse_buf, self.fill)


def run(c, fill=NAN, frame=True, given=None):
    """Forward + backward; `given` = (o, lse) replaces the forward.  Checks what may and may not be written and
    returns (o, lse, dqkv) as contiguous copies."""
    b = Buffers(c, fill, frame)
    ins = [t.clone() for t in (b.qkv_buf, b.dout_buf)]
    if given is None:
        b.fwd()
    else:
        b.o.copy_(given[0])
        b.lse.copy_(given[1])
    mid = [t.clone() for t in (b.o_buf, b.lse_buf)]
    b.bwd()
    torch.cuda.synchronize()
    ok = b.outputs_untouched_outside()
    assert all(ok.values()), f"written outside its operand: {ok}"
    assert same_bits(b.qkv_buf, ins[0]) and same_bits(b.dout_buf, ins[1]), "the kernels changed qkv or dout"
    assert same_bits(b.o_buf, mid[0]) and same_bits(b.lse_buf, mid[1]), "the backward changed o or lse"
    out = (b.o.contiguous(), b.lse.contiguous(), b.dqkv.contiguous())
    for name, t in zip(("o", "lse", "dqkv"), out):
        assert torch.isfinite(t.float()).all(), f"{name} is not finite"
    return out


def equal_bits(a, b, what):
    for name, x, y in zip(("o", "lse", "dqkv"), a, b):
        assert torch.equal(x, y), (what, name, float((x.float() - y.float()).abs().max()))


# ------------------------------------------------------------------------------------------------------------
# bars
# ------------------------------------------------------------------------------------------------------------
def check(c, out, tag, model=None, only_grads=False):
    """Section 4's bars for one (o, lse, dqkv); returns and prints the worst kernel / model ratio per tensor."""
    B, N, H, D = c.B, c.N, c.H, c.H * R.DH
    o_ref, lse_ref, g_ref = c.ref
    model = c.model if model is None else model
    bars = R.BARS[c.dtype]
    floor = R.cancel_floor(c.qkv, c.dout, B, N, H, c.scale) if N == 1 else torch.zeros(3, B, H, dtype=torch.float64)
    items = [("dqkv", out[2], g_ref, 3, "g", 2)]
    if not only_grads:
        items = [("o", out[0], o_ref, 1, "o", 0), ("lse", out[1], lse_ref, 1, "lse", 1)] + items
    ratios, whole = {}, {}
    for name, x, ref, parts, bar, mi in items:
        err, den = R.head_err(x, ref, B, N, H, parts)
        fl = torch.where(den == 0, floor if parts == 3 else floor[2:], torch.zeros_like(den))
        names = ["dq", "dk", "dv"] if parts == 3 else [name]
        if c.dtype == F32:
            ok = err <= bars[bar] * den + fl
            assert bool(ok.all()), (tag, name, "per-head f32 bar", (err / den.clamp_min(1e-300)).tolist())
            for i, n in enumerate(names):
                ratios[n] = float((err[i] / den[i].clamp_min(1e-300)).max()) if bool((den[i] > 0).all()) else 0.0
        else:
            err_m, _ = R.head_err(model[mi], ref, B, N, H, parts)
            ok = err <= 2.0 * err_m + fl
            r = torch.where(err <= fl, torch.zeros_like(err), err / err_m.clamp_min(1e-300))
            for i, n in enumerate(names):
                ratios[n] = float(r[i].max())
            assert bool(ok.all()), (tag, name, "kernel / model per head", r.tolist(), (err / den.clamp_min(1e-300)).tolist())
        for i, n in enumerate(names):
            xs = x if parts == 1 else x[:, i * D:(i + 1) * D]
            rs = ref if parts == 1 else ref[:, i * D:(i + 1) * D]
            whole[n] = R.rel(xs.float(), rs) if float(rs.abs().max()) > 0 else float(err[i].max())
            lim = bars[bar] if float(rs.abs().max()) > 0 else float(fl[i].max())
            assert whole[n] <= lim, (tag, n, "whole-tensor bar", whole[n])
    kind = "kernel/model" if c.dtype == BF16 else "err/max|ref| per head"
    print(f"attn-contract {tag} {kind}: " + ", ".join(f"{k} {v:.4g}" for k, v in ratios.items())
          + " | whole-tensor: " + ", ".join(f"{k} {v:.2e}" for k, v in whole.items()))
    return ratios


def framed_vs_plain(c, tag, fills=(NAN,)):
    """Sections 2 and 3: framed runs (one per fill) equal each other and the contiguous call bit for bit, and the
    contiguous result is within the bars."""
    plain = run(c, frame=False)
    for fill in fills:
        equal_bits(run(c, fill), plain, f"{tag}: framed (fill {fill}) against contiguous")
    check(c, plain, tag)


# ------------------------------------------------------------------------------------------------------------
# 2. frames and leading dimensions; the tail under padded leading dimensions (both fills)
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [33, 128, 130, 257])
@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
def test_frames_and_leading_dimensions(knobs, cfg, N):
    dtype, knob = cfg
    knobs("attn_variant", knob)
    framed_vs_plain(case(2, N, 2, dtype), f"frames {cfg_id(cfg)} N={N}", FILLS)


# ------------------------------------------------------------------------------------------------------------
# 3. the N ladder: every unit of the kernels (32-row wave blocks, 64-key tiles, 128-row workgroups, pairs of
#    32-row units) at, one below and one above its edge
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", R.LADDER)
@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
def test_n_ladder(knobs, cfg, N):
    dtype, knob = cfg
    knobs("attn_variant", knob)
    framed_vs_plain(case(2, N, 2, dtype), f"ladder {cfg_id(cfg)} N={N}")


# ------------------------------------------------------------------------------------------------------------
# 5. independence, bit for bit
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [33, 130, 257])
@pytest.mark.parametrize("cfg", FORCED, ids=cfg_id)
def test_batches_are_independent(knobs, cfg, N):
    dtype, knob = cfg
    knobs("attn_variant", knob)
    B, H = 3, 2
    c = case(B, N, H, dtype)
    o, lse, g = run(c)
    for b in range(B):
        one = Case.__new__(Case)
        one.B, one.N, one.H, one.dtype, one.scale = 1, N, H, dtype, c.scale
        one.qkv, one.dout = c.qkv[b * N:(b + 1) * N], c.dout[b * N:(b + 1) * N]
        equal_bits(run(one), (o[b * N:(b + 1) * N], lse[b:b + 1], g[b * N:(b + 1) * N]), f"batch {b} alone")


@pytest.mark.parametrize("cfg", FORCED, ids=cfg_id)
def test_heads_are_independent(knobs, cfg):
    dtype, knob = cfg
    knobs("attn_variant", knob)
    B, N, H, b1, h1 = 2, 130, 3, 1, 1
    D = H * R.DH
    c = case(B, N, H, dtype)
    base = run(c)
    other = Case.__new__(Case)
    other.B, other.N, other.H, other.dtype, other.scale = B, N, H, dtype, c.scale
    other.qkv, other.dout = c.qkv.clone(), c.dout.clone()
    g = torch.Generator().manual_seed(99)
    rows = slice(b1 * N, (b1 + 1) * N)
    for part in range(3):                           # new Q, K, V of (b1, h1), some of them large
        new = torch.randn(N, R.DH, generator=g) * 2.0
        new[::7, ::5] *= 40.0
        other.qkv[rows, part * D + h1 * R.DH:part * D + (h1 + 1) * R.DH] = new.to(dtype)
    other.dout[rows, h1 * R.DH:(h1 + 1) * R.DH] = (torch.randn(N, R.DH, generator=g) * 30.0).to(dtype)
    moved = run(other)
    keep = torch.ones(B * N, D, dtype=torch.bool)
    keep[rows, h1 * R.DH:(h1 + 1) * R.DH] = False
    keep3 = keep.repeat(1, 3).to(DEV)
    keep, lkeep = keep.to(DEV), torch.ones(B, H, dtype=torch.bool, device=DEV)
    lkeep[b1, h1] = False
    assert torch.equal(base[0][keep], moved[0][keep]), "o of another head moved"
    assert torch.equal(base[1][lkeep], moved[1][lkeep]), "lse of another head moved"
    assert torch.equal(base[2][keep3], moved[2][keep3]), "dqkv of another head moved"
    assert not torch.equal(base[0][~keep], moved[0][~keep])        # the replaced head itself did change


# ------------------------------------------------------------------------------------------------------------
# 6. scale
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [130, 257])
@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
def test_scale(knobs, cfg, scale, N):
    dtype, knob = cfg
    knobs("attn_variant", knob)
    c = case(2, N, 2, dtype, scale)
    check(c, run(c), f"scale {cfg_id(cfg)} scale={scale} N={N}")


# ------------------------------------------------------------------------------------------------------------
# 7. the backward's default pick at its threshold, with twelve heads
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["below", "above"])
def test_default_backward_pick_and_twelve_heads(knobs, side):
    """bv == 0 picks the pipelined-pair kernel (6) up to 3 x CUs workgroups and the 3-wave kernel (9) beyond."""
    from vspike import _lib as L
    N, H = 33, 12
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b_lo = 3 * cus // (H * ((N + 127) // 128))                  # the last B with cdiv(N, 128) * H * B <= 3 * CUs
    B, forced, wrong = (b_lo, 0x60, 0x90) if side == "below" else (b_lo + 1, 0x90, 0x60)
    c = case(B, N, H, BF16)
    knobs("attn_variant", 0)
    L.dispatch_reset()
    auto = run(c, frame=False)
    counts = L.dispatch_counts()
    assert counts["attn_fwd"] == 1 and counts["attn_bwd"] == 1 and counts["attn_f32"] == 0, counts
    knobs("attn_variant", forced)
    equal_bits(run(c, frame=False), auto, f"default pick {side} the threshold against {forced:#x}")
    check(c, auto, f"pick {side} B={B} H={H} N={N}")
    knobs("attn_variant", wrong)
    check(c, run(c, frame=False), f"pick {side} B={B} H={H} N={N} knob {wrong:#x}", only_grads=True)


# ------------------------------------------------------------------------------------------------------------
# 8. the forward's redo pass under frames
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fv", [0, 6, 7, 8])
def test_redo_pass_under_frames(knobs, fv):
    from vspike import _lib as L
    knobs("attn_variant", fv)
    c = case(2, 321, 2, BF16, seed=6, extreme=True)     # seed: see test_cpu_attn_contract's extreme-input test
    L.attn_redo_count(reset=True)
    out = run(c)
    assert L.attn_redo_count() > 0, "the safe pass did not run"
    check(c, out, f"redo fwd={fv} N=321")


# ------------------------------------------------------------------------------------------------------------
# 9. the backward on the reference's own O and lse
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [130, 257])
@pytest.mark.parametrize("cfg", [(BF16, 0x60), (BF16, 0x90), (F32, 0)], ids=cfg_id)
def test_backward_on_reference_inputs(knobs, cfg, N):
    dtype, knob = cfg
    knobs("attn_variant", knob)
    c = case(2, N, 2, dtype)
    o_in, lse_in = c.ref[0].to(dtype), c.ref[1].float()
    model = None
    if dtype == BF16:
        model = (None, None, R.model_bwd(c.qkv, o_in, lse_in, c.dout, c.B, N, c.H, c.scale))
    out = run(c, given=(o_in.to(DEV), lse_in.to(DEV)))
    check(c, out, f"bwd-on-ref {cfg_id(cfg)} N={N}", model=model, only_grads=True)


# ------------------------------------------------------------------------------------------------------------
# 10. refusals
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_refusals_write_nothing_and_count_nothing(dtype):
    from vspike import _lib as L
    c = case(2, 33, 2, dtype)
    b = Buffers(c, 3.0e4)
    b.ws_buf.fill_(3.0e4)
    es = 2 if dtype == BF16 else 4
    code = L.dtype_code(dtype)
    base = dict(dtype=code, B=c.B, N=c.N, H=c.H, Dh=64, qkv=b.qkv.data_ptr(), ld_qkv=b.qkv.stride(0), o=b.o.data_ptr(),
                ld_o=b.o.stride(0), dout=b.dout.data_ptr(), ld_do=b.dout.stride(0), lse=b.lse.data_ptr(),
                dqkv=b.dqkv.data_ptr(), ld_dqkv=b.dqkv.stride(0), ws=b.ws.data_ptr())

    def call(which, **kw):
        a = dict(base, **kw)
        if which == "fwd":
            rc = L.lib().vs_attn_fwd(a["dtype"], a["B"], a["N"], a["H"], a["Dh"], a["qkv"], a["ld_qkv"], a["o"], a["ld_o"],
                                     a["lse"], 0.125, L.stream())
        else:
            rc = L.lib().vs_attn_bwd(a["dtype"], a["B"], a["N"], a["H"], a["Dh"], a["qkv"], a["ld_qkv"], a["o"], a["ld_o"],
                                     a["dout"], a["ld_do"], a["lse"], a["dqkv"], a["ld_dqkv"], a["ws"], 0.125, L.stream())
        L.check(rc, "vs_attn_" + which)

    D = c.H * 64
    both = [(dict(Dh=32), "head dim must be 64"), (dict(B=0), "empty problem"), (dict(N=0), "empty problem"),
            (dict(H=0), "empty problem"), (dict(ld_qkv=3 * D - 8), "leading dims too small"),
            (dict(ld_o=D - 8), "leading dims too small"), (dict(qkv=None), "null pointer"), (dict(o=None), "null pointer"),
            (dict(lse=None), "null pointer"), (dict(dtype=L.VS_FP8), "bad dtype"), (dict(dtype=L.VS_U8), "bad dtype")]
    fwd = list(both)
    bwd = both + [(dict(ld_do=D - 8), "leading dims too small"), (dict(ld_dqkv=3 * D - 4), "leading dims too small"),
                  (dict(dout=None), "null pointer"), (dict(dqkv=None), "null pointer"), (dict(ws=None), "null pointer")]
    if dtype == BF16:       # the alignment each entry states (include/vspike.h), one element off it
        fwd += [(dict(ld_qkv=3 * D + 4), "16-byte aligned"), (dict(ld_o=D + 4), "16-byte aligned"),
                (dict(qkv=base["qkv"] + 4 * es), "16-byte aligned"), (dict(o=base["o"] + 4 * es), "16-byte aligned")]
        bwd += [(dict(ld_qkv=3 * D + 4), "16-byte aligned"), (dict(ld_do=D + 4), "16-byte aligned"),
                (dict(ld_dqkv=3 * D + 2), "16-byte aligned"), (dict(qkv=base["qkv"] + 4 * es), "16-byte aligned"),
                (dict(dout=base["dout"] + 4 * es), "16-byte aligned"), (dict(dqkv=base["dqkv"] + 2 * es), "16-byte aligned"),
                (dict(ld_o=D + 4), "o / workspace alignment"), (dict(o=base["o"] + 4 * es), "o / workspace alignment"),
                (dict(ws=base["ws"] + 8), "o / workspace alignment")]
    L.dispatch_reset()
    for which, cases in (("fwd", fwd), ("bwd", bwd)):
        for kw, msg in cases:
            with pytest.raises(L.VsError, match=msg):
                call(which, **kw)
    torch.cuda.synchronize()
    counts = L.dispatch_counts()
    assert not any(counts.values()), {k: v for k, v in counts.items() if v}
    assert b.outputs_all_fill() and is_fill(b.ws_buf, 3.0e4), "a refused call wrote to an output"
    call("fwd")                                       # the same buffers, unaltered arguments: accepted
    call("bwd")
    torch.cuda.synchronize()
    assert all(b.outputs_untouched_outside().values())
