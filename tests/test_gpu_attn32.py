"""Head-dim-32 short-sequence attention (vs_attn32_fwd / vs_attn32_bwd, csrc/attn32.hip) and the block executor's
hidden == heads * 32 route.

Reference: float64 softmax attention on the same inputs (bf16 inputs are exactly representable).  The bars are the
ones tests/test_gpu_ops.py holds the head-dim-64 kernels to, because the number formats and the places where they
round are the same: f32 sums at most 256 fmaf terms per row (1e-5 forward, 2e-5 backward, of max|ref|); the bf16
kernels round P, dS and the outputs to bf16 (2^-9 each) and take O from the forward kernel as training does (1.5e-2 on
O, 3e-3 on lse, 3e-2 on each of dQ, dK, dV).  Measured on an MI355X, worst over the shapes: f32 O 7.3e-7, lse
1.5e-7, gradients 1.3e-6; bf16 O 3.3e-3, lse 1.1e-7, gradients 7.2e-3 (dQ at N = 256).

Shapes: N = 1, a partial 16-row tile (10), a partial second 32-key step (33), exact tiles (64, 256), one row past a
64-query workgroup (65), the decoder's 82 and 197 tokens; more than one head and batch entry.  Every leading
dimension is larger than minimal and every buffer sits between NaN / large-valued rows and columns that the
kernels must neither read into a result nor overwrite.
"""
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1, 1), (2, 10, 2), (1, 33, 2), (1, 64, 1), (1, 65, 1), (2, 82, 3), (1, 197, 2), (1, 256, 1)]
FILLS = (float("nan"), 3.0e4)
BARS = {torch.float32: dict(o=1e-5, lse=1e-5, g=2e-5), torch.bfloat16: dict(o=1.5e-2, lse=3e-3, g=3e-2)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _framed(rows, cols, dtype, fill, src=None, pad_cols=16, pad_rows=8):
    """A [rows, cols] view (leading dimension cols + pad_cols) in the middle of a buffer of `fill`: `pad_rows` rows
    before and after it and `pad_cols` columns to its right.  Returns (view, whole buffer)."""
    buf = torch.full((rows + 2 * pad_rows, cols + pad_cols), fill, dtype=dtype, device=DEV)
    view = buf[pad_rows:pad_rows + rows, :cols]
    if src is not None:
        view.copy_(src)
    return view, buf


def _frame_untouched(buf, rows, cols, fill, pad_rows=8):
    m = torch.ones_like(buf, dtype=torch.bool)
    m[pad_rows:pad_rows + rows, :cols] = False
    got = buf[m].float()
    want = torch.tensor(fill, dtype=buf.dtype).float()        # 3.0e4 is 29952 in bf16
    return bool(torch.isnan(got).all()) if math.isnan(fill) else bool((got == want.to(got.device)).all())


def _attn_ref(qkv, B, N, H):
    q, k, v = qkv.view(B, N, 3, H, 32).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(32.0)
    o = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B * N, H * 32)
    return o, torch.logsumexp(s, dim=-1)


_REF = {}


def _case(shape, dtype):
    """Inputs and the float64 reference of one (shape, dtype), computed once and shared."""
    key = (shape, dtype)
    if key not in _REF:
        B, N, H = shape
        D = 32 * H
        qkv = _rand(B * N, 3 * D, seed=40 + N, scale=1.5).to(dtype)
        do = _rand(B * N, D, seed=41 + N).to(dtype)
        ref_in = qkv.double().requires_grad_()
        o_ref, lse_ref = _attn_ref(ref_in, B, N, H)
        (g_ref,) = torch.autograd.grad(o_ref, ref_in, do.double())
        _REF[key] = (qkv, do, o_ref.detach(), lse_ref.detach(), g_ref)
    return _REF[key]


def _run(shape, dtype, fill):
    from vspike import ops
    B, N, H = shape
    D = 32 * H
    qkv, do, *_ = _case(shape, dtype)
    qd, _ = _framed(B * N, 3 * D, dtype, fill, qkv)
    dd, _ = _framed(B * N, D, dtype, fill, do)
    o, obuf = _framed(B * N, D, dtype, fill)
    lse_buf = torch.full((B * H * N + 512,), fill, device=DEV)
    lse = lse_buf[256:256 + B * H * N].view(B, H, N)
    ops.attn32_fwd(qd, o, lse, B, N, H)
    dqkv, gbuf = _framed(B * N, 3 * D, dtype, fill)
    ws = torch.full((ops.attn32_bwd_workspace_bytes(B, N, H) // 4 + 64,), float("nan"), device=DEV)
    ops.attn32_bwd(qd, o, dd, lse, dqkv, ws, B, N, H)      # the backward consumes the forward's own O and lse
    torch.cuda.synchronize()
    assert _frame_untouched(obuf, B * N, D, fill) and _frame_untouched(gbuf, B * N, 3 * D, fill)
    edge = torch.cat([lse_buf[:256], lse_buf[256 + B * H * N:]])
    assert bool(torch.isnan(edge).all()) if math.isnan(fill) else bool((edge == fill).all())
    return o.clone(), lse.clone(), dqkv.clone()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attn32_against_float64_and_reruns_bitwise(shape, dtype):
    B, N, H = shape
    D = 32 * H
    _, _, o_ref, lse_ref, g_ref = _case(shape, dtype)
    runs = [_run(shape, dtype, fill) for fill in FILLS for _ in range(2)]
    o, lse, dqkv = runs[0]
    bars = BARS[dtype]
    errs = {"o": rel(o.float(), o_ref), "lse": rel(lse, lse_ref)}
    for part in range(3):
        sl = slice(part * D, (part + 1) * D)
        errs["d" + "qkv"[part]] = rel(dqkv[:, sl].float(), g_ref[:, sl])
    print(f"attn32 {shape} {dtype}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for t in (o, lse, dqkv):
        assert torch.isfinite(t.float()).all()
    assert errs["o"] < bars["o"] and errs["lse"] < bars["lse"], errs
    for part in "qkv":
        assert errs["d" + part] < bars["g"], errs
    for k, run in enumerate(runs[1:], 1):
        for name, a, b in zip(("o", "lse", "dqkv"), run, runs[0]):
            assert torch.equal(a, b), (name, k, float((a.float() - b.float()).abs().max()))


def test_attn32_refuses_long_sequences_on_the_device():
    from vspike import ops
    from vspike._lib import VsError
    B, N, H = 1, 257, 1
    qkv = torch.zeros(B * N, 96, device=DEV)
    o = torch.full((B * N, 32), 7.0, device=DEV)
    lse = torch.full((B, H, N), 7.0, device=DEV)
    with pytest.raises(VsError, match="1..256"):
        ops.attn32_fwd(qkv, o, lse, B, N, H)
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((lse == 7.0).all())


# ------------------------------------------------------------------------------------------------------------
# the block executor at hidden 64 / 2 heads
# ------------------------------------------------------------------------------------------------------------
_B, _N, _D, _H, _F = 2, 10, 64, 2, 128
_W = (("ln1_g", (_D,)), ("ln1_b", (_D,)), ("w_qkv", (3 * _D, _D)), ("b_qkv", (3 * _D,)), ("w_proj", (_D, _D)),
      ("b_proj", (_D,)), ("ln2_g", (_D,)), ("ln2_b", (_D,)), ("w_fc1", (_F, _D)), ("b_fc1", (_F,)), ("w_fc2", (_D, _F)),
      ("b_fc2", (_D,)))


def _block_params():
    P = {}
    for i, (k, shape) in enumerate(_W):
        if k.endswith("_g"):
            P[k] = 1.0 + _rand(*shape, seed=60 + i, scale=0.1)
        elif len(shape) == 2:
            P[k] = _rand(*shape, seed=60 + i, scale=1.0 / math.sqrt(shape[1]))
        else:
            P[k] = _rand(*shape, seed=60 + i, scale=0.2)
    P["b_qkv"][_D:2 * _D] = 0.0          # the key bias is not a parameter
    return P


def _cpu_block(x, P):
    """oracle.cpu_ref.vit_layer (the CPU block) on this test's parameter names, in float64."""
    from oracle import cpu_ref
    D = _D
    Q = {"layernorm_before.weight": P["ln1_g"], "layernorm_before.bias": P["ln1_b"],
         "attention.attention.query.weight": P["w_qkv"][:D], "attention.attention.query.bias": P["b_qkv"][:D],
         "attention.attention.key.weight": P["w_qkv"][D:2 * D],
         "attention.attention.value.weight": P["w_qkv"][2 * D:], "attention.attention.value.bias": P["b_qkv"][2 * D:],
         "attention.output.dense.weight": P["w_proj"], "attention.output.dense.bias": P["b_proj"],
         "layernorm_after.weight": P["ln2_g"], "layernorm_after.bias": P["ln2_b"],
         "intermediate.dense.weight": P["w_fc1"], "intermediate.dense.bias": P["b_fc1"],
         "output.dense.weight": P["w_fc2"], "output.dense.bias": P["b_fc2"]}
    cfg = types.SimpleNamespace(num_attention_heads=_H, layer_norm_eps=1e-12)
    return cpu_ref.vit_layer(x, Q, "", cfg)


def _executor(dtype, P, x, dx_out):
    """One vs_vit_layer_fwd + vs_vit_layer_bwd at hidden 64 / 2 heads; returns the tensors by name."""
    from vspike import _lib as L
    from vspike import ops
    M = _B * _N
    lp = dtype != torch.float32
    t = {k: (v.to(dtype) if k.startswith("w_") else v.clone()).to(DEV).contiguous() for k, v in P.items()}
    f32 = torch.float32
    for k, shape, d in (("h1", (M, _D), dtype), ("mean1", (M,), f32), ("rstd1", (M,), f32), ("qkv", (M, 3 * _D), dtype),
                        ("attn_o", (M, _D), dtype), ("lse", (_B, _H, _N), f32), ("y", (M, _D), f32), ("h2", (M, _D), dtype),
                        ("mean2", (M,), f32), ("rstd2", (M,), f32), ("a_pre", (M, _F), dtype), ("a_act", (M, _F), dtype),
                        ("x_out", (M, _D), f32), ("dx_in", (M, _D), f32), ("d_a", (M, _F), dtype), ("d_h", (M, _D), f32),
                        ("dy", (M, _D), f32), ("d_o", (M, _D), dtype), ("d_qkv", (M, 3 * _D), dtype),
                        ("dx_in_lp", (M, _D), dtype), ("dy_lp", (M, _D), dtype)):
        t[k] = torch.full(shape, float("nan"), dtype=d, device=DEV)
    t["x_in"] = x.to(DEV).contiguous()
    t["dx_out"] = dx_out.to(DEV).contiguous()
    t["dx_out_lp"] = t["dx_out"].to(dtype)
    t["attn_ws"] = torch.full((ops.attn32_bwd_workspace_bytes(_B, _N, _H) // 4 + 64,), float("nan"), device=DEV)
    t["ln_ws"] = torch.zeros(ops.layernorm_bwd_workspace_bytes(M, _D) // 4 + 64, device=DEV)
    gws = max(ops.splitk_workspace_bytes(dtype, m, n, M) for m, n in ((_D, _F), (_F, _D), (_D, _D), (3 * _D, _D)))
    t["gemm_ws"] = torch.zeros(gws // 4 + 64, device=DEV)
    s = L.VitLayer()
    s.dtype, s.heads = L.dtype_code(dtype), _H
    s.batch, s.tokens, s.hidden, s.mlp = _B, _N, _D, _F
    s.ln_eps, s.attn_scale = 1e-12, ops.attn_scale(32)
    for k, _ in _W:
        setattr(s, k, t[k].data_ptr())
    for k in ("x_in", "h1", "mean1", "rstd1", "qkv", "attn_o", "lse", "y", "h2", "mean2", "rstd2", "a_pre", "a_act",
              "x_out"):
        setattr(s, k, t[k].data_ptr())
    ops.vit_layer_fwd(s)
    g = L.VitLayerGrad()
    for k, shape in _W:
        t["g_" + k] = torch.zeros(shape, device=DEV)
        setattr(g, k, t["g_" + k].data_ptr())
    for k in ("dx_out", "dx_in", "d_a", "d_h", "dy", "d_o", "d_qkv", "attn_ws", "ln_ws", "gemm_ws"):
        setattr(g, k, t[k].data_ptr())
    if lp:
        g.dx_out_lp, g.dx_in_lp, g.dy_lp = t["dx_out_lp"].data_ptr(), t["dx_in_lp"].data_ptr(), t["dy_lp"].data_ptr()
    g.gemm_ws_bytes, g.flags, g.chain = t["gemm_ws"].numel() * 4, 0, None
    ops.vit_layer_bwd(s, g)
    torch.cuda.synchronize()
    return t


def test_vit_layer_hidden64_two_heads_f32_matches_cpu_block():
    """The project's fp32 bars (tests/test_gpu_contrast.py): outputs 1e-4 of max|ref|, gradients 1e-3 norm-relative."""
    P = _block_params()
    x = _rand(_B * _N, _D, seed=80)
    dx_out = _rand(_B * _N, _D, seed=81)
    t = _executor(torch.float32, P, x, dx_out)
    P64 = {k: v.double().requires_grad_() for k, v in P.items()}
    x64 = x.double().view(_B, _N, _D).requires_grad_()
    out = _cpu_block(x64, P64)
    grads = torch.autograd.grad(out, [x64] + [P64[k] for k, _ in _W], dx_out.double().view(_B, _N, _D))
    assert rel(t["x_out"].view(_B, _N, _D), out.detach()) < 1e-4
    nrel = lambda a, b: ((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-30)).item()  # noqa: E731
    assert nrel(t["dx_in"].view(_B, _N, _D), grads[0]) < 1e-3
    for (k, _), gr in zip(_W, grads[1:]):
        got = t["g_" + k].cpu().double()
        if k == "b_qkv":       # the key third is fixed at zero: its slot stays exactly 0
            assert bool((got[_D:2 * _D] == 0).all())
            got, gr = torch.cat([got[:_D], got[2 * _D:]]), torch.cat([gr[:_D], gr[2 * _D:]])
        assert nrel(got, gr) < 1e-3, (k, nrel(got, gr))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_vit_layer_hidden64_two_heads_runs_the_attn32_kernels(dtype):
    """The executor's attention output and gradient are bit for bit what vs_attn32_fwd / vs_attn32_bwd give on the
    executor's own qkv, O, dO and lse buffers."""
    from vspike import ops
    P = _block_params()
    t = _executor(dtype, P, _rand(_B * _N, _D, seed=82), _rand(_B * _N, _D, seed=83))
    M = _B * _N
    o = torch.empty(M, _D, dtype=dtype, device=DEV)
    lse = torch.empty(_B, _H, _N, device=DEV)
    ops.attn32_fwd(t["qkv"], o, lse, _B, _N, _H)
    dqkv = torch.empty(M, 3 * _D, dtype=dtype, device=DEV)
    ws = torch.empty(ops.attn32_bwd_workspace_bytes(_B, _N, _H) // 4 + 64, device=DEV)
    ops.attn32_bwd(t["qkv"], t["attn_o"], t["d_o"], t["lse"], dqkv, ws, _B, _N, _H)
    torch.cuda.synchronize()
    assert torch.isfinite(t["x_out"]).all() and torch.isfinite(t["dx_in"]).all()
    assert torch.equal(o, t["attn_o"]) and torch.equal(lse, t["lse"]) and torch.equal(dqkv, t["d_qkv"])
