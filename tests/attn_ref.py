"""Float64 reference of the head-dim-64 attention (vs_attn_fwd / vs_attn_bwd) and a rounding model of its bf16
kernels (csrc/attn_fwd.hip, attn_bwd.hip, attn_common.h).  Pure torch on the CPU; shared by
tests/test_cpu_attn_contract.py (which checks this module) and tests/test_gpu_attn_contract.py (which holds the
kernels to it).

Layout (include/vspike.h): qkv [B*N, 3*H*64], Q of head h at column 64h, K at 64(H+h), V at 64(2H+h); o and dout
[B*N, H*64]; lse [B, H, N], natural log; dqkv as qkv.

Reference: `reference()` -- softmax(Q K^T scale) V, its log-sum-exp and the closed-form gradient, all float64.

Rounding model: `model_fwd()` / `model_bwd()` compute the same quantities in float64 except at the places where the
bf16 kernels round to bf16, each of which can be switched off (`Rounding`).  The statements restated, by function
(forward kernels in attn_fwd.hip, backward passes in attn_bwd.hip):

  prescale  Q (forward, dQ pass) or K (dK/dV pass) times c = scale * log2(e), the product in f32, rounded to bf16
            once; the scores are then in log2 units and P = exp2(S).  One statement for every kernel:
              attn_common.h scaled_frag  `v[j] = (float)x[j] * c; return __builtin_convertvector(v, bf16x8)`,
              called for qf[s] (attn_fwd_bf16_kernel), qf[qt][dc] (attn_fwd16_bf16_kernel), w.kf[s] (dkdv_prologue)
              and w.qf[s] (dq_prologue).
            c itself is the f32 product `scale * kLog2e` (vs_attn_fwd's launch; `c2` in the backward prologues).
  p         P rounded to bf16 as the MFMA operand of O += P V and dV += P^T dO:
              forward `pa = pack8f(p); pb = pack8f(p + 8)` (softmax_m), fwd16 `p[qt] = __builtin_convertvector`
              (softmax); dK/dV `pb = pack8f(p)` (attn_bwd_dkdv<false>'s slice), `mma_p`'s `pack8f(pv + 8 * s2)` on P
              (attn_bwd_dkdv<true>).
            The forward's FAST pass also takes the row sum l from the ROUNDED P (`lacc = mfma(sel, pa, lacc)`;
            fwd16 `mfma16(ones, p[qt], lacc[qt])`), its SAFE pass (the redo) from the unrounded one in f32
            (`l_half += ...`) with P = exp2(S - m), m the maximum of the row's first 32-key block
            (`m_new = move ? mxp : m_run` with first_blk; raised later only past 2^32).  `safe` selects it.
            dS = P * (dP - delta) uses the UNROUNDED f32 P (`ds[r] = p[r] * dpa[...]` in the 3-wave slice,
            `pa[r] *= xa[r]` in the pair slice; dQ: `exp2f(sacc) * dpacc` in ds_mma).
  ds        dS rounded to bf16 as the operand of dK += dS^T Q and dQ += dS K:
              `db = pack8f(ds)` (the 3-wave dK/dV slice, ds_mma), `mma_p(fa, pa, w.dkacc)` (the pair slice).
  out       O, dQ, dK, dV rounded to bf16 at the store, after 1/l (O) or `* scale` (dQ, dK) in f32:
              `pack4` in fwd_o_put4 on `oacc * inv`, `pack4(dkacc * scale ...)` / `pack4(dvacc ...)` (dkdv_epilogue),
              `pack4(dqacc * scale ...)` (dq_epilogue).
  delta = rowsum(dO * O) takes O as it is given (the bf16 O of the forward, attn_rowprep_kernel), and lse is
  the f32 the forward stored; both are inputs of `model_bwd`.  Everything else -- the f32 MFMA accumulation, exp2,
  log2, 1/l -- is float64 here.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

DH = 64
LOG2E_F32 = torch.tensor(1.4426950408889634, dtype=torch.float32)     # kLog2e
LN2 = math.log(2.0)
LADDER = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 191, 192, 193, 255, 256, 257, 320, 383, 384, 385)
SCALES = (0.0625, 0.125, 0.2, 1.0)
# the bars tests/test_gpu_ops.py holds the kernels to: max-abs error over max|ref|
BARS = {torch.float32: dict(o=1e-5, lse=1e-5, g=2e-5), torch.bfloat16: dict(o=1.5e-2, lse=3e-3, g=3e-2)}


@dataclass(frozen=True)
class Rounding:
    prescale: bool = True
    p: bool = True
    ds: bool = True
    out: bool = True


ON = Rounding()
OFF = Rounding(False, False, False, False)


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """Round float64 values to 8 significant bits, nearest-even, with no exponent limit (the model must not
    overflow where the kernel's safe pass does not)."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


def split_heads(x: torch.Tensor, B: int, N: int, H: int, parts: int = 3):
    """[B*N, parts*H*64] -> `parts` tensors [B, H, N, 64]."""
    return x.reshape(B, N, parts, H, DH).permute(2, 0, 3, 1, 4)


def merge_heads(x: torch.Tensor) -> torch.Tensor:
    """[B, H, N, 64] -> [B*N, H*64]."""
    B, H, N, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * N, H * DH)


def merge_qkv(q, k, v) -> torch.Tensor:
    return torch.cat([merge_heads(q), merge_heads(k), merge_heads(v)], dim=1)


def make_inputs(B: int, N: int, H: int, seed: int, dtype=torch.bfloat16, scale: float = 0.125):
    """The fixture inputs of both test files: qkv ~ 1.5 * randn and dout ~ randn (the magnitudes tests/test_gpu_ops.py
    uses), rounded to `dtype`.  For scale > 0.125, Q and K shrink by sqrt(0.125 / scale) each so that the logits
    keep the magnitude they have at the trained scale."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * N, 3 * H * DH, generator=g) * 1.5
    dout = torch.randn(B * N, H * DH, generator=g)
    if scale > 0.125:
        qkv[:, :2 * H * DH] *= math.sqrt(0.125 / scale)
    return qkv.to(dtype), dout.to(dtype)


def make_extreme_inputs(B: int, N: int, H: int, seed: int, dtype=torch.bfloat16):
    """Inputs that send the bf16 forward's fast pass out of its band (the construction of tests/test_gpu_ops.py's
    test_attention_extreme_logits_move_reference, in every (batch, head)): every key close to 0.75 * ones, query 3
    with all its scores near -96 (-138 in log2 units: a row sum below the band's 2^-100), query 40 near +82 (above
    2^96) and query 70 dominated by one late key.  The amplitudes are the smallest round ones that leave the band
    by a clear margin at N of a few hundred: the pre-scaling's bf16 rounding moves a logit by 2^-9 of its size,
    and at the original's +-300 the gradients of these three rows would be dominated by that in any bf16 kernel.
    The two constant queries are spread by 25 % per dimension for the same reason: on a constant row the 64 rounding
    errors of c * q are one and the same, the forward's lse moves by it, and the dK/dV pass (which rounds c * k
    instead) then sees P = exp(S - lse) off by as much."""
    assert N > 100
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * N, 3 * H * DH, generator=g) * 0.3
    dout = torch.randn(B * N, H * DH, generator=g)
    q, k, _ = split_heads(qkv, B, N, H)             # views into qkv
    k += 6.0 / 8.0
    spread = 1.0 + 0.25 * torch.randn(2, B, H, DH, generator=g)
    q[:, :, 3] = -128.0 / 8.0 * spread[0]
    q[:, :, 40] = 110.0 / 8.0 * spread[1]
    q[:, :, 70] = k[:, :, N - 21] * 16.0
    return qkv.to(dtype), dout.to(dtype)


def reference(qkv, dout, B, N, H, scale):
    """float64 attention: (o [B*N, H*64], lse [B, H, N], dqkv [B*N, 3*H*64])."""
    q, k, v = split_heads(qkv.double(), B, N, H)
    do = split_heads(dout.double(), B, N, H, 1)[0]
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    dv = p.transpose(-1, -2) @ do
    ds = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
    dq = ds @ k * scale
    dk = ds.transpose(-1, -2) @ q * scale
    return merge_heads(o), lse, merge_qkv(dq, dk, dv)


def _prescale(x, scale, on):
    """x * (scale * log2 e): as the kernels do it (f32 factor, f32 product, one bf16 rounding), or exactly."""
    if not on:
        return x * (scale * math.log2(math.e))
    c = torch.tensor(scale, dtype=torch.float32) * LOG2E_F32
    return (x.float() * c).to(torch.bfloat16).double()


def model_fwd(qkv, B, N, H, scale, rnd: Rounding = ON, safe: bool = False):
    """The bf16 forward's roundings on float64 arithmetic: (o, lse).  safe: the redo pass's softmax."""
    q, k, v = split_heads(qkv.double(), B, N, H)
    s2 = _prescale(q, scale, rnd.prescale) @ k.transpose(-1, -2)          # log2 units
    m = s2[..., :32].max(dim=-1, keepdim=True).values if safe else torch.zeros_like(s2[..., :1])
    p = torch.exp2(s2 - m)
    pr = bf16_round(p) if rnd.p else p
    l = (p if safe else pr).sum(-1, keepdim=True)
    o = (pr @ v) / l
    lse = (m + torch.log2(l)).squeeze(-1) * LN2
    o = merge_heads(o)
    return (bf16_round(o) if rnd.out else o), lse


def model_bwd(qkv, o, lse, dout, B, N, H, scale, rnd: Rounding = ON):
    """The bf16 backward's roundings on float64 arithmetic, from the O and lse it is given: dqkv."""
    q, k, v = split_heads(qkv.double(), B, N, H)
    do = split_heads(dout.double(), B, N, H, 1)[0]
    od = split_heads(o.double(), B, N, H, 1)[0]
    nlse2 = -lse.double()[..., None] * math.log2(math.e)
    dp = do @ v.transpose(-1, -2) - (do * od).sum(-1, keepdim=True)
    rd = bf16_round if rnd.ds else (lambda x: x)
    # dK / dV pass: K pre-scaled
    p = torch.exp2(q @ _prescale(k, scale, rnd.prescale).transpose(-1, -2) + nlse2)
    dv = (bf16_round(p) if rnd.p else p).transpose(-1, -2) @ do
    dk = rd(p * dp).transpose(-1, -2) @ q * scale
    # dQ pass: Q pre-scaled
    p = torch.exp2(_prescale(q, scale, rnd.prescale) @ k.transpose(-1, -2) + nlse2)
    dq = rd(p * dp) @ k * scale
    g = merge_qkv(dq, dk, dv)
    return bf16_round(g) if rnd.out else g


def rel(a, b) -> float:
    """max-abs error over max|ref| of the whole tensor (the bars of tests/test_gpu_ops.py)."""
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def head_err(x, ref, B, N, H, parts=1):
    """Per (part, batch, head): the worst row's max-abs error and the head's max|ref|, as two [parts, B, H] float64
    tensors.  x, ref: [B*N, parts*H*64], or lse [B, H, N] (every entry its own row)."""
    x, ref = x.double().cpu(), ref.double().cpu()
    if x.dim() == 3:
        return (x - ref).abs().amax(-1)[None], ref.abs().amax(-1)[None]
    xs, rs = split_heads(x, B, N, H, parts), split_heads(ref, B, N, H, parts)
    return (xs - rs).abs().amax(dim=(-1, -2)), rs.abs().amax(dim=(-1, -2))


def cancel_floor(qkv, dout, B, N, H, scale):
    """[3, B, H]: what f32 accumulation may leave of a dQ / dK head whose reference is exactly zero.  That is the case
    at N = 1 only (P = 1 and dP = delta, so dS = 0 in exact arithmetic) and the tests apply this nowhere else.  dP
    and delta are two differently ordered f32 sums of the same 64 products dO[d] * V[d], each carrying at most
    64 * 2^-24 * max|dO| * max|V| of rounding; dS = P (dP - delta) with P = 1, times |K| (dQ) or |Q| (dK) and scale.
    Zero for dV, which has no such cancellation."""
    assert N == 1
    q, k, v = (t.abs().amax(dim=(-1, -2)) for t in split_heads(qkv.double().cpu(), B, N, H))
    do = split_heads(dout.double().cpu(), B, N, H, 1)[0].abs().amax(dim=(-1, -2))
    e = 2.0 * 64 * 2.0 ** -24 * do * v * scale
    return torch.stack([e * k, e * q, torch.zeros_like(e)])
