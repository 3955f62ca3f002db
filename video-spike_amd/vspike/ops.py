"""Tensor-level wrappers over the libvspike C-ABI (one function per entry point).

Each wrapper validates devices, passes raw pointers + sizes and enqueues on the current stream.
Outputs are caller-allocated tensors (the PyTorch caching allocator owns all memory).
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

import torch

from . import _lib as L
from ._lib import check, lib, ptr, require_device, stream


def gemm(a, b, c, *, M, N, K, a_kcontig, b_kcontig, lda, ldb, ldc, epilogue=0, alpha=1.0, bias=None,
         residual=None, ld_residual=0, pos=None, pos_rows=0, aux_in=None, ld_aux_in=0, aux_out=None,
         ld_aux_out=0, split_k=0, a_rowsum=None, workspace=None):
    """C[M,N] = epilogue(alpha * A @ B); layouts as in include/vspike.h (vs_gemm).
    workspace: optional device tensor for split-K partials of an ATOMIC GEMM (see vs_gemm_desc)."""
    require_device(a, b, c)
    d = L.GemmDesc()
    d.dtype = L.dtype_code(a.dtype)
    if L.dtype_code(b.dtype) != d.dtype:
        raise L.VsError("gemm: A and B must share a dtype")
    d.out_dtype = L.dtype_code(c.dtype)
    d.a_kcontig, d.b_kcontig = int(a_kcontig), int(b_kcontig)
    d.M, d.N, d.K = M, N, K
    d.a, d.lda, d.b, d.ldb, d.c, d.ldc = a.data_ptr(), lda, b.data_ptr(), ldb, c.data_ptr(), ldc
    d.epilogue, d.alpha = epilogue, alpha
    d.bias = ptr(bias)
    d.residual, d.ld_residual = ptr(residual), ld_residual
    d.pos, d.pos_rows = ptr(pos), pos_rows
    d.aux_in, d.ld_aux_in = ptr(aux_in), ld_aux_in
    d.aux_out, d.ld_aux_out = ptr(aux_out), ld_aux_out
    d.split_k = split_k
    d.a_rowsum = ptr(a_rowsum)
    if workspace is not None:
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    check(lib().vs_gemm(ctypes.byref(d), stream()), "vs_gemm")
    return c


def linear(x, w, out, *, bias=None, epilogue=0, **kw):
    """out[M,N] = x[M,K] @ w[N,K]^T (+ epilogue): the nn.Linear forward."""
    M, K = x.shape
    N = w.shape[0]
    if bias is not None:
        epilogue |= L.EPI_BIAS
    return gemm(x, w, out, M=M, N=N, K=K, a_kcontig=True, b_kcontig=True, lda=x.stride(0), ldb=w.stride(0),
                ldc=out.stride(0), epilogue=epilogue, bias=bias, **kw)


def quant_mxfp8(x, q, scales):
    """MX-FP8 quantisation (vs_quant_mxfp8): x [M, K] f32/bf16 -> q [M, K] uint8 (OCP e4m3 codes) and
    scales [M, K // 32] uint8 (E8M0 exponents, 2^(e - 127) per 32 consecutive elements of a row)."""
    require_device(x, q, scales)
    M, K = x.shape
    check(lib().vs_quant_mxfp8(L.dtype_code(x.dtype), M, K, x.data_ptr(), x.stride(0), q.data_ptr(), q.stride(0),
                               scales.data_ptr(), scales.stride(0), stream()), "vs_quant_mxfp8")
    return q, scales


def gemm_mxfp8(a_q, a_s, b_q, b_s, c, *, epilogue=0, bias=None, residual=None, aux_out=None, alpha=1.0):
    """c = epilogue(A B^T) on the block-scaled fp8 MFMA (vs_gemm_mxfp8): a_q [M, K], b_q [N, K] uint8
    e4m3 codes with their E8M0 scales (quant_mxfp8 layout); c [M, N] f32 or bf16."""
    require_device(a_q, b_q, c)
    M, K = a_q.shape
    N = b_q.shape[0]
    d = L.GemmDesc()
    d.dtype, d.out_dtype = L.VS_FP8, L.dtype_code(c.dtype)
    d.a_kcontig = d.b_kcontig = 1
    d.M, d.N, d.K = M, N, K
    d.a, d.lda, d.b, d.ldb, d.c, d.ldc = a_q.data_ptr(), a_q.stride(0), b_q.data_ptr(), b_q.stride(0), c.data_ptr(), c.stride(0)
    d.epilogue, d.alpha = epilogue, alpha
    d.bias = ptr(bias)
    d.residual, d.ld_residual = ptr(residual), (residual.stride(0) if residual is not None else 0)
    d.aux_out, d.ld_aux_out = ptr(aux_out), (aux_out.stride(0) if aux_out is not None else 0)
    check(lib().vs_gemm_mxfp8(ctypes.byref(d), a_s.data_ptr(), a_s.stride(0), b_s.data_ptr(), b_s.stride(0), stream()),
          "vs_gemm_mxfp8")
    return c


def mlp_fused_ok(M: int, D: int, F: int) -> bool:
    """vs_mlp_fused_ok: the fused MLP kernels take this shape (bf16, D = 192, F % 64 == 0)."""
    return bool(lib().vs_mlp_fused_ok(int(M), int(D), int(F)))


def mlp_fwd(h2, w1, b1, w2, b2, y, out):
    """out = y + gelu(h2 @ w1^T + b1) @ w2^T + b2 in one launch (vs_mlp_fwd): h2 [M, D] bf16, w1 [F, D],
    w2 [D, F] bf16, y / out [M, D] f32 (modeling_videomae.py:370-399)."""
    require_device(h2, w1, w2, y, out)
    M, D = h2.shape
    F = w1.shape[0]
    check(lib().vs_mlp_fwd(M, D, F, h2.data_ptr(), h2.stride(0), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                           b2.data_ptr(), y.data_ptr(), y.stride(0), out.data_ptr(), out.stride(0), stream()),
          "vs_mlp_fwd")
    return out


def mlp_bwd_da(h2, w1, b1, w2, dy, da, a):
    """da = (dy @ w2) * gelu'(h2 @ w1^T + b1) and a = gelu(h2 @ w1^T + b1), the pre-activation
    recomputed (vs_mlp_bwd_da): dy [M, D] bf16, da / a [M, F] bf16."""
    require_device(h2, w1, w2, dy, da, a)
    M, D = h2.shape
    F = w1.shape[0]
    check(lib().vs_mlp_bwd_da(M, D, F, h2.data_ptr(), h2.stride(0), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                              dy.data_ptr(), dy.stride(0), da.data_ptr(), da.stride(0), a.data_ptr(), a.stride(0),
                              stream()), "vs_mlp_bwd_da")
    return da, a


def linear_dx(dy, w, out, *, epilogue=0, accumulate=False, **kw):
    """out[M,K] = dy[M,N] @ w[N,K]; accumulate=True adds into an f32 `out` with split-K atomics
    (for skinny products whose reduction N is long, e.g. the head's dZ over 100*neurons)."""
    M, N = dy.shape
    K = w.shape[1]
    if accumulate:
        epilogue |= L.EPI_ATOMIC
    return gemm(dy, w, out, M=M, N=K, K=N, a_kcontig=True, b_kcontig=False, lda=dy.stride(0), ldb=w.stride(0),
                ldc=out.stride(0), epilogue=epilogue, **kw)


def splitk_workspace_bytes(dtype, M, N, K):
    return int(lib().vs_gemm_splitk_workspace_bytes(L.dtype_code(dtype), M, N, K))


def linear_dw(dy, x, dw, *, accumulate=True, db=None, workspace=None):
    """dw[N,K] (+)= dy[M,N]^T @ x[M,K]  (f32 dw, split-K over the M reduction).
    db (optional, f32 [N]) += column sums of dy, fused into the same pass.  The splits are summed
    through `workspace` (allocated here when None; False = f32 atomics instead)."""
    M, N = dy.shape
    K = x.shape[1]
    epi = L.EPI_ATOMIC if accumulate else 0
    if accumulate and workspace is None:
        nb = splitk_workspace_bytes(dy.dtype, N, K, M)
        workspace = torch.empty(nb // 4 + 4, dtype=torch.float32, device=dy.device) if nb else None
    ws = None if workspace is False else workspace
    return gemm(dy, x, dw, M=N, N=K, K=M, a_kcontig=False, b_kcontig=False, lda=dy.stride(0), ldb=x.stride(0),
                ldc=dw.stride(0), epilogue=epi, split_k=0 if accumulate else 1, a_rowsum=db, workspace=ws)


def layernorm_fwd(x, gamma, beta, eps, y, mean, rstd):
    require_device(x, y)
    rows, cols = x.shape
    check(lib().vs_layernorm_fwd(L.dtype_code(y.dtype), rows, cols, x.data_ptr(), x.stride(0), gamma.data_ptr(),
                                 beta.data_ptr(), eps, y.data_ptr(), y.stride(0), mean.data_ptr(), rstd.data_ptr(),
                                 stream()), "vs_layernorm_fwd")
    return y


def layernorm_bwd_workspace_bytes(rows, cols):
    return int(lib().vs_layernorm_bwd_workspace_bytes(rows, cols))


def layernorm_bwd(dy, x, mean, rstd, gamma, dx, dgamma, dbeta, dres=None, dx_lp=None, workspace=None):
    """LayerNorm backward (dy f32 or bf16); dgamma/dbeta accumulate.  `workspace` (f32, >= layernorm_bwd_workspace_bytes)
    is allocated here when not given; pass False to use the per-block atomic reduction instead."""
    require_device(dy, x, dx)
    rows, cols = x.shape
    if workspace is None:
        workspace = torch.empty(layernorm_bwd_workspace_bytes(rows, cols) // 4 + 4, dtype=torch.float32,
                                device=x.device)
    ws = None if workspace is False else workspace
    check(lib().vs_layernorm_bwd_dt(L.dtype_code(dy.dtype), rows, cols, dy.data_ptr(), dy.stride(0), x.data_ptr(),
                                    x.stride(0), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), ptr(dres),
                                    dres.stride(0) if dres is not None else 0, dx.data_ptr(), dx.stride(0), ptr(dx_lp),
                                    dgamma.data_ptr(), dbeta.data_ptr(), ptr(ws), stream()), "vs_layernorm_bwd")
    return dx


def linear_dx_ln_bwd(dy, w, x, mean, rstd, gamma, dx, dgamma, dbeta, *, dres=None, dx_lp=None, scratch=None,
                     workspace=None):
    """dx = dres + LN'(dy @ w; x, mean, rstd, gamma), dgamma/dbeta accumulate (vs_gemm_ln_bwd): the
    dX product of a Linear fused with the backward of the LayerNorm that feeds it.  dy [M, Nout]
    (bf16 or f32), w [Nout, D]; `scratch` ([M, D] f32) is only written off the fused path."""
    require_device(dy, w, x, dx)
    M, Nout = dy.shape
    D = w.shape[1]
    if scratch is None:
        scratch = torch.empty(M, D, dtype=torch.float32, device=x.device)
    if workspace is None:
        workspace = torch.empty(layernorm_bwd_workspace_bytes(M, D) // 4 + 4, dtype=torch.float32, device=x.device)
    d = L.GemmDesc()
    d.dtype = L.dtype_code(dy.dtype)
    d.out_dtype = L.dtype_code(torch.float32)
    d.a_kcontig, d.b_kcontig = 1, 0
    d.M, d.N, d.K = M, D, Nout
    d.a, d.lda, d.b, d.ldb, d.c, d.ldc = dy.data_ptr(), dy.stride(0), w.data_ptr(), w.stride(0), scratch.data_ptr(), D
    d.alpha = 1.0
    check(lib().vs_gemm_ln_bwd(ctypes.byref(d), x.data_ptr(), x.stride(0), mean.data_ptr(), rstd.data_ptr(),
                               gamma.data_ptr(), ptr(dres), dres.stride(0) if dres is not None else 0, dx.data_ptr(),
                               dx.stride(0), ptr(dx_lp), dgamma.data_ptr(), dbeta.data_ptr(), workspace.data_ptr(),
                               stream()), "vs_gemm_ln_bwd")
    return dx


def linear_ln_fwd(x, w, y, residual, gamma, beta, eps, h, mean, rstd, *, bias=None):
    """y = x @ w^T (+ bias) + residual (f32) and h = LayerNorm(y) (bf16) with its row mean / rstd
    (vs_gemm_ln_fwd): the ViT block's attention-output product fused with layernorm_after."""
    require_device(x, w, y, residual, h)
    M, K = x.shape
    N = w.shape[0]
    d = L.GemmDesc()
    d.dtype = L.dtype_code(x.dtype)
    d.out_dtype = L.dtype_code(torch.float32)
    d.a_kcontig, d.b_kcontig = 1, 1
    d.M, d.N, d.K = M, N, K
    d.a, d.lda, d.b, d.ldb, d.c, d.ldc = x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), y.data_ptr(), y.stride(0)
    d.alpha = 1.0
    d.epilogue = L.EPI_RESIDUAL | (L.EPI_BIAS if bias is not None else 0)
    d.bias = ptr(bias)
    d.residual, d.ld_residual = residual.data_ptr(), residual.stride(0)
    check(lib().vs_gemm_ln_fwd(ctypes.byref(d), gamma.data_ptr(), beta.data_ptr(), float(eps), h.data_ptr(),
                               h.stride(0), mean.data_ptr(), rstd.data_ptr(), stream()), "vs_gemm_ln_fwd")
    return h


def attn_fwd(qkv, o, lse, B, N, H, scale=0.125):
    require_device(qkv, o, lse)
    check(lib().vs_attn_fwd(L.dtype_code(qkv.dtype), B, N, H, 64, qkv.data_ptr(), qkv.stride(0), o.data_ptr(),
                            o.stride(0), lse.data_ptr(), scale, stream()), "vs_attn_fwd")
    return o


def attn_bwd_workspace_bytes(B, N, H):
    return int(lib().vs_attn_bwd_workspace_bytes(B, N, H, 64))


def attn_bwd(qkv, o, dout, lse, dqkv, workspace, B, N, H, scale=0.125):
    require_device(qkv, o, dout, lse, dqkv, workspace)
    check(lib().vs_attn_bwd(L.dtype_code(qkv.dtype), B, N, H, 64, qkv.data_ptr(), qkv.stride(0), o.data_ptr(),
                            o.stride(0), dout.data_ptr(), dout.stride(0), lse.data_ptr(), dqkv.data_ptr(),
                            dqkv.stride(0), workspace.data_ptr(), scale, stream()), "vs_attn_bwd")
    return dqkv


def attn32_fwd(qkv, o, lse, B, N, H, scale=None):
    """Head-dim-32 attention for 1 <= N <= 256 (vs_attn32_fwd): qkv [B*N, >= 3*H*32], o [B*N, >= H*32], lse
    [B, H, N] f32.  scale defaults to 1 / sqrt(32)."""
    require_device(qkv, o, lse)
    scale = attn_scale(32) if scale is None else scale
    check(lib().vs_attn32_fwd(L.dtype_code(qkv.dtype), B, N, H, qkv.data_ptr(), qkv.stride(0), o.data_ptr(),
                              o.stride(0), lse.data_ptr(), scale, stream()), "vs_attn32_fwd")
    return o


def attn32_bwd_workspace_bytes(B, N, H):
    return int(lib().vs_attn32_bwd_workspace_bytes(B, N, H))


def attn32_bwd(qkv, o, dout, lse, dqkv, workspace, B, N, H, scale=None):
    require_device(qkv, o, dout, lse, dqkv, workspace)
    scale = attn_scale(32) if scale is None else scale
    check(lib().vs_attn32_bwd(L.dtype_code(qkv.dtype), B, N, H, qkv.data_ptr(), qkv.stride(0), o.data_ptr(),
                              o.stride(0), dout.data_ptr(), dout.stride(0), lse.data_ptr(), dqkv.data_ptr(),
                              dqkv.stride(0), workspace.data_ptr(), scale, stream()), "vs_attn32_bwd")
    return dqkv


def patch_im2col(pixels, cols, tubelet, patch):
    require_device(pixels, cols)
    B, F, C, H, W = pixels.shape
    check(lib().vs_patch_im2col(L.dtype_code(cols.dtype), B, F, C, H, W, tubelet, patch, pixels.data_ptr(),
                                cols.data_ptr(), stream()), "vs_patch_im2col")
    return cols


def patch_embed_fwd(pixels, weight, bias, pos, out, tubelet, patch, cols=None):
    """out[B*n_tok, D] f32 = Conv3d patch embedding of pixels (B, F, C, H, W) f32 + bias + pos, with the
    tubelet gather inside the GEMM (vs_patch_embed_fwd); cols (optional bf16 [B*n_tok, C*t*p*p])
    receives the gathered rows for the weight gradient."""
    require_device(pixels, weight, bias, pos, out)
    B, F, C, H, W = pixels.shape
    check(lib().vs_patch_embed_fwd(B, F, C, H, W, tubelet, patch, pixels.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                                   pos.data_ptr(), out.shape[1], out.data_ptr(), ptr(cols), stream()),
          "vs_patch_embed_fwd")
    return out


def patch_embed_fused_ok(cfg, dtype) -> bool:
    """Shapes the fused patch embedding covers (else im2col + GEMM)."""
    return (dtype == torch.bfloat16 and cfg.tubelet_size == 2 and cfg.patch_size == 16 and
            cfg.hidden_size in (64, 128, 192) and cfg.num_channels <= 8 and L.knob_get("no_patch_fused") == 0)


def patch_embed_dw_workspace_bytes(tokens, D, K):
    return int(lib().vs_patch_embed_dw_workspace_bytes(tokens, D, K))


def patch_dw_ok(cfg, dtype) -> bool:
    """Shapes the gather weight gradient covers (else im2col + the dW product of vs_gemm)."""
    return (dtype == torch.bfloat16 and cfg.tubelet_size == 2 and cfg.patch_size == 16 and cfg.hidden_size % 64 == 0
            and cfg.num_channels <= 8 and cfg.hidden_size <= cfg.num_channels * 512
            and L.knob_get("no_patch_fused") == 0)


def patch_embed_dw(pixels, dx, dweight, dbias, tubelet, patch, workspace=None):
    """dweight[D, C*t*p*p] += dx^T X and dbias[D] += column sums of dx, X the tubelet gather of the f32
    pixels (B, F, C, H, W) read in the operand load (vs_patch_embed_dw); dx bf16 [B*n_tok, D]."""
    require_device(pixels, dx, dweight)
    B, F, C, H, W = pixels.shape
    D = dx.shape[1]
    K = dweight.shape[1]
    if workspace is None:
        workspace = torch.empty(patch_embed_dw_workspace_bytes(dx.shape[0], D, K) // 4 + 4, dtype=torch.float32,
                                device=dx.device)
    check(lib().vs_patch_embed_dw(B, F, C, H, W, tubelet, patch, pixels.data_ptr(), dx.data_ptr(), dx.stride(0), D,
                                  dweight.data_ptr(), dweight.stride(0), ptr(dbias), workspace.data_ptr(),
                                  workspace.numel() * 4, stream()), "vs_patch_embed_dw")
    return dweight


def sinusoid_table(n_pos, dim, device):
    out = torch.empty(n_pos, dim, dtype=torch.float32, device=device)
    check(lib().vs_sinusoid_table(n_pos, dim, out.data_ptr(), stream()), "vs_sinusoid_table")
    return out


def colsum(x, out, rows=None, cols=None):
    """out[c] += sum_r x[r, c] (out f32)."""
    require_device(x, out)
    rows = x.shape[0] if rows is None else rows
    cols = x.shape[1] if cols is None else cols
    check(lib().vs_colsum(L.dtype_code(x.dtype), rows, cols, x.data_ptr(), x.stride(0), out.data_ptr(), stream()),
          "vs_colsum")
    return out


def cast(x, out):
    require_device(x, out)
    check(lib().vs_cast(L.dtype_code(x.dtype), L.dtype_code(out.dtype), x.numel(), x.data_ptr(), out.data_ptr(),
                        stream()), "vs_cast")
    return out


def token_pool_fwd(x, S, out, pos=None, out_lp=None):
    """out[g] = mean of the S consecutive rows g*S .. g*S+S-1 of x [G*S, D] f32 (row stride x.stride(0))
    (+ pos[g % pos.shape[0]]); out_lp (optional bf16 [G, D]) = out rounded (vs_token_pool_fwd)."""
    require_device(x, out, pos, out_lp)
    G, D = out.shape
    if x.shape[0] != G * S or x.shape[1] != D or (pos is not None and pos.shape[1] != D):
        raise L.VsError("token_pool_fwd: x must be [G*S, D], out [G, D], pos [rows, D]")
    check(lib().vs_token_pool_fwd(G, S, D, x.data_ptr(), x.stride(0), ptr(pos), pos.shape[0] if pos is not None else 0,
                                  out.data_ptr(), ptr(out_lp), stream()), "vs_token_pool_fwd")
    return out


def token_pool_bwd(dpool, S, dx, dx_lp=None):
    """dx[g*S + s] = dpool[g] / S for every s (dx [G*S, D] f32, dense); dx_lp (optional bf16) = dx
    rounded (vs_token_pool_bwd)."""
    require_device(dpool, dx, dx_lp)
    G, D = dpool.shape
    if dx.numel() != G * S * D or (dx_lp is not None and dx_lp.numel() != G * S * D):
        raise L.VsError("token_pool_bwd: dx (and dx_lp) must hold G*S rows of D")
    check(lib().vs_token_pool_bwd(G, S, D, dpool.data_ptr(), dx.data_ptr(), ptr(dx_lp), stream()),
          "vs_token_pool_bwd")
    return dx


def cls_embed_fwd(patches, cls, table, x):
    """x [G, P+1, D] f32: row 0 = cls + table[0], rows 1..P = the patch rows patches [G*P, D] (vs_cls_embed_fwd)."""
    require_device(patches, cls, table, x)
    G, T, D = x.shape
    if patches.shape != (G * (T - 1), D) or table.shape != (T, D) or cls.numel() != D:
        raise L.VsError("cls_embed_fwd: patches [G*P, D], cls [D], table [P+1, D], x [G, P+1, D]")
    check(lib().vs_cls_embed_fwd(G, T - 1, D, patches.data_ptr(), cls.data_ptr(), table.data_ptr(), x.data_ptr(),
                                 stream()), "vs_cls_embed_fwd")
    return x


def cls_embed_bwd(dx, d_cls, d_patches):
    """d_cls [D] = sum over images (ascending) of dx[:, 0]; d_patches [G*P, D] (f32 or bf16) = dx[:, 1:]
    (vs_cls_embed_bwd).  dx [G, P+1, D] f32, dense."""
    require_device(dx, d_cls, d_patches)
    G, T, D = dx.shape
    if d_patches.shape != (G * (T - 1), D) or d_cls.numel() != D or not dx.is_contiguous():
        raise L.VsError("cls_embed_bwd: dx [G, P+1, D] dense, d_cls [D], d_patches [G*P, D]")
    check(lib().vs_cls_embed_bwd(L.dtype_code(d_patches.dtype), G, T - 1, D, dx.data_ptr(), d_cls.data_ptr(),
                                 d_patches.data_ptr(), stream()), "vs_cls_embed_bwd")
    return d_patches


def _mae_ids(ids, shape, what):
    if ids.dtype != torch.int32 or tuple(ids.shape) != tuple(shape) or not ids.is_contiguous():
        raise L.VsError(f"{what}: the index tensor must be a dense int32 {tuple(shape)}")


def _mae_dense(what, *tensors):
    for t in tensors:
        if not t.is_contiguous():
            raise L.VsError(f"{what}: tensors must be dense")


def mae_embed_fwd(patches, ids_keep, cls, table, x0):
    """x0 [G, Lk+1, D] f32: row 0 = cls + table[0], row 1 + j = patches[g * P + ids_keep[g, j]] (vs_mae_embed_fwd).
    patches [G*P, D] f32, ids_keep [G, Lk] int32, table [>= 1, D] (row 0 is read)."""
    require_device(patches, ids_keep, cls, table, x0)
    G, T, D = x0.shape
    P = patches.shape[0] // G
    if patches.shape != (G * P, D) or cls.numel() != D or table.shape[-1] != D or x0.dtype != torch.float32:
        raise L.VsError("mae_embed_fwd: patches [G*P, D], cls [D], table [., D], x0 [G, Lk+1, D] f32")
    _mae_ids(ids_keep, (G, T - 1), "mae_embed_fwd")
    _mae_dense("mae_embed_fwd", patches, table, x0)
    check(lib().vs_mae_embed_fwd(G, P, T - 1, D, patches.data_ptr(), ids_keep.data_ptr(), cls.data_ptr(),
                                 table.data_ptr(), x0.data_ptr(), stream()), "vs_mae_embed_fwd")
    return x0


def mae_embed_bwd(dx, ids_restore, d_cls, d_patches):
    """d_patches [G*P, D] (f32 or bf16) = the kept rows of dx [G, Lk+1, D] f32 (zero rows for masked patches), d_cls [D]
    = sum over images (ascending) of dx[:, 0] (vs_mae_embed_bwd).  ids_restore [G, P] int32."""
    require_device(dx, ids_restore, d_cls, d_patches)
    G, T, D = dx.shape
    P = ids_restore.shape[1]
    if d_patches.shape != (G * P, D) or d_cls.numel() != D or dx.dtype != torch.float32:
        raise L.VsError("mae_embed_bwd: dx [G, Lk+1, D] f32, d_cls [D], d_patches [G*P, D]")
    _mae_ids(ids_restore, (G, P), "mae_embed_bwd")
    _mae_dense("mae_embed_bwd", dx, d_patches)
    check(lib().vs_mae_embed_bwd(L.dtype_code(d_patches.dtype), G, P, T - 1, D, dx.data_ptr(), ids_restore.data_ptr(),
                                 d_cls.data_ptr(), d_patches.data_ptr(), stream()), "vs_mae_embed_bwd")
    return d_patches


def mae_dec_assemble_fwd(e, ids_restore, mask_token, tabd, xd):
    """xd [G, P+1, D] f32 from e [G, Lk+1, D] f32: the decoder's sequence (vs_mae_dec_assemble_fwd)."""
    require_device(e, ids_restore, mask_token, tabd, xd)
    G, T, D = xd.shape
    if e.shape[0] != G or e.shape[2] != D or tabd.shape != (T, D) or mask_token.numel() != D or \
            e.dtype != torch.float32 or xd.dtype != torch.float32:
        raise L.VsError("mae_dec_assemble_fwd: e [G, Lk+1, D] f32, mask_token [D], tabd [P+1, D], xd [G, P+1, D] f32")
    _mae_ids(ids_restore, (G, T - 1), "mae_dec_assemble_fwd")
    _mae_dense("mae_dec_assemble_fwd", e, tabd, xd)
    check(lib().vs_mae_dec_assemble_fwd(G, T - 1, e.shape[1] - 1, D, e.data_ptr(), ids_restore.data_ptr(),
                                        mask_token.data_ptr(), tabd.data_ptr(), xd.data_ptr(), stream()),
          "vs_mae_dec_assemble_fwd")
    return xd


def mae_dec_assemble_bwd_workspace_bytes(G, D):
    return int(lib().vs_mae_dec_assemble_bwd_workspace_bytes(G, D))


def mae_dec_assemble_bwd(dxd, ids_keep, ids_restore, d_e, d_mask_token, workspace):
    """d_e [G, Lk+1, D] (f32 or bf16) and d_mask_token [D] f32 (written) from dxd [G, P+1, D] f32
    (vs_mae_dec_assemble_bwd); workspace: f32, mae_dec_assemble_bwd_workspace_bytes(G, D)."""
    require_device(dxd, ids_keep, ids_restore, d_e, d_mask_token, workspace)
    G, T, D = dxd.shape
    Lk = d_e.shape[1] - 1
    if d_e.shape != (G, Lk + 1, D) or d_mask_token.numel() != D or dxd.dtype != torch.float32 or \
            workspace.numel() * workspace.element_size() < mae_dec_assemble_bwd_workspace_bytes(G, D):
        raise L.VsError("mae_dec_assemble_bwd: dxd [G, P+1, D] f32, d_e [G, Lk+1, D], d_mask_token [D], workspace")
    _mae_ids(ids_keep, (G, Lk), "mae_dec_assemble_bwd")
    _mae_ids(ids_restore, (G, T - 1), "mae_dec_assemble_bwd")
    _mae_dense("mae_dec_assemble_bwd", dxd, d_e)
    check(lib().vs_mae_dec_assemble_bwd(L.dtype_code(d_e.dtype), G, T - 1, Lk, D, dxd.data_ptr(), ids_keep.data_ptr(),
                                        ids_restore.data_ptr(), d_e.data_ptr(), d_mask_token.data_ptr(),
                                        workspace.data_ptr(), stream()), "vs_mae_dec_assemble_bwd")
    return d_e


def mae_recon_loss_workspace_bytes(G, P):
    return int(lib().vs_mae_recon_loss_workspace_bytes(G, P))


def mae_recon_loss(pred, pixels, ids_restore, len_keep, patch, loss, d_pred, workspace):
    """HF ViTMAE's forward_loss (norm_pix_loss false) and its gradient (vs_mae_recon_loss): pred [G, P+1, K] f32 (the
    CLS row is ignored), pixels [G, C, S, S] f32, loss [1] f32, d_pred [G, P+1, K] f32 or bf16."""
    require_device(pred, pixels, ids_restore, loss, d_pred, workspace)
    G, C, S, _ = pixels.shape
    P = (S // patch) ** 2
    K = patch * patch * C
    if pred.shape != (G, P + 1, K) or d_pred.shape != (G, P + 1, K) or pred.dtype != torch.float32 or \
            pixels.dtype != torch.float32 or pixels.shape[3] != S or \
            workspace.numel() * workspace.element_size() < mae_recon_loss_workspace_bytes(G, P):
        raise L.VsError("mae_recon_loss: pred / d_pred [G, P+1, patch^2 C], pixels [G, C, S, S] f32, workspace")
    _mae_ids(ids_restore, (G, P), "mae_recon_loss")
    _mae_dense("mae_recon_loss", pred, pixels, d_pred)
    check(lib().vs_mae_recon_loss(L.dtype_code(d_pred.dtype), G, C, S, patch, int(len_keep), pred.data_ptr(), K,
                                  pixels.data_ptr(), ids_restore.data_ptr(), loss.data_ptr(), d_pred.data_ptr(), K,
                                  workspace.data_ptr(), stream()), "vs_mae_recon_loss")
    return loss


def embed_head_fwd(x, ldx, gamma, beta, eps, w, b, h, mean, rstd, z_raw, nrm, z):
    """Final LayerNorm -> projection -> L2-normalise on one row per image (vs_embed_head_fwd): image g's
    row starts at x.data_ptr() + g * ldx floats; h [G, D], mean / rstd / nrm [G], z_raw / z [G, E]."""
    require_device(x, gamma, beta, w, b, h, mean, rstd, z_raw, nrm, z)
    G, D = h.shape
    E = w.shape[0]
    if w.shape != (E, D) or z.shape != (G, E) or z_raw.shape != (G, E) or x.numel() < (G - 1) * ldx + D:
        raise L.VsError("embed_head_fwd: w [E, D], h [G, D], z / z_raw [G, E], x at least (G-1)*ldx + D elements")
    check(lib().vs_embed_head_fwd(G, D, E, x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), float(eps),
                                  w.data_ptr(), b.data_ptr(), h.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                  z_raw.data_ptr(), nrm.data_ptr(), z.data_ptr(), stream()), "vs_embed_head_fwd")
    return z


def embed_head_bwd_workspace_bytes(G, D, E):
    return int(lib().vs_embed_head_bwd_workspace_bytes(G, D, E))


def embed_head_bwd(dz, x, ldx, h, mean, rstd, z_raw, nrm, gamma, w, dx, dx_lp=None, dw=None, db=None, dgamma=None,
                   dbeta=None, workspace=None):
    """Backward of embed_head_fwd (vs_embed_head_bwd): dx [G, P+1, D] f32 gets the LayerNorm backward in row
    0 of every image and zeros elsewhere, dx_lp (bf16, optional) its rounding; dw [E, D], db [E], dgamma,
    dbeta [D] (all or none) are written, summed over images in ascending order."""
    require_device(dz, x, h, mean, rstd, z_raw, nrm, gamma, w, dx, dx_lp, dw, db, dgamma, dbeta, workspace)
    G, T, D = dx.shape
    E = w.shape[0]
    if (h.shape != (G, D) or dz.shape != (G, E) or z_raw.shape != (G, E) or not dx.is_contiguous()
            or x.numel() < (G - 1) * ldx + D or (dx_lp is not None and dx_lp.numel() != dx.numel())
            or (dw is not None and dw.shape != (E, D))):
        raise L.VsError("embed_head_bwd: dz / z_raw [G, E], h [G, D], dx (and dx_lp) [G, P+1, D] dense, dw [E, D]")
    if dw is not None and workspace is None:
        workspace = torch.empty(embed_head_bwd_workspace_bytes(G, D, E) // 4 + 4, dtype=torch.float32, device=dx.device)
    if workspace is not None and workspace.numel() * workspace.element_size() < embed_head_bwd_workspace_bytes(G, D, E):
        raise L.VsError("embed_head_bwd: workspace too small")
    check(lib().vs_embed_head_bwd(G, T - 1, D, E, dz.data_ptr(), x.data_ptr(), ldx, h.data_ptr(), mean.data_ptr(),
                                  rstd.data_ptr(), z_raw.data_ptr(), nrm.data_ptr(), gamma.data_ptr(), w.data_ptr(),
                                  dx.data_ptr(), ptr(dx_lp), ptr(dw), ptr(db), ptr(dgamma), ptr(dbeta), ptr(workspace),
                                  stream()), "vs_embed_head_bwd")
    return dx


def info_nce_workspace_bytes(n, m):
    return int(lib().vs_info_nce_workspace_bytes(n, m))


def info_nce(ref, pos, neg, out, log_inv_tau=None, d_ref=None, d_pos=None, d_neg=None, grad_scale=1.0,
             d_log_inv_tau=None, workspace=None):
    """InfoNCE of loss_utils.py:409-431 (vs_info_nce): out f32[3] = (loss, pos_loss, neg_loss); ref / pos
    [n, E], neg [m, E] f32 dense; log_inv_tau a device scalar (None: tau = 1); gradients optional."""
    require_device(ref, pos, neg, out, log_inv_tau, d_ref, d_pos, d_neg, d_log_inv_tau, workspace)
    n, E = ref.shape
    m = neg.shape[0]
    for t, shape in ((ref, (n, E)), (pos, (n, E)), (neg, (m, E)), (d_ref, (n, E)), (d_pos, (n, E)), (d_neg, (m, E))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()):
            raise L.VsError("info_nce: ref / pos [n, E], neg [m, E] (and their gradients) dense float32")
    if out.numel() < 3 or out.dtype != torch.float32:
        raise L.VsError("info_nce: out must hold three float32")
    need = info_nce_workspace_bytes(n, m)
    if workspace is None:
        workspace = torch.empty(need // 8 + 2, dtype=torch.float64, device=ref.device)
    elif workspace.numel() * workspace.element_size() < need:
        raise L.VsError("info_nce: workspace too small")
    check(lib().vs_info_nce(n, m, E, ref.data_ptr(), pos.data_ptr(), neg.data_ptr(), ptr(log_inv_tau), out.data_ptr(),
                            ptr(d_ref), ptr(d_pos), ptr(d_neg), float(grad_scale), ptr(d_log_inv_tau),
                            workspace.data_ptr(), stream()), "vs_info_nce")
    return out


def _rrr_dims(X, y, U, V, b, what):
    """(K, T, N, C, r) of the RRR operands after checking them: X [K, T, C+1] f64, y [K, T, N] f32 / f64,
    U [N, C, r], V [r, T], b [N, 1, T] f64, all dense."""
    K, T, C1 = X.shape
    N, C, r = U.shape
    ok = (C1 == C + 1 and tuple(y.shape) == (K, T, N) and tuple(V.shape) == (r, T) and b.numel() == N * T
          and y.dtype in (torch.float32, torch.float64)
          and all(t.dtype == torch.float64 for t in (X, U, V, b))
          and all(t.is_contiguous() for t in (X, y, U, V, b)))
    if not ok:
        raise L.VsError(f"{what}: X [K, T, C+1], U [N, C, r], V [r, T], b [N, 1, T] dense float64 and "
                        "y [K, T, N] dense float32 / float64")
    return K, T, N, C, r


def _f64_code(t):
    return L.VS_F64 if t.dtype == torch.float64 else L.VS_F32


def _rrr_grad_outputs(what, U, V, b, loss, dU, dV, db):
    """The output checks of the three *_loss_grad entries."""
    for g, ref in ((dU, U), (dV, V), (db, b)):
        if g is not None and (g.numel() != ref.numel() or g.dtype != torch.float64 or not g.is_contiguous()):
            raise L.VsError(f"{what}: dU / dV / db are dense float64 of the shapes of U / V / b")
    if loss.dtype != torch.float64 or loss.numel() < 1:
        raise L.VsError(f"{what}: loss must hold one float64")


def _rrr_score_outputs(what, K, T, N, mean_y, std_y, bps, r2, out, pred):
    """The checks of the three *_score entries on the statistics of y and the outputs."""
    for t, numel in ((mean_y, T * N), (std_y, T * N), (bps, N), (r2, N), (pred, K * T * N)):
        if t is not None and (t.numel() != numel or t.dtype != torch.float64 or not t.is_contiguous()):
            raise L.VsError(f"{what}: mean_y / std_y [T, N], bps / r2 [N], pred [K, T, N] dense float64")
    if out.dtype != torch.float64 or out.numel() < 2:
        raise L.VsError(f"{what}: out must hold two float64")


def _rrr_workspace(what, need, workspace, device):
    """A workspace of `need` bytes: a new one, or the caller's after checking its size."""
    if workspace is None:
        return torch.empty(need // 8 + 2, dtype=torch.float64, device=device)
    if workspace.numel() * workspace.element_size() < need:
        raise L.VsError(f"{what}: workspace too small")
    return workspace


def rrr_loss_grad_workspace_bytes(K, T, N, C):
    return int(lib().vs_rrr_loss_grad_workspace_bytes(K, T, N, C))


def rrr_loss_grad(X, y, U, V, b, l2, loss, dU=None, dV=None, db=None, workspace=None):
    """The RRR loss sum (yhat - y)^2 + l2 sum beta^2 into `loss` (f64[1]) and, when dU / dV / db are given
    (together), its gradients (vs_rrr_loss_grad).  1 <= C <= 32, 1 <= r <= 8."""
    require_device(X, y, U, V, b, loss, dU, dV, db, workspace)
    K, T, N, C, r = _rrr_dims(X, y, U, V, b, "rrr_loss_grad")
    _rrr_grad_outputs("rrr_loss_grad", U, V, b, loss, dU, dV, db)
    workspace = _rrr_workspace("rrr_loss_grad", rrr_loss_grad_workspace_bytes(K, T, N, C), workspace, X.device)
    check(lib().vs_rrr_loss_grad(K, T, N, C, r, X.data_ptr(), y.data_ptr(), _f64_code(y), U.data_ptr(), V.data_ptr(),
                                 b.data_ptr(), float(l2), loss.data_ptr(), ptr(dU), ptr(dV), ptr(db),
                                 workspace.data_ptr(), stream()), "vs_rrr_loss_grad")
    return loss


def rrr_score_workspace_bytes(K, N):
    return int(lib().vs_rrr_score_workspace_bytes(K, N))


def rrr_score(X, U, V, b, mean_y, std_y, gt, bps, r2, out, pred=None, workspace=None):
    """train_rrr's scoring on the held-out trials (vs_rrr_score): pred = max(yhat std_y + mean_y, 1e-3)
    (written when `pred` [K, T, N] f64 is given), per-neuron bits per spike `bps` [N] and trial-mean R^2 `r2`
    [N], and out f64[2] = their NaN-ignoring means over neurons (co_bps, mean R^2)."""
    require_device(X, U, V, b, mean_y, std_y, gt, bps, r2, out, pred, workspace)
    K, T, N, C, r = _rrr_dims(X, gt, U, V, b, "rrr_score")
    _rrr_score_outputs("rrr_score", K, T, N, mean_y, std_y, bps, r2, out, pred)
    workspace = _rrr_workspace("rrr_score", rrr_score_workspace_bytes(K, N), workspace, X.device)
    check(lib().vs_rrr_score(K, T, N, C, r, X.data_ptr(), U.data_ptr(), V.data_ptr(), b.data_ptr(), mean_y.data_ptr(),
                             std_y.data_ptr(), gt.data_ptr(), _f64_code(gt), ptr(pred), bps.data_ptr(), r2.data_ptr(),
                             out.data_ptr(), workspace.data_ptr(), stream()), "vs_rrr_score")
    return out


def rrr_wide_loss_grad_workspace_bytes(K, T, N, C):
    return int(lib().vs_rrr_wide_loss_grad_workspace_bytes(K, T, N, C))


def rrr_wide_loss_grad(X, y, U, V, b, l2, loss, dU=None, dV=None, db=None, workspace=None):
    """rrr_loss_grad for 1 <= C <= 1024 features (vs_rrr_wide_loss_grad: the two products per time bin on the
    float64 MFMA).  The same operands, results and checks; 1 <= r <= 8."""
    require_device(X, y, U, V, b, loss, dU, dV, db, workspace)
    K, T, N, C, r = _rrr_dims(X, y, U, V, b, "rrr_wide_loss_grad")
    _rrr_grad_outputs("rrr_wide_loss_grad", U, V, b, loss, dU, dV, db)
    workspace = _rrr_workspace("rrr_wide_loss_grad", rrr_wide_loss_grad_workspace_bytes(K, T, N, C), workspace,
                               X.device)
    check(lib().vs_rrr_wide_loss_grad(K, T, N, C, r, X.data_ptr(), y.data_ptr(), _f64_code(y), U.data_ptr(),
                                      V.data_ptr(), b.data_ptr(), float(l2), loss.data_ptr(), ptr(dU), ptr(dV),
                                      ptr(db), workspace.data_ptr(), stream()), "vs_rrr_wide_loss_grad")
    return loss


def rrr_wide_score_workspace_bytes(K, T, N):
    return int(lib().vs_rrr_wide_score_workspace_bytes(K, T, N))


def rrr_wide_score(X, U, V, b, mean_y, std_y, gt, bps, r2, out, pred=None, workspace=None):
    """rrr_score for 1 <= C <= 1024 features (vs_rrr_wide_score): the same operands, results and checks."""
    require_device(X, U, V, b, mean_y, std_y, gt, bps, r2, out, pred, workspace)
    K, T, N, C, r = _rrr_dims(X, gt, U, V, b, "rrr_wide_score")
    _rrr_score_outputs("rrr_wide_score", K, T, N, mean_y, std_y, bps, r2, out, pred)
    workspace = _rrr_workspace("rrr_wide_score", rrr_wide_score_workspace_bytes(K, T, N), workspace, X.device)
    check(lib().vs_rrr_wide_score(K, T, N, C, r, X.data_ptr(), U.data_ptr(), V.data_ptr(), b.data_ptr(),
                                  mean_y.data_ptr(), std_y.data_ptr(), gt.data_ptr(), _f64_code(gt), ptr(pred),
                                  bps.data_ptr(), r2.data_ptr(), out.data_ptr(), workspace.data_ptr(), stream()),
          "vs_rrr_wide_score")
    return out


# ---- the RRR baseline straight from the pixels (csrc/rrr_pixel.hip): X [K, F, C] uint8 / float32, stored once ----
RRR_PIXEL_MAX_FEATURES, RRR_PIXEL_MAX_COMPONENTS = 32768, 4


def _rrr_pixel_x(X, what):
    require_device(X)
    if X.dim() != 3 or X.dtype not in (torch.uint8, torch.float32) or not X.is_contiguous():
        raise L.VsError(f"{what}: X [K, F, C] dense uint8 / float32")
    return L.VS_U8 if X.dtype == torch.uint8 else L.VS_F32


def _rrr_pixel_dims(X, idx, mean, std, y, U, V, b, what):
    """(K, F, T, N, C, r, x dtype code) of the pixel RRR operands after checking them: X [K, F, C] uint8 / float32,
    idx [T] int64 frame indices on the device, mean / std [F, C] float64 (uint8 X) or float32 (float32 X),
    y [K, T, N] float32 / float64, U [N, C, r], V [r, T], b [N, 1, T] float64, all dense."""
    code = _rrr_pixel_x(X, what)
    K, F, C = X.shape
    stat = torch.float64 if X.dtype == torch.uint8 else torch.float32
    N, Cu, r = U.shape
    T = V.shape[1] if V.dim() == 2 else -1
    ok = (Cu == C and tuple(y.shape) == (K, T, N) and tuple(V.shape) == (r, T) and b.numel() == N * T
          and y.dtype in (torch.float32, torch.float64) and idx.dtype == torch.int64 and tuple(idx.shape) == (T,)
          and all(tuple(t.shape) == (F, C) and t.dtype == stat for t in (mean, std))
          and all(t.dtype == torch.float64 for t in (U, V, b))
          and all(t.is_contiguous() for t in (idx, mean, std, y, U, V, b)))
    if not ok:
        raise L.VsError(f"{what}: X [K, F, C] uint8 / float32, idx [T] int64, mean / std [F, C] float64 (uint8 X) or "
                        "float32 (float32 X), U [N, C, r], V [r, T], b [N, 1, T] dense float64 and y [K, T, N] dense "
                        "float32 / float64")
    return K, F, T, N, C, r, code


def rrr_pixel_stats(X, mean=None, std=None):
    """(mean, std) [F, C] over the trials of X [K, F, C] uint8 / float32 with numpy's roundings: np.mean, np.std
    and np.clip(., 1e-8, None) along axis 0, bit for bit (vs_rrr_pixel_stats).  float64 for uint8 X, float32 for
    float32 X, as numpy gives them."""
    code = _rrr_pixel_x(X, "rrr_pixel_stats")
    K, F, C = X.shape
    stat = torch.float64 if X.dtype == torch.uint8 else torch.float32
    if mean is None:
        mean = torch.empty(F, C, dtype=stat, device=X.device)
    if std is None:
        std = torch.empty(F, C, dtype=stat, device=X.device)
    require_device(mean, std)
    for t in (mean, std):
        if tuple(t.shape) != (F, C) or t.dtype != stat or not t.is_contiguous():
            raise L.VsError("rrr_pixel_stats: mean / std are dense [F, C], float64 for uint8 X and float32 for float32 X")
    check(lib().vs_rrr_pixel_stats(K, F, C, X.data_ptr(), code, mean.data_ptr(), std.data_ptr(), stream()),
          "vs_rrr_pixel_stats")
    return mean, std


def rrr_pixel_loss_grad_workspace_bytes(K, T, N, C, r):
    return int(lib().vs_rrr_pixel_loss_grad_workspace_bytes(K, T, N, C, r))


def rrr_pixel_loss_grad(X, idx, mean, std, y, U, V, b, l2, loss, dU=None, dV=None, db=None, workspace=None):
    """rrr_wide_loss_grad for one session whose features are the pixels of X [K, F, C] uint8 / float32, 1 <= C <=
    32768 (vs_rrr_pixel_loss_grad): time bin t reads frame idx[t], standardised with mean / std [F, C] at the
    operand load; the bias column is implicit.  The same results and checks; 1 <= r <= 4.  The caller guarantees
    0 <= idx < F (PixelFeatures checks it once); the kernel clamps."""
    require_device(X, idx, mean, std, y, U, V, b, loss, dU, dV, db, workspace)
    K, F, T, N, C, r, code = _rrr_pixel_dims(X, idx, mean, std, y, U, V, b, "rrr_pixel_loss_grad")
    _rrr_grad_outputs("rrr_pixel_loss_grad", U, V, b, loss, dU, dV, db)
    workspace = _rrr_workspace("rrr_pixel_loss_grad", rrr_pixel_loss_grad_workspace_bytes(K, T, N, C, r), workspace,
                               X.device)
    check(lib().vs_rrr_pixel_loss_grad(K, F, T, N, C, r, X.data_ptr(), code, idx.data_ptr(), mean.data_ptr(),
                                       std.data_ptr(), y.data_ptr(), _f64_code(y), U.data_ptr(), V.data_ptr(),
                                       b.data_ptr(), float(l2), loss.data_ptr(), ptr(dU), ptr(dV), ptr(db),
                                       workspace.data_ptr(), stream()), "vs_rrr_pixel_loss_grad")
    return loss


def rrr_pixel_score_workspace_bytes(K, T, N):
    return int(lib().vs_rrr_pixel_score_workspace_bytes(K, T, N))


def rrr_pixel_score(X, idx, mean, std, U, V, b, mean_y, std_y, gt, bps, r2, out, pred=None, workspace=None):
    """rrr_wide_score for pixel features (vs_rrr_pixel_score): the operands of rrr_pixel_loss_grad, the results
    and checks of rrr_wide_score."""
    require_device(X, idx, mean, std, U, V, b, mean_y, std_y, gt, bps, r2, out, pred, workspace)
    K, F, T, N, C, r, code = _rrr_pixel_dims(X, idx, mean, std, gt, U, V, b, "rrr_pixel_score")
    _rrr_score_outputs("rrr_pixel_score", K, T, N, mean_y, std_y, bps, r2, out, pred)
    workspace = _rrr_workspace("rrr_pixel_score", rrr_pixel_score_workspace_bytes(K, T, N), workspace, X.device)
    check(lib().vs_rrr_pixel_score(K, F, T, N, C, r, X.data_ptr(), code, idx.data_ptr(), mean.data_ptr(),
                                   std.data_ptr(), U.data_ptr(), V.data_ptr(), b.data_ptr(), mean_y.data_ptr(),
                                   std_y.data_ptr(), gt.data_ptr(), _f64_code(gt), ptr(pred), bps.data_ptr(),
                                   r2.data_ptr(), out.data_ptr(), workspace.data_ptr(), stream()),
          "vs_rrr_pixel_score")
    return out


def gauss_weights(sigma):
    """(weights float64 [2 radius + 1], radius) of scipy.ndimage.gaussian_filter1d(., sigma) with its default
    truncate = 4, computed as scipy's _gaussian_kernel1d does."""
    sigma = float(sigma)
    if not sigma > 0:
        raise L.VsError("gauss_smooth_time: sigma must be positive")
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum(), radius


def gauss_smooth_time(y, sigma, out=None):
    """scipy.ndimage.gaussian_filter1d(y, sigma, axis=1) (mode 'reflect') for y [K, T, N] float32 / float64 on
    the device, bit for bit (vs_gauss_smooth_time).  T >= radius + 1 with radius = int(4 sigma + 0.5)."""
    require_device(y, out)
    if y.dim() != 3 or y.dtype not in (torch.float32, torch.float64) or not y.is_contiguous():
        raise L.VsError("gauss_smooth_time: y [K, T, N] dense float32 / float64")
    w, radius = gauss_weights(sigma)
    K, T, N = y.shape
    if T < radius + 1:
        raise L.VsError(f"gauss_smooth_time: T = {T} < radius + 1 = {radius + 1} (one reflection at each end)")
    if out is None:
        out = torch.empty_like(y)
    elif out.shape != y.shape or out.dtype != y.dtype or not out.is_contiguous() or out.data_ptr() == y.data_ptr():
        raise L.VsError("gauss_smooth_time: out is a dense tensor of y's shape and dtype, not y itself")
    wd = torch.from_numpy(w).to(y.device)
    check(lib().vs_gauss_smooth_time(K, T, N, y.data_ptr(), _f64_code(y), wd.data_ptr(), radius, out.data_ptr(),
                                     stream()), "vs_gauss_smooth_time")
    return out


# ---- PCA by subspace iteration (csrc/pca.hip): X [M, D] uint8 / float32 stored once, never centred in memory ----
def pca_tiles() -> dict:
    """The tile constants of csrc/pca.hip a test places its shapes by (vs_pca_tiles)."""
    buf = (L.c_i32 * 4)()
    check(lib().vs_pca_tiles(buf), "vs_pca_tiles")
    return dict(zip(("rows", "cols", "chunk_rows", "max_chunks"), (int(v) for v in buf)))


def _pca_x(X, what):
    require_device(X)
    if X.dim() != 2 or X.dtype not in (torch.uint8, torch.float32) or not X.is_contiguous():
        raise L.VsError(f"{what}: X [M, D] dense uint8 / float32")
    return X.shape[0], X.shape[1], (L.VS_U8 if X.dtype == torch.uint8 else L.VS_F32)


def _pca_f64(t, shape, what, name):
    require_device(t)
    if t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise L.VsError(f"{what}: {name} must be dense float64 of shape {tuple(shape)}")


def _pca_ws(workspace, need, device, what):
    if workspace is None:
        return torch.empty(need // 8 + 2, dtype=torch.float64, device=device)
    require_device(workspace)
    if workspace.numel() * workspace.element_size() < need:
        raise L.VsError(f"{what}: workspace too small")
    return workspace


def pca_colmean_workspace_bytes(M, D):
    return int(lib().vs_pca_colmean_workspace_bytes(M, D))


def pca_colmean(X, mu=None, workspace=None):
    """mu [D] float64 = the column means of X [M, D] (vs_pca_colmean), summed in an order fixed by (M, D)."""
    M, D, code = _pca_x(X, "pca_colmean")
    if mu is None:
        mu = torch.empty(D, dtype=torch.float64, device=X.device)
    _pca_f64(mu, (D,), "pca_colmean", "mu")
    ws = _pca_ws(workspace, pca_colmean_workspace_bytes(M, D), X.device, "pca_colmean")
    check(lib().vs_pca_colmean(M, D, X.data_ptr(), code, mu.data_ptr(), ws.data_ptr(), stream()), "vs_pca_colmean")
    return mu


def pca_project_workspace_bytes(M, D, Lq):
    return int(lib().vs_pca_project_workspace_bytes(M, D, Lq))


def pca_project(X, mu, Q, Y=None, workspace=None):
    """Y [M, L] float64 = (X - 1 mu^T) Q for Q [D, L] float64, 1 <= L <= 32 (vs_pca_project)."""
    M, D, code = _pca_x(X, "pca_project")
    _pca_f64(mu, (D,), "pca_project", "mu")
    if Q.dim() != 2:
        raise L.VsError("pca_project: Q [D, L]")
    Lq = Q.shape[1]
    _pca_f64(Q, (D, Lq), "pca_project", "Q")
    if Y is None:
        Y = torch.empty(M, Lq, dtype=torch.float64, device=X.device)
    _pca_f64(Y, (M, Lq), "pca_project", "Y")
    ws = _pca_ws(workspace, pca_project_workspace_bytes(M, D, Lq), X.device, "pca_project")
    check(lib().vs_pca_project(M, D, Lq, X.data_ptr(), code, mu.data_ptr(), Q.data_ptr(), Y.data_ptr(), ws.data_ptr(),
                               stream()), "vs_pca_project")
    return Y


def pca_gram_apply_workspace_bytes(M, D, Lq):
    return int(lib().vs_pca_gram_apply_workspace_bytes(M, D, Lq))


def pca_gram_apply(X, mu, Q, W=None, workspace=None):
    """W [D, L] float64 = Xc^T (Xc Q) with Xc = X - 1 mu^T: one step of the subspace iteration
    (vs_pca_gram_apply)."""
    M, D, code = _pca_x(X, "pca_gram_apply")
    _pca_f64(mu, (D,), "pca_gram_apply", "mu")
    if Q.dim() != 2:
        raise L.VsError("pca_gram_apply: Q [D, L]")
    Lq = Q.shape[1]
    _pca_f64(Q, (D, Lq), "pca_gram_apply", "Q")
    if W is None:
        W = torch.empty(D, Lq, dtype=torch.float64, device=X.device)
    _pca_f64(W, (D, Lq), "pca_gram_apply", "W")
    ws = _pca_ws(workspace, pca_gram_apply_workspace_bytes(M, D, Lq), X.device, "pca_gram_apply")
    check(lib().vs_pca_gram_apply(M, D, Lq, X.data_ptr(), code, mu.data_ptr(), Q.data_ptr(), W.data_ptr(),
                                  ws.data_ptr(), stream()), "vs_pca_gram_apply")
    return W


def poisson_nll(log_rate, target, loss_out, dx=None, grad_scale=1.0, workspace=None):
    require_device(log_rate, target, loss_out)
    n = log_rate.numel()
    if workspace is None:
        workspace = torch.empty(int(lib().vs_poisson_workspace_bytes(n)) // 4, dtype=torch.float32,
                                device=log_rate.device)
    check(lib().vs_poisson_nll(n, log_rate.data_ptr(), target.data_ptr(), loss_out.data_ptr(), ptr(dx), grad_scale,
                               workspace.data_ptr(), stream()), "vs_poisson_nll")
    return loss_out


def poisson_nll_bwd(log_rate, target, grad_out, dx):
    require_device(log_rate, target, grad_out, dx)
    check(lib().vs_poisson_nll_bwd(log_rate.numel(), log_rate.data_ptr(), target.data_ptr(), grad_out.data_ptr(),
                                   dx.data_ptr(), stream()), "vs_poisson_nll_bwd")
    return dx


def mse_loss(pred, target, loss_out, dx=None, grad_scale=1.0, workspace=None):
    """mean((pred - target)^2) into loss_out (device scalar); dx = grad_scale * 2 (pred - target) / n."""
    require_device(pred, target, loss_out)
    n = pred.numel()
    if workspace is None:
        workspace = torch.empty(int(lib().vs_poisson_workspace_bytes(n)) // 4, dtype=torch.float32, device=pred.device)
    check(lib().vs_mse_loss(n, pred.data_ptr(), target.data_ptr(), loss_out.data_ptr(), ptr(dx), grad_scale,
                            workspace.data_ptr(), stream()), "vs_mse_loss")
    return loss_out


def mse_loss_bwd(pred, target, grad_out, dx):
    require_device(pred, target, grad_out, dx)
    check(lib().vs_mse_loss_bwd(pred.numel(), pred.data_ptr(), target.data_ptr(), grad_out.data_ptr(), dx.data_ptr(),
                                stream()), "vs_mse_loss_bwd")
    return dx


def adamw(param, grad, exp_avg, exp_avg_sq, hyper, param_lp=None):
    require_device(param, grad, exp_avg, exp_avg_sq, hyper)
    check(lib().vs_adamw(param.numel(), param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                         ptr(param_lp), hyper.data_ptr(), stream()), "vs_adamw")


def vit_layer_fwd(layer_struct):
    check(lib().vs_vit_layer_fwd(ctypes.byref(layer_struct), stream()), "vs_vit_layer_fwd")


def vit_layer_bwd(layer_struct, grad_struct):
    check(lib().vs_vit_layer_bwd(ctypes.byref(layer_struct), ctypes.byref(grad_struct), stream()),
          "vs_vit_layer_bwd")


# ---- timing (bench instrumentation) -----------------------------------------------------------
def timing_enable(mask: int):
    """mask: OR of (1 << TIMER_*); 0 disables and discards recorded events."""
    check(lib().vs_timing_enable(int(mask)), "vs_timing_enable")


def timing_collect(timer: int, with_bytes: bool = False):
    """(launches, total ms) of one timer, and its total algorithmic bytes with `with_bytes`."""
    n = ctypes.c_int64(0)
    ms = ctypes.c_double(0.0)
    nb = ctypes.c_double(0.0)
    check(lib().vs_timing_bytes(timer, ctypes.byref(nb)), "vs_timing_bytes")
    check(lib().vs_timing_collect(timer, ctypes.byref(n), ctypes.byref(ms)), "vs_timing_collect")
    return (int(n.value), float(ms.value), float(nb.value)) if with_bytes else (int(n.value), float(ms.value))


def attn_scale(head_dim: int = 64) -> float:
    return 1.0 / math.sqrt(head_dim)


def video_preprocess(video, frame_idx, size=224, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), out=None):
    """K0 on the device (videomae.py:18-25): raw (B, T, 1, H, W) float32 (integer-valued 0..255) or
    uint8 video -> pixel_values (B, len(frame_idx), 3, size, size) f32, bit-identical to the
    reference's HF image processor.  frame_idx: host sequence of source frame indices."""
    require_device(video)
    if video.dim() != 5 or video.shape[2] != 1:
        raise L.VsError("video_preprocess: expected (B, T, 1, H, W)")
    if video.dtype == torch.uint8:
        code = L.VS_U8
    elif video.dtype == torch.float32:
        code = L.VS_F32
    else:
        raise L.VsError("video_preprocess: float32 or uint8 frames")
    video = video.contiguous()
    B, T, _, H, W = video.shape
    idx = [int(i) for i in frame_idx]
    if out is None:
        out = torch.empty(B, len(idx), 3, size, size, dtype=torch.float32, device=video.device)
    fi = (ctypes.c_int32 * len(idx))(*idx)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    sd = (ctypes.c_float * 3)(*[float(v) for v in std])
    check(lib().vs_video_preprocess(code, B, T, H, W, video.data_ptr(), fi, len(idx), size, m, sd, out.data_ptr(),
                                    stream()), "vs_video_preprocess")
    return out


# ---- the contrastive loader's frame transform (csrc/contrast_loader.hip) ----
def contrast_frames_plan(H, W, size) -> dict:
    """How vs_contrast_frames splits (H, W) -> size: what a test places its shapes by (vs_contrast_frames_plan)."""
    buf = (L.c_i32 * 6)()
    check(lib().vs_contrast_frames_plan(int(H), int(W), int(size), buf), "vs_contrast_frames_plan")
    return dict(zip(("rows", "bands", "src_rows", "taps_w", "taps_h", "lds_bytes"), (int(v) for v in buf)))


_CONTRAST_TABLES = {}     # (device, stream, H, W, S) -> the f64 weight tables vs_contrast_frames filled on that stream


def contrast_frames(video, idx, size=144, mean=0.5, std=0.5, out=None, check_idx=True):
    """out (G, 1, size, size) f32 = Normalize(mean, std)(Resize((size, size))(video[idx] / 255)): the reference's
    per-frame transform (src/loader/contrast.py:65-93 with src/pretrain.py:60-66) in one launch (vs_contrast_frames).
    video (F, 1, H, W) uint8 or float32 on the device, idx G int64 source-frame numbers on the device.
    check_idx: the indices are checked against [0, F) on the host before the launch, which waits for `idx`; a
    caller that drew them on the host (vspike.data.ContrastFrames) checks there and passes False.  Unchecked, an
    index out of range reads nothing and gives a frame of NaN.
    The weight tables of a geometry (a few KB) are filled by the first call on a stream and kept for the later ones."""
    require_device(video, idx, out)
    if video.dim() != 4 or video.shape[1] != 1:
        raise L.VsError("contrast_frames: video (F, 1, H, W)")
    if video.dtype == torch.uint8:
        code = L.VS_U8
    elif video.dtype == torch.float32:
        code = L.VS_F32
    else:
        raise L.VsError("contrast_frames: float32 or uint8 frames")
    if not video.is_contiguous():
        raise L.VsError("contrast_frames: video must be dense (it is stored once; no copy is made here)")
    if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous() or idx.device != video.device:
        raise L.VsError("contrast_frames: idx must be a dense 1-D int64 tensor on the video's device")
    F, _, H, W = video.shape
    G, S = idx.numel(), int(size)
    need = int(lib().vs_contrast_frames_workspace_bytes(H, W, S))
    if need == 0:
        raise L.VsError("contrast_frames: 1 <= size <= 512 and 1 <= H, W <= 8 size")
    if check_idx and G and (int(idx.min()) < 0 or int(idx.max()) >= F):
        raise L.VsError(f"contrast_frames: frame index outside [0, {F})")
    if out is None:
        out = torch.empty(G, 1, S, S, dtype=torch.float32, device=video.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (G, 1, S, S) or not out.is_contiguous() or \
            out.device != video.device:
        raise L.VsError(f"contrast_frames: out must be a dense float32 ({G}, 1, {S}, {S}) tensor on the video's device")
    st = stream()
    key = (video.device.index, st.value, H, W, S)
    table = _CONTRAST_TABLES.get(key)
    ready = table is not None
    if not ready:
        table = torch.empty(need // 8, dtype=torch.float64, device=video.device)
    check(lib().vs_contrast_frames(code, F, H, W, video.data_ptr(), idx.data_ptr(), G, S, float(mean), float(std),
                                   out.data_ptr(), table.data_ptr(), int(ready), st), "vs_contrast_frames")
    if G:
        _CONTRAST_TABLES[key] = table
    return out


# ---- behaviour features of the RRR baselines (csrc/flow_features.hip) ----
FLOW_MAX_PIXELS = 1 << 20


def flow_plan() -> dict:
    """The sizes at which the flow kernels change path (vs_flow_plan): `stage_max`, the largest H W whose keys
    flow_median2 keeps in LDS; `quantile_chunk`, the pixels one workgroup of flow_quantiles counts per pass."""
    buf = (L.c_i32 * 3)()
    check(lib().vs_flow_plan(buf), "vs_flow_plan")
    return {"stage_max": int(buf[0]), "quantile_chunk": int(buf[1]), "median_threads": int(buf[2])}


def _flow_dims(flow, what):
    """(K, F - 1, H W) of a flow field (K, F - 1, H, W, 2): dense float32 on the device."""
    require_device(flow)
    if flow.dim() != 5 or flow.shape[4] != 2 or flow.dtype != torch.float32 or not flow.is_contiguous():
        raise L.VsError(f"{what}: flow (K, F - 1, H, W, 2) dense float32")
    K, Fp, H, W, _ = flow.shape
    if Fp < 1 or not 1 <= H * W <= FLOW_MAX_PIXELS:
        raise L.VsError(f"{what}: at least one flow frame of 1 <= H W <= 2^20 pixels")
    return K, Fp, H * W


def flow_median2(flow, absolute=False):
    """(K, F - 1, 2) float32: np.median over (h, w) of each component of each frame of flow (K, F - 1, H, W, 2), of
    the signed values or (absolute=True) of |flow|, bit for bit (vs_flow_median2).  A NaN in a component of a frame gives NaN for
    that component."""
    K, Fp, HW = _flow_dims(flow, "flow_median2")
    out = torch.empty(K, Fp, 2, dtype=torch.float32, device=flow.device)
    check(lib().vs_flow_median2(K * Fp, HW, flow.data_ptr(), int(bool(absolute)), out.data_ptr(), stream()),
          "vs_flow_median2")
    return out


def flow_quantiles(flow, q=(10, 90), with_stats=False, workspace=None):
    """(K, 2, 2) float32: [trial, component] -> (np.percentile(x, q[0]), np.percentile(x, q[1])) of
    x = |flow[trial, ..., component]| as numpy 2 computes them for a float32 array and a scalar q (vs_flow_quantiles).
    with_stats: also the (K, 2, 4) order statistics the two are interpolated between."""
    K, Fp, HW = _flow_dims(flow, "flow_quantiles")
    if K > 65535 or Fp * HW >= 1 << 31:
        raise L.VsError("flow_quantiles: at most 65535 trials of fewer than 2^31 values per component")
    if len(q) != 2 or not all(0 <= float(v) <= 100 for v in q):
        raise L.VsError("flow_quantiles: q holds two percentiles in [0, 100]")
    bounds = torch.empty(K, 2, 2, dtype=torch.float32, device=flow.device)
    stats = torch.empty(K, 2, 4, dtype=torch.float32, device=flow.device) if with_stats else None
    if K:
        need = int(lib().vs_flow_quantiles_workspace_bytes(K))
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=flow.device)
        elif workspace.device != flow.device or workspace.numel() * workspace.element_size() < need \
                or not workspace.is_contiguous():
            raise L.VsError(f"flow_quantiles: workspace of {need} bytes on the flow's device")
        check(lib().vs_flow_quantiles(K, Fp, HW, flow.data_ptr(), float(q[0]), float(q[1]), bounds.data_ptr(),
                                      ptr(stats), workspace.data_ptr(), stream()), "vs_flow_quantiles")
    return (bounds, stats) if with_stats else bounds


def flow_clip_mean(flow, bounds):
    """(K, F - 1) float32: the mean over (h, w, 2) of clip(|flow|, bounds[k, c, 0], bounds[k, c, 1]) per frame, an
    f64 sum rounded once (vs_flow_clip_mean).  bounds (K, 2, 2) float32 as flow_quantiles returns them."""
    K, Fp, HW = _flow_dims(flow, "flow_clip_mean")
    require_device(bounds)
    if tuple(bounds.shape) != (K, 2, 2) or bounds.dtype != torch.float32 or not bounds.is_contiguous() \
            or bounds.device != flow.device:
        raise L.VsError("flow_clip_mean: bounds (K, 2, 2) dense float32 on the flow's device")
    out = torch.empty(K, Fp, dtype=torch.float32, device=flow.device)
    check(lib().vs_flow_clip_mean(K, Fp, HW, flow.data_ptr(), bounds.data_ptr(), out.data_ptr(), stream()),
          "vs_flow_clip_mean")
    return out


def motion_energy(video):
    """(K, F - 1) float32: the mean over the pixels of |video[k, f + 1] - video[k, f]| for video (K, F, H, W) uint8
    or float32, read in place (vs_motion_energy).  uint8: integer differences, an exact sum."""
    require_device(video)
    if video.dim() != 4 or video.dtype not in (torch.uint8, torch.float32) or not video.is_contiguous():
        raise L.VsError("motion_energy: video (K, F, H, W) dense uint8 / float32 (it is read in place; no copy is made)")
    K, F, H, W = video.shape
    if F < 2 or not 1 <= H * W <= FLOW_MAX_PIXELS:
        raise L.VsError("motion_energy: at least two frames of 1 <= H W <= 2^20 pixels")
    out = torch.empty(K, F - 1, dtype=torch.float32, device=video.device)
    code = L.VS_U8 if video.dtype == torch.uint8 else L.VS_F32
    check(lib().vs_motion_energy(code, K, F, H * W, video.data_ptr(), out.data_ptr(), stream()), "vs_motion_energy")
    return out
