"""Host-side contract of the head-dim-32 attention entries (no kernel is launched here)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from vspike import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_abi_version_and_workspace(lib):
    assert lib.vs_version() >= 15
    # delta [B, H, N] f32, padded to 256 bytes
    assert lib.vs_attn32_bwd_workspace_bytes(128, 82, 16) == 128 * 82 * 16 * 4
    assert lib.vs_attn32_bwd_workspace_bytes(1, 1, 1) == 256


def test_attn32_rejects_bad_arguments_without_launching(lib):
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    for dtype in (0, 1):
        assert lib.vs_attn32_fwd(dtype, 1, 257, 1, p, 96, p, 32, p, 0.17, None) == -1
        assert b"1..256" in lib.vs_last_error()
        assert lib.vs_attn32_bwd(dtype, 1, 257, 1, p, 96, p, 32, p, 32, p, p, 96, p, 0.17, None) == -1
        assert b"1..256" in lib.vs_last_error()
        assert lib.vs_attn32_fwd(dtype, 1, 10, 1, None, 96, None, 32, None, 0.17, None) == -1
        assert b"null pointer" in lib.vs_last_error()
        assert lib.vs_attn32_bwd(dtype, 1, 10, 1, p, 96, p, 32, p, 32, p, p, 96, None, 0.17, None) == -1
        assert b"null pointer" in lib.vs_last_error()
        assert lib.vs_attn32_fwd(dtype, 1, 10, 2, p, 96, p, 64, p, 0.17, None) == -1
        assert b"leading dims" in lib.vs_last_error()
        assert lib.vs_attn32_fwd(dtype, 1, 10, 1, p + 4, 96, p, 32, p, 0.17, None) == -1
        assert b"aligned" in lib.vs_last_error()
        assert lib.vs_attn32_fwd(dtype, 0, 10, 1, p, 96, p, 32, p, 0.17, None) == -1
        assert b"empty" in lib.vs_last_error()
    assert lib.vs_attn32_fwd(3, 1, 10, 1, p, 96, p, 32, p, 0.17, None) == -1      # VS_FP8
    assert b"dtype" in lib.vs_last_error()


def test_vit_layer_accepts_heads_times_32_up_to_256_tokens(lib):
    from vspike import _lib as L
    s = L.VitLayer()
    s.dtype, s.heads, s.batch, s.tokens, s.hidden, s.mlp = L.VS_F32, 2, 1, 257, 64, 128
    assert lib.vs_vit_layer_fwd(ctypes.byref(s), None) == -1
    assert b"256 tokens" in lib.vs_last_error()
    s.tokens, s.dtype = 10, L.VS_FP8
    assert lib.vs_vit_layer_fwd(ctypes.byref(s), None) == -1
    s.dtype, s.hidden = L.VS_F32, 96        # neither heads * 64 nor heads * 32
    assert lib.vs_vit_layer_fwd(ctypes.byref(s), None) == -1
    assert b"heads*64 or heads*32" in lib.vs_last_error()
