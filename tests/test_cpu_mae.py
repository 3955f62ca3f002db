"""MAE on the CPU: the float64 restatement (tests/mae_ref.py) against HF's pinned outputs (tests/golden/mae.npz), the
condition on the fixture's noise, and the host side of the plugin and of the csrc/mae.hip entries."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mae_ref as mr
from oracle import cpu_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden):
    return golden("mae.npz")


@pytest.fixture(scope="module")
def lib():
    from vspike import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("geom", list(mr.GEOMETRIES))
def test_noise_condition(fx, geom):
    """A condition on the inputs: every row of `noise` has pairwise gaps >= 1e-3 (argsort is unambiguous on any
    device) and every image has a masked patch; the stored noise is the one mae_ref derives."""
    noise = fx[f"{geom}/noise"]
    assert np.array_equal(noise, mr.make_noise(geom))
    keep = mr.len_keep(geom)
    assert mr.noise_ok(noise, keep)
    assert not mr.noise_ok(np.full_like(noise, 0.5), keep)
    mask = fx[f"{geom}/mask"]
    assert (mask.sum(1) == noise.shape[1] - keep).all() and (mask.sum(1) >= 1).all()
    _, restore = mr.indices(torch.from_numpy(noise), keep)
    assert np.array_equal(restore.numpy(), fx[f"{geom}/ids_restore"])
    assert np.array_equal((restore >= keep).float().numpy(), mask)
    assert {"g1": 2, "g2": 32}[geom] == keep


@pytest.mark.parametrize("geom", list(mr.GEOMETRIES))
def test_restatement_matches_hf(fx, geom):
    """float64 restatement against HF's float64 run (whose softmax is float32: its own error is `hf32_err`-sized,
    about 1e-6).  Bars: a tenth of the project's fp32 bars (outputs 1e-5 of max|ref|, loss 1e-6, gradients 1e-4)."""
    P = mr.to_torch(mr.make_params(geom))
    x = torch.from_numpy(mr.make_images(geom)).double()
    out = mr.forward(x, torch.from_numpy(mr.make_noise(geom)), P, geom)
    for k in ("z", "latent", "logits"):
        ref = fx[f"{geom}/{k}"].astype(np.float64)
        assert np.abs(out[k].detach().numpy() - ref).max() <= 1e-5 * np.abs(ref).max(), k
    assert abs(out["recon_loss"].item() - fx[f"{geom}/recon_loss"][0]) <= 1e-6 * fx[f"{geom}/recon_loss"][0]
    assert np.array_equal(out["ids_restore"].numpy(), fx[f"{geom}/ids_restore"])
    out["recon_loss"].backward()
    sub = {k[len(geom) + 1:]: v for k, v in fx.items() if k.startswith(geom + "/")}
    for name, p in P.items():
        if not mr.trainable(name):
            assert p.grad is None or not p.grad.any()
            continue
        assert cpu_ref.summary_rel_error(name, p.grad.numpy(), sub) <= 1e-4, name
        assert float(sub["hf32_err/" + name][0]) <= 1e-4          # HF float32 against HF float64
    z0 = mr.forward(x, None, mr.to_torch(mr.make_params(geom), requires_grad=False), geom, mask_ratio=0.0)["z"]
    ref0 = fx[f"{geom}/z_mask0"].astype(np.float64)
    assert np.abs(z0.numpy() - ref0).max() <= 1e-5 * np.abs(ref0).max()


def test_mae_entries_reject_bad_arguments_without_launching(lib):
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    assert lib.vs_mae_embed_fwd(2, 9, 2, 64, None, p, p, p, p, None) == -1
    assert b"null pointer" in lib.vs_last_error()
    assert lib.vs_mae_embed_fwd(2, 9, 10, 64, p, p, p, p, p, None) == -1
    assert b"1..P" in lib.vs_last_error()
    assert lib.vs_mae_embed_bwd(2, 2, 9, 2, 64, p, p, p, p, None) == -1           # VS_U8
    assert b"dtype" in lib.vs_last_error()
    assert lib.vs_mae_dec_assemble_fwd(2, 9, 2, 66, p, p, p, p, p, None) == -1
    assert b"multiple of 4" in lib.vs_last_error()
    assert lib.vs_mae_dec_assemble_bwd(0, 2, 9, 2, 64, p, p, p, p, p, None, None) == -1
    assert b"null pointer" in lib.vs_last_error()
    assert lib.vs_mae_recon_loss(0, 2, 1, 48, 16, 9, p, 256, p, p, p, p, 256, p, None) == -1
    assert b"at least one masked" in lib.vs_last_error()
    assert lib.vs_mae_recon_loss(0, 2, 1, 50, 16, 2, p, 256, p, p, p, p, 256, p, None) == -1
    assert b"multiple of the patch" in lib.vs_last_error()
    assert lib.vs_mae_dec_assemble_bwd_workspace_bytes(128, 512) == 128 * 512 * 4
    assert lib.vs_mae_recon_loss_workspace_bytes(128, 81) == 128 * 81 * 8


# ------------------------------------------------------------------------------------------------------------
# the plugin's host side
# ------------------------------------------------------------------------------------------------------------
CFG = os.path.join(ROOT, "video-spike_amd", "config")


def test_builds_from_the_yaml_through_the_registry():
    from vspike import MAE, NAME2MODEL
    from vspike.config import load_run_config
    cfg = load_run_config(os.path.join(CFG, "model", "mae.yaml"), os.path.join(CFG, "train", "vmae_video.yaml"))
    assert cfg.model.model_class == "MAE"
    m = NAME2MODEL[cfg.model.model_class](cfg.model)
    assert isinstance(m, MAE)
    assert (m.num_patches, m.hidden_size, m.decoder_hidden_size, m.patch_dim) == (81, 768, 512, 256)
    assert (m.enc_stack.layers, m.enc_stack.head_dim, m.dec_stack.layers, m.dec_stack.head_dim) == (12, 64, 8, 32)
    assert m.config.mask_ratio == 0.75 and m.compute_dtype == torch.bfloat16
    with pytest.raises(Exception):
        m(torch.zeros(1, 1, 144, 144))          # CPU tensor: no fallback path
    with pytest.raises(ValueError):
        m.set_side_stream(True)
    with pytest.raises(NotImplementedError):
        m.grad_sink = object()


@pytest.mark.parametrize("geom", list(mr.GEOMETRIES))
def test_state_dict_round_trip_in_both_spellings(geom):
    from vspike import MAE
    params = {k: torch.from_numpy(v) for k, v in mr.make_params(geom).items()}
    m = MAE(mr.model_config(geom))
    m.load_reference_state_dict(params)
    for modern in (False, True):
        back = m.reference_state_dict(modern_names=modern)
        if modern:
            assert any(".attention.q_proj." in k for k in back) and any(".vit.layers." in k for k in back)
            assert any("decoder_layers.0.mlp.fc1." in k for k in back)
        m2 = MAE(mr.model_config(geom))
        m2.load_reference_state_dict(back)
        assert torch.equal(m.enc_flat, m2.enc_flat) and torch.equal(m.dec_flat, m2.dec_flat)
    back = m.reference_state_dict()
    for k, v in params.items():
        if k.endswith("key.bias"):
            assert not back[k].any()            # accepted on load, exported as zeros
        else:
            assert torch.equal(back[k], v), k
    assert set(back) - set(params) == {"vit_mae.vit.embeddings.position_embeddings", "vit_mae.decoder.decoder_pos_embed"}
    for s in list(m.layout.enc.slots.values()) + list(m.layout.dec.slots.values()):
        assert s.offset % 64 == 0
    with pytest.raises(KeyError):
        m.load_reference_state_dict({k: v for k, v in params.items() if "mask_token" not in k})
    bad = dict(back)
    bad["vit_mae.decoder.decoder_pos_embed"] = back["vit_mae.decoder.decoder_pos_embed"] + 1e-3
    with pytest.raises(ValueError):
        m.load_reference_state_dict(bad)


@pytest.mark.parametrize("override", [{"decoder_num_attention_heads": 1}, {"norm_pix_loss": True},
                                      {"hidden_dropout_prob": 0.1}, {"attention_probs_dropout_prob": 0.1},
                                      {"compute_dtype": "fp8"}, {"num_attention_heads": 4}])
def test_unsupported_configs_raise(override):
    from vspike import MAE
    conf = mr.model_config("g1")
    conf.update(override)
    with pytest.raises(ValueError):
        MAE(conf)


def test_bf16_rounding_model_moves_the_restatement_a_little():
    """mae_ref.forward(bf16=True), the yardstick of the GPU bf16 test: within a few bf16 steps of the float path."""
    geom = "g1"
    P = mr.to_torch(mr.make_params(geom), torch.float32, requires_grad=False)
    x, noise = torch.from_numpy(mr.make_images(geom)), torch.from_numpy(mr.make_noise(geom))
    a, b = mr.forward(x, noise, P, geom), mr.forward(x, noise, P, geom, bf16=True)
    d = abs(a["recon_loss"].item() - b["recon_loss"].item()) / a["recon_loss"].item()
    assert 0 < d < 5e-2
