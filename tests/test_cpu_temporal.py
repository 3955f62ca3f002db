"""CPU-only tests of the VideoMAETemporal plugin's host logic (construction from the YAML, flat layout,
reference-style names) and of the token-pool entry points' argument checks.  No kernel is launched."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "video-spike_amd", "config")

SMALL = {"model_class": "VideoMAETemporal", "freeze_encoder": False,
         "backbone": {"image_size": 112, "num_frames": 8, "hidden_size": 128, "num_hidden_layers": 2,
                      "num_attention_heads": 2, "intermediate_size": 512},
         "temporal": {"num_layers": 2, "intermediate_size": 256},
         "encoder": {"output_dim": 64}, "decoder": {"output_dim": 1600}}


@pytest.fixture(scope="module")
def built_lib():
    from vspike import build
    build.build(verbose=False)
    return build.LIB_PATH


def test_builds_from_the_yaml_on_cpu():
    from vspike import NAME2MODEL, VideoMAETemporal
    from vspike.config import load_run_config
    cfg = load_run_config(os.path.join(CFG, "model", "vmae_temporal.yaml"), os.path.join(CFG, "train", "vmae_video.yaml"))
    assert cfg.model.model_class == "VideoMAETemporal"
    m = NAME2MODEL[cfg.model.model_class](cfg.model)
    assert isinstance(m, VideoMAETemporal)
    lay = m.layout
    # C5 geometry: 32 frames -> 16 time steps of 196 tokens, Base width, two temporal blocks, fp8 encoder
    assert (lay.time_steps, m.backbone.num_tokens, m.backbone.hidden_size) == (16, 3136, 768)
    assert lay.temporal_layers == 2 and lay.temporal_mlp == 3072 and m.fp8
    assert lay.head.slots["enc_w"].shape == (64, 16 * 768)
    assert m.temp_flat.numel() == lay.temp.numel and m.temp_flat.requires_grad
    assert not m.enc_flat.requires_grad            # freeze_encoder freezes the encoder buffer only
    assert [n for n, _ in m.named_parameters()] == ["enc_flat", "head_flat", "temp_flat"]
    with pytest.raises(Exception):
        m(torch.zeros(1, 32, 3, 224, 224))         # CPU tensor: no fallback path


def test_temporal_mlp_defaults_to_the_backbone_and_zero_layers_is_valid():
    from vspike import VideoMAETemporal
    conf = dict(SMALL, temporal={"num_layers": 1})
    assert VideoMAETemporal(conf).layout.temporal_mlp == 512
    m0 = VideoMAETemporal({k: v for k, v in SMALL.items() if k != "temporal"})
    assert m0.layout.temporal_layers == 0 and m0.temp_flat.numel() == 0
    assert m0.layout.head.slots["enc_w"].shape == (64, 4 * 128)


def test_temporal_layout_slots_aligned_and_disjoint():
    from vspike import VideoMAETemporal
    from vspike.layout import LAYER_KEYS
    lay = VideoMAETemporal(SMALL).layout
    slots = sorted(lay.temp.slots.values(), key=lambda s: s.offset)
    assert [s.name for s in slots] == [f"{j}.{k}" for j in range(2) for k in LAYER_KEYS]
    end = 0
    for s in slots:
        assert s.offset % 64 == 0 and s.offset >= end, s
        end = s.offset + s.numel
    assert end <= lay.temp.numel
    assert lay.temp_ranges == [(0, lay.temp.numel // 2), (lay.temp.numel // 2, lay.temp.numel)]
    assert lay.temp.slots["0.w_fc1"].shape == (256, 128) and lay.temp.slots["1.w_fc2"].shape == (128, 256)
    # the encoder flat is the VideoMAE plugin's, slot for slot
    from vspike import VideoMAE
    ref = VideoMAE({k: v for k, v in SMALL.items() if k != "temporal"}).layout
    assert {k: (s.shape, s.offset) for k, s in lay.enc.slots.items()} == \
        {k: (s.shape, s.offset) for k, s in ref.enc.slots.items()}


def test_state_dict_names_unique_and_round_trip():
    from temporal_ref import temporal_param_shapes
    from oracle import cpu_ref
    from vspike import VideoMAETemporal
    from vspike.layout import modern_name
    m = VideoMAETemporal(SMALL)
    names = [n for n, *_ in m.layout.hf_items()]
    assert len(names) == len(set(names))
    assert "temporal.layer.1.attention.attention.q_bias" in names and "encoder.weight" in names
    want = temporal_param_shapes(cpu_ref.VIT_SMALL_FIXTURE, 2, 256, 64, 16)
    assert sorted(modern_name(n) for n in names) == sorted(want)
    for modern in (False, True):                    # both Q/V-bias spellings
        sd = m.reference_state_dict(modern_names=modern)
        assert {k: tuple(v.shape) for k, v in sd.items()} == \
            {(k if modern else n): want[k] for n in names for k in [modern_name(n)]}
        m2 = VideoMAETemporal(SMALL)
        assert not torch.equal(m2.temp_flat, m.temp_flat)
        m2.load_reference_state_dict(sd, strict=True)
        for a, b in ((m.enc_flat, m2.enc_flat), (m.temp_flat, m2.temp_flat), (m.head_flat, m2.head_flat)):
            assert torch.equal(a, b)
    with pytest.raises(KeyError):
        m2.load_reference_state_dict({k: v for k, v in sd.items() if "temporal.layer.0.output" not in k}, strict=True)


def test_pool_entry_points_reject_bad_args_without_launching(built_lib):
    from vspike import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 256)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    fwd = lambda G, S, D, x, ldx, out: lib.vs_token_pool_fwd(G, S, D, x, ldx, None, 0, out, None, None)  # noqa: E731
    bwd = lambda G, S, D, dp, dx: lib.vs_token_pool_bwd(G, S, D, dp, dx, None, None)  # noqa: E731
    assert fwd(1, 1, 96, p, 96, p) == -1 and b"multiple of 64" in lib.vs_last_error()
    assert bwd(1, 1, 96, p, p) == -1 and b"multiple of 64" in lib.vs_last_error()
    assert fwd(1, 1, 64, None, 64, p) == -1 and b"null pointer" in lib.vs_last_error()
    assert fwd(1, 1, 64, p, 64, None) == -1 and b"null pointer" in lib.vs_last_error()
    assert bwd(1, 1, 64, None, p) == -1 and b"null pointer" in lib.vs_last_error()
    assert bwd(1, 1, 64, p, None) == -1 and b"null pointer" in lib.vs_last_error()
    for S in (0, -3):
        assert fwd(1, S, 64, p, 64, p) == -1 and b"positive" in lib.vs_last_error()
        assert bwd(1, S, 64, p, p) == -1 and b"positive" in lib.vs_last_error()
    assert fwd(1, 1, 128, p, 64, p) == -1 and b"ldx" in lib.vs_last_error()
    assert fwd(1, 1, 64, p, 66, p) == -1 and b"ldx" in lib.vs_last_error()
    assert fwd(1, 1, 64, p + 4, 64, p) == -1 and b"aligned" in lib.vs_last_error()
    # a position table without rows
    assert lib.vs_token_pool_fwd(1, 1, 64, p, 64, p, 0, p, None, None) == -1 and b"pos_rows" in lib.vs_last_error()


def test_token_pool_dispatch_counter_is_declared(built_lib):
    from vspike import _lib
    assert "token_pool" in _lib.PATH_NAMES
    assert _lib.PATH_NAMES.index("token_pool") == 26 and _lib.PATH_COUNT == 27
    _lib.dispatch_reset()
    assert _lib.dispatch_counts()["token_pool"] == 0


def test_exchange_treats_the_temporal_buffer_as_sunk():
    from vspike import VideoMAETemporal
    from vspike.dp import GradExchange
    m = VideoMAETemporal(SMALL)
    ex = GradExchange(m)
    assert ex._sunk == {id(m.enc_flat), id(m.temp_flat), id(m.head_flat)}
    assert m.grad_sink is ex
