"""The contrastive loader on the GPU: vs_contrast_frames (csrc/contrast_loader.hip), vspike.data.ContrastFrames on the
device, ContrastTrainer.step_fused and ContrastTrainer.fit.

Frame bars.  The yardstick is tests/contrast_loader_ref.py, the float64 restatement of torchvision's Resize +
Normalize.  The bar of every case is d_ref, the fixture's figure for how far the reference's own float32 frames lie
from that restatement on the very same frames (margin 1x): the kernel computes its weights and sums in float64 and
must land inside the reference's error.  Identity (H = W = S) and the one-pixel frame must be torch's bits.
"""
import os

import numpy as np
import pytest
import torch

import contrast_loader_ref as cl

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 4096           # bytes of guard on each side of an operand


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("contrast_loader.npz")


def _session(fx, name):
    return {f"{k}_{part}": fx[f"{name}/{k}_{part}"] for k in ("train", "val", "test") for part in ("X", "y", "timestamp")}


def _sorted_frames(fx, name):
    if name == "W":
        return fx["W/video"][fx["W/sort"]]
    data = _session(fx, name)
    video = np.concatenate([data[f"{s}_X"] for s in ("train", "val", "test")])
    return video.reshape((-1,) + video.shape[2:])[fx[f"{name}/sort"]]


def _cases(fx):
    """name -> (frames uint8 (n, 1, H, W), S, d_ref): the fixture's sessions, the workload pair, the small geometries."""
    out = {name: (_sorted_frames(fx, name), 144 if name == "W" else 24, float(fx[f"{name}/d_ref"]))
           for name in ("A", "B", "W")}
    for (H, W, S) in cl.EXTRA_GEOMETRIES:
        out[f"{H}x{W}_{S}"] = (cl.extra_frames(H, W, S), S, float(fx[f"extra/{H}x{W}_{S}/d_ref"]))
    return out


CASES = ["A", "B", "W"] + [f"{H}x{W}_{S}" for (H, W, S) in cl.EXTRA_GEOMETRIES]


def _run(frames, S, idx=None, **kw):
    from vspike import ops
    v = torch.as_tensor(frames).to(DEV)
    i = torch.arange(v.shape[0], device=DEV) if idx is None else torch.as_tensor(idx, dtype=torch.int64).to(DEV)
    return ops.contrast_frames(v, i, size=S, **kw)


@pytest.mark.parametrize("case", CASES)
def test_frames_within_the_references_own_error(fixture, case):
    """Largest distance to the float64 restatement <= d_ref (1x).  Measured on MI355X, kernel / d_ref:
    A 4.4e-2, B 3.5e-2, W 8.0e-3, 7x192_24 3.9e-1, 1x1_24 both 0 (torch's bits), 145x143_144 4.9e-3: the kernel sits
    1.1e-7 .. 1.2e-7 from the restatement everywhere, two float32 roundings of values in (-1, 1)."""
    frames, S, d_ref = _cases(fixture)[case]
    got = _run(frames, S).cpu().numpy().astype(np.float64)
    want = cl.transform(frames, S)
    d = float(np.abs(got - want).max())
    print(f"\ncontrast_frames {case}: distance to the restatement {d:.3e}, d_ref {d_ref:.3e}, "
          f"ratio {d / d_ref if d_ref else float('nan'):.3g}")
    assert got.shape == want.shape and np.isfinite(got).all()
    assert d <= d_ref


def test_one_pixel_and_identity_are_torchs_bits():
    """H = W = S: (float32(p) / 255 - 0.5) / 0.5 bit for bit, for every pixel value, with 16-byte stores (S = 16), scalar
    stores (S = 18) and a std that is no power of two (the division path).  A 1 x 1 frame is that value everywhere."""
    from vspike import ops
    for S in (16, 18):
        p = (np.arange(3 * S * S) % 256).astype(np.uint8).reshape(3, 1, S, S)
        assert len(np.unique(p)) == 256
        got = _run(p, S).cpu().numpy()
        assert np.array_equal(got.view(np.int32), cl.identity_expected(p).view(np.int32))
        got = _run(p, S, mean=0.45, std=0.225).cpu().numpy()
        assert np.array_equal(got.view(np.int32), cl.identity_expected(p, 0.45, 0.225).view(np.int32))
    one = np.arange(256, dtype=np.uint8).reshape(256, 1, 1, 1)
    got = _run(one, 24).cpu().numpy()
    want = np.broadcast_to(cl.identity_expected(one), (256, 1, 24, 24))
    assert np.array_equal(got.view(np.int32), np.ascontiguousarray(want).view(np.int32))
    assert ops.contrast_frames_plan(16, 16, 16)["taps_w"] == 2


@pytest.mark.parametrize("case", ["B", "7x192_24", "W"])
def test_float_input_equals_uint8_input(fixture, case):
    frames, S, _ = _cases(fixture)[case]
    a = _run(frames[:3], S)
    b = _run(frames[:3].astype(np.float32), S)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _guarded(t, fill):
    """A copy of t inside a larger allocation whose margins hold `fill`: (buffer, view)."""
    t = t.contiguous()
    pad = MARGIN // t.element_size()
    buf = torch.full((t.numel() + 2 * pad,), fill, dtype=t.dtype, device=DEV)
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


@pytest.mark.parametrize("case,G", [("A", 1), ("B", 3), ("A", 385), ("7x192_24", 3), ("W", 3)])
def test_repeatable_and_writes_nothing_outside_out(fixture, case, G):
    """G = 1, 3, 385 indices with repeats, the first and the last frame among them: equal to the plain run on those
    frames, the same bits twice, and with video, idx and out inside guarded allocations (255 / an index far out of
    range / NaN around them) the margins are untouched and the result is the plain run's."""
    from vspike import ops
    frames, S, _ = _cases(fixture)[case]
    F = frames.shape[0]
    rs = np.random.RandomState(G)
    idx = rs.randint(0, F, size=G)
    idx[0] = F - 1
    if G > 2:
        idx[1], idx[2] = 0, F - 1
    plain = _run(frames, S, idx)
    every = _run(frames, S)
    assert torch.equal(plain.view(torch.int32), every[torch.as_tensor(idx).to(DEV)].view(torch.int32))
    vb, v = _guarded(torch.as_tensor(frames).to(DEV), 255)
    ib, i = _guarded(torch.as_tensor(idx, dtype=torch.int64).to(DEV), 1 << 40)
    ob, o = _guarded(torch.full((G, 1, S, S), float("nan"), device=DEV), float("nan"))
    for _ in range(2):
        o.fill_(float("nan"))
        ops.contrast_frames(v, i, size=S, out=o)
        assert torch.equal(o.view(torch.int32), plain.view(torch.int32))
    pad = MARGIN // 4
    assert bool(torch.isnan(ob[:pad]).all() and torch.isnan(ob[pad + o.numel():]).all())
    assert bool((vb[:MARGIN] == 255).all() and (vb[MARGIN + v.numel():] == 255).all())
    assert torch.equal(v.cpu(), torch.as_tensor(frames)) and torch.equal(i.cpu(), torch.as_tensor(idx, dtype=torch.int64))
    assert bool((ib[:MARGIN // 8] == 1 << 40).all() and (ib[MARGIN // 8 + G:] == 1 << 40).all())


def test_unsupported_extents_and_bad_indices_are_refused():
    """Outside 1 <= S <= 512, 1 <= H, W <= 8 S the call is an error and `out` stays untouched; a negative index or
    one >= F is refused on the host before any launch."""
    from vspike import ops
    from vspike._lib import VsError
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    for (H, W, S) in ((8, 8, 0), (8, 8, 513), (65, 8, 8), (8, 65, 8), (4097, 8, 512)):
        v = torch.zeros(2, 1, H, W, dtype=torch.uint8, device=DEV)
        out = torch.full((2, 1, max(S, 1), max(S, 1)), 7.0, device=DEV)
        with pytest.raises(VsError):
            ops.contrast_frames(v, idx, size=S, out=out if S >= 1 else None)
        assert bool((out == 7.0).all())
    v = torch.zeros(4, 1, 8, 8, dtype=torch.uint8, device=DEV)
    out = torch.full((2, 1, 8, 8), 7.0, device=DEV)
    for bad in ([0, 4], [-1, 0]):
        with pytest.raises(VsError, match="index outside"):
            ops.contrast_frames(v, torch.tensor(bad, device=DEV), size=8, out=out)
        assert bool((out == 7.0).all())
    for badv in (v[:, :, ::2], v.to(torch.float64), v[:, 0]):
        with pytest.raises(VsError):
            ops.contrast_frames(badv, idx, size=8)
    with pytest.raises(VsError):
        ops.contrast_frames(v, idx.to(torch.int32), size=8)
    with pytest.raises(VsError, match="std"):
        ops.contrast_frames(v, idx, size=8, std=0.0)


# ---- ContrastFrames on the device -------------------------------------------------------------------------------
def _loader(fx, name, mode="pretrain", **kw):
    from vspike.data import ContrastFrames
    how = cl.EPOCHS[name][0]
    args = dict(mode=mode, batch_size=cl.BATCH, shuffle=True, size=cl.SESSIONS[name]["S"], idx_offset=cl.IDX_OFFSET,
                time_offset=cl.TIME_OFFSET if how == "time" else None, device=DEV)
    args.update(kw)
    return ContrastFrames(_session(fx, name), **args)


@pytest.mark.parametrize("name", sorted(cl.SESSIONS))
def test_loader_yields_the_fixtures_epochs(fixture, name):
    """Every recorded epoch on the device: ref, pos and neg are the restatement's frames at the fixture's triplets
    within d_ref (and so the reference's, whose frames lie within d_ref of the same), three views of one 3b buffer;
    numpy's generator stands where the reference's did."""
    ld = _loader(fixture, name)
    assert ld.video.dtype == torch.uint8 and ld.video.is_cuda
    seed = cl.EPOCHS[name][2]
    torch.manual_seed(seed)
    np.random.seed(seed)
    want = cl.transform(_sorted_frames(fixture, name), 24)
    d_ref, worst = float(fixture[f"{name}/d_ref"]), 0.0
    for e, tri in enumerate(fixture[f"{name}/triplets"]):
        at = 0
        for batch in ld:
            b = batch["ref"].shape[0]
            x = ld.fused(batch)
            assert x.shape == (3 * b, 1, 24, 24) and x.dtype == torch.float32 and x.is_contiguous()
            for k, view in enumerate(("ref", "pos", "neg")):
                assert batch[view].data_ptr() == x[k * b:].data_ptr() and batch[view].shape == (b, 1, 24, 24)
                d = np.abs(batch[view].cpu().numpy() - want[tri[at:at + b, k]]).max()
                worst = max(worst, float(d))
            at += b
        assert at == 48 and cl.peek_numpy() == fixture[f"{name}/next_draw"][e]
    print(f"\nContrastFrames {name}: distance to the restatement {worst:.3e}, d_ref {d_ref:.3e}")
    assert worst <= d_ref


def test_loader_trial_modes_and_raw_frames(fixture):
    data = _session(fixture, "A")
    got = list(_loader(fixture, "A", mode="train", batch_size=1, shuffle=False))
    assert len(got) == 4
    d_ref = float(fixture["A/d_ref"])
    for i, b in enumerate(got):
        assert b["ref"].shape == (1, 6, 1, 24, 24) and b["ref"].dtype == torch.float32 and b["ref"].is_cuda
        assert b["neural"].shape == (1, 5, 7) and np.array_equal(b["neural"][0].cpu().numpy(), data["train_y"][i])
        assert np.abs(b["ref"][0].cpu().numpy() - cl.transform(data["train_X"][i], 24)).max() <= d_ref
    raw = next(iter(_loader(fixture, "A", mode="val", batch_size=1, shuffle=False, transform=None)))
    assert raw["ref"].dtype == torch.uint8 and np.array_equal(raw["ref"][0].cpu().numpy(), data["val_X"][0])


# ---- the fused step and fit -------------------------------------------------------------------------------------
FIT = dict(H=20, W=28, S=32, splits=(4, 2, 2), t=8, T=5, N=9, E=3, batch=32)


def _fit_model(dtype="fp32"):
    """The smallest ContrastViT of the existing contrast tests (test_gpu_rrr.py's validation model)."""
    from vspike import ContrastViT
    torch.manual_seed(5)
    cfg = {"model_class": "ContrastViT", "compute_dtype": dtype, "fix_temp": True, "image_size": FIT["S"],
           "patch_size": 16, "num_channels": 1, "hidden_size": 64, "num_hidden_layers": 1, "num_attention_heads": 1,
           "intermediate_size": 128, "layer_norm_eps": 1e-12, "embed_size": FIT["E"], "mask_ratio": 0.75,
           "decoder_hidden_size": 512}
    return ContrastViT(cfg).to(DEV)


def _fit_session():
    """64 frames: 4 / 2 / 2 trials of 8 frames, spikes that follow the frames' brightness."""
    rs = np.random.RandomState(77)
    n, t = sum(FIT["splits"]), FIT["t"]
    level = rs.uniform(40, 215, size=(n, t, 1, 1, 1))
    video = np.clip(level + rs.normal(0, 25, size=(n, t, 1, FIT["H"], FIT["W"])), 0, 255).astype(np.uint8)
    rate = 0.3 + 2.0 * (level[:, :FIT["T"], 0, 0, 0] / 255.0)[..., None] * rs.uniform(0.2, 1.0, size=(1, 1, FIT["N"]))
    spikes = rs.poisson(rate).astype(np.float32)
    times = (np.arange(n * t) / 60.0).reshape(n, t)
    out, lo = {}, 0
    for split, k in zip(("train", "val", "test"), FIT["splits"]):
        out[f"{split}_X"], out[f"{split}_y"], out[f"{split}_timestamp"] = video[lo:lo + k], spikes[lo:lo + k], times[lo:lo + k]
        lo += k
    return out


def _fit_run(path):
    from vspike import FusedAdamW
    from vspike.data import make_contrast_loader
    from vspike.trainer import ContrastTrainer
    data = _fit_session()
    m = _fit_model()
    torch.manual_seed(21)
    np.random.seed(21)
    pre, _ = make_contrast_loader(data, "pretrain", FIT["batch"], True, size=FIT["S"], idx_offset=3, device=DEV)
    train, _ = make_contrast_loader(data, "train", 1, False, size=FIT["S"], device=DEV)
    val, _ = make_contrast_loader(data, "val", 1, False, size=FIT["S"], device=DEV)
    tr = ContrastTrainer(m, FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2))
    calls = {"validate": 0, "weights": []}
    validate = tr.validate

    def counted(*a, **k):
        calls["validate"] += 1
        calls["weights"].append(m.enc_flat.detach().clone())
        return validate(*a, **k)
    tr.validate = counted
    res = tr.fit(pre, train, val, max_steps=5, path=path)
    return m, tr, res, calls


def test_fit_steps_validates_and_keeps_the_best(tmp_path):
    """max_steps = 5 over 2 batches per pass: 5 steps, 3 validations (the pass cut short included), the file holds the
    best pass's weights and loads through load_best; a second run from the same seeds gives the same bits."""
    path = str(tmp_path / "best_model.pth")
    m, tr, res, calls = _fit_run(path)
    assert len(res["steps"]) == 5 and calls["validate"] == 3 and len(res["val_bps"]) == 3
    assert all(isinstance(s["loss"], torch.Tensor) and s["loss"].is_cuda for s in res["steps"])
    assert m.training
    vals = np.array(res["val_bps"])
    assert np.isfinite(vals).all() and res["best_val_bps"] == vals.max() and res["best_pass"] == int(vals.argmax())
    assert os.path.exists(path)
    saved = torch.load(path)
    fresh = _fit_model()
    fresh.load_reference_state_dict(saved)
    assert torch.equal(fresh.enc_flat.detach(), calls["weights"][res["best_pass"]])
    assert tr.load_best(path) and torch.equal(m.enc_flat.detach(), calls["weights"][res["best_pass"]])
    assert not tr.load_best(str(tmp_path / "missing.pth"))
    _, _, again, _ = _fit_run(str(tmp_path / "again.pth"))
    for a, b in zip(res["steps"], again["steps"]):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert again["val_bps"] == res["val_bps"]
    losses = [float(s["loss"]) for s in res["steps"]]
    print(f"\nfit: losses {losses}, val_bps {res['val_bps']}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fused_step_equals_the_three_tensor_step(dtype):
    """step_fused on the loader's 3b buffer = step(ref, pos, neg) on its views, bit for bit: losses and weights."""
    from vspike import FusedAdamW
    from vspike.data import make_contrast_loader
    from vspike.trainer import ContrastTrainer
    data = _fit_session()
    torch.manual_seed(3)
    np.random.seed(3)
    pre, _ = make_contrast_loader(data, "pretrain", 24, True, size=FIT["S"], idx_offset=3, device=DEV)
    batch = next(iter(pre))
    out = []
    for fused in (True, False):
        m = _fit_model(dtype)
        tr = ContrastTrainer(m, FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2))
        for _ in range(2):
            res = tr.step_fused(pre.fused(batch), 24) if fused else tr.step(batch["ref"], batch["pos"], batch["neg"])
        out.append((res, m.enc_flat.detach().clone(), m.head_flat.detach().clone()))
    (ra, ea, ha), (rb, eb, hb) = out
    assert set(ra) == set(rb)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    assert torch.equal(ea, eb) and torch.equal(ha, hb)
    with pytest.raises(ValueError):
        tr.step_fused(pre.fused(batch), 36)
