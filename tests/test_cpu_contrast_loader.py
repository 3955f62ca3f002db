"""The contrastive loader's sampling on the CPU (vspike.data.ContrastFrames), against tests/golden/contrast_loader.npz:
what the reference's ContrastDataset gave under a real torch DataLoader (scripts/gen_contrast_loader_fixture.py).

No GPU: the loader's frame transform is replaced, through its `frame_fn` seam, by the float64 restatement
tests/contrast_loader_ref.py; the video sits on the CPU.  Index triplets and the state of numpy's generator must be
the fixture's exactly.  Frames are compared within d_ref, the fixture's own figure for how far the reference's float32
frames lie from the restatement (2.6e-6 .. 2.3e-5 on these sessions).
"""
import numpy as np
import pytest
import torch

import contrast_loader_ref as cl


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("contrast_loader.npz")


def _session(fx, name):
    return {f"{k}_{part}": fx[f"{name}/{k}_{part}"] for k in ("train", "val", "test") for part in ("X", "y", "timestamp")}


def _restated(video, idx, size, mean, std):
    return torch.from_numpy(cl.transform(video[idx].numpy(), size, mean, std))


def _loader(fx, name, mode="pretrain", **kw):
    from vspike.data import ContrastFrames
    how = cl.EPOCHS[name][0]
    args = dict(mode=mode, batch_size=cl.BATCH, shuffle=True, size=cl.SESSIONS[name]["S"], idx_offset=cl.IDX_OFFSET,
                time_offset=cl.TIME_OFFSET if how == "time" else None, device="cpu", frame_fn=_restated)
    args.update(kw)
    return ContrastFrames(_session(fx, name), **args)


def _seed(name):
    seed = cl.EPOCHS[name][2]
    torch.manual_seed(seed)
    np.random.seed(seed)


def test_the_fixture_is_the_committed_generators_inputs(fixture):
    """The sessions in the fixture are contrast_loader_ref.make_session's, so the generator script and the tests
    speak about the same data."""
    for name in cl.SESSIONS:
        for k, v in cl.make_session(name).items():
            assert np.array_equal(fixture[f"{name}/{k}"], v), (name, k)
        assert fixture[f"{name}/triplets"].shape == (cl.EPOCHS[name][1], 48, 3)


@pytest.mark.parametrize("name", sorted(cl.SESSIONS))
def test_triplets_and_generator_state_are_the_references(fixture, name):
    """Every recorded epoch: the items in the loader's order, each item's positive and negative, and numpy's next
    draw after the epoch.  Session A is the idx_offset mode (two epochs), B the time_offset mode, whose positives
    follow the real timestamps (the reference's quirk: ContrastFrames' docstring)."""
    ld = _loader(fixture, name)
    assert np.array_equal(ld.sort, fixture[f"{name}/sort"])
    _seed(name)
    want = fixture[f"{name}/triplets"]
    for e in range(want.shape[0]):
        got = np.concatenate([ld.draw([int(i) for i in items]) for items in ld._batches()])
        assert np.array_equal(got, want[e]), f"epoch {e}"
        assert cl.peek_numpy() == fixture[f"{name}/next_draw"][e], f"numpy's generator after epoch {e}"
    if cl.EPOCHS[name][0] == "time":        # a linspace timestamp would leave every positive on its own frame
        assert (want[..., 1] != want[..., 0]).any()


@pytest.mark.parametrize("name", sorted(cl.SESSIONS))
def test_batches_are_the_references_frames(fixture, name):
    """The iterator end to end on the CPU: batch sizes 5 .. 5, 3, the three views of one buffer, and the frames the
    reference's loader gave (its per-frame transform at the triplets), within d_ref of the restatement's."""
    ld = _loader(fixture, name)
    _seed(name)
    ref_frames, d_ref = fixture[f"{name}/ref_frames"], float(fixture[f"{name}/d_ref"])
    tri = fixture[f"{name}/triplets"][0]
    at, worst = 0, 0.0
    sizes = []
    for batch in ld:
        b = batch["ref"].shape[0]
        sizes.append(b)
        assert set(batch) == {"ref", "pos", "neg"} and ld.fused(batch).shape == (3 * b, 1, 24, 24)
        for k, view in enumerate(("ref", "pos", "neg")):
            assert batch[view].data_ptr() == ld.fused(batch)[k * b:].data_ptr()
            d = np.abs(batch[view].numpy() - ref_frames[tri[at:at + b, k]].astype(np.float64)).max()
            worst = max(worst, float(d))
        at += b
    assert sizes == [5] * 9 + [3] and len(ld) == 10
    print(f"\n{name}: restatement to the reference's frames {worst:.3e}, d_ref {d_ref:.3e}")
    assert worst <= d_ref


def test_restatement_reproduces_the_fixture(fixture):
    """tests/contrast_loader_ref.transform against the frames stored when the fixture was made: bitwise its own
    stored result, and within d_ref of the reference's float32 frames, for both sessions and the workload's
    110 x 166 -> 144.  The extra geometries' d_ref are of the size the fixture was made with."""
    for name in ("A", "B", "W"):
        if name == "W":
            frames = fixture["W/video"][fixture["W/sort"]]
            S = 144
        else:
            data = _session(fixture, name)
            video = np.concatenate([data[f"{s}_X"] for s in ("train", "val", "test")]).reshape(48, 1, *data["train_X"].shape[-2:])
            frames, S = video[fixture[f"{name}/sort"]], 24
        got = cl.transform(frames, S)
        keep = fixture[f"{name}/restatement"].shape[0]
        assert np.array_equal(got[:keep], fixture[f"{name}/restatement"])
        d = float(np.abs(got - fixture[f"{name}/ref_frames"].astype(np.float64)).max())
        assert d == float(fixture[f"{name}/d_ref"]) and 0 < d < 5e-5, (name, d)
    for (H, W, S) in cl.EXTRA_GEOMETRIES:
        assert 0.0 <= float(fixture[f"extra/{H}x{W}_{S}/d_ref"]) < 5e-5


def test_restatement_windows_and_identity():
    """The weights' windows at the edges of the supported range: 16 taps at the 8x limit (the kernel's bound of 17 is
    never reached: a window of width 2 support <= 16 covers at most 16 pixel centres), two taps at in == out with
    weights (1, 0), rows that sum to one; and the identity's float32 formula."""
    xmin, xsize = cl.axis_windows(192, 24)
    assert xsize.max() == 16 and xmin.min() == 0 and (xmin + xsize).max() == 192
    assert max(cl.axis_windows(n, 24)[1].max() for n in range(170, 193)) == 16
    M = cl.axis_matrix(24, 24)
    assert np.array_equal(M, np.eye(24)) and cl.axis_windows(24, 24)[1].max() == 2
    for n_in, n_out in ((7, 24), (192, 24), (145, 144), (143, 144), (1, 24), (166, 144), (110, 144)):
        assert np.abs(cl.axis_matrix(n_in, n_out).sum(1) - 1.0).max() < 1e-15
    p = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16)
    want = cl.identity_expected(p)
    assert want.dtype == np.float32 and np.abs(cl.transform(p, 16) - want).max() < 1e-7
    t = torch.tensor(p, dtype=torch.float32).div_(255.0)
    assert np.array_equal(((t - 0.5) / 0.5).numpy(), want)


def test_kernel_plan_uses_the_restatements_windows():
    """vs_contrast_frames_plan (host code of csrc/contrast_loader.hip, no GPU needed): the tap counts it plans with
    are the restatement's largest windows, every band's source rows fit what it stages, and the supported range's
    corners stay within the LDS budget."""
    from vspike import ops
    from vspike._lib import VsError
    for (H, W, S) in cl.EXTRA_GEOMETRIES + [(20, 28, 24), (40, 19, 24), (110, 166, 144), (24, 24, 24), (4096, 4096, 512),
                                            (1, 4096, 512), (512, 1, 512), (3, 5, 1)]:
        p = ops.contrast_frames_plan(H, W, S)
        assert p["taps_w"] == cl.axis_windows(W, S)[1].max() and p["taps_h"] == cl.axis_windows(H, S)[1].max()
        assert p["taps_w"] <= 17 and p["taps_h"] <= 17 and p["lds_bytes"] <= 64 * 1024
        assert p["bands"] == -(-S // p["rows"])
        ymin, ysize = cl.axis_windows(H, S)
        for y0 in range(0, S, p["rows"]):
            y1 = min(S, y0 + p["rows"])
            assert ymin[y1 - 1] + ysize[y1 - 1] - ymin[y0] <= p["src_rows"]
    for bad in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (8, 8, 513), (65, 8, 8), (8, 65, 8)):
        with pytest.raises(VsError):
            ops.contrast_frames_plan(*bad)


def test_two_ranks_split_every_global_batch(fixture):
    """world = 2: the ranks' items are disjoint, together they are the global batch (the permutation in steps of
    2 b, the last one filled from the start), and both ranks get the same number of batches of full size."""
    seed = cl.EPOCHS["A"][2]
    per_rank = []
    for rank in (0, 1):
        ld = _loader(fixture, "A", rank=rank, world=2)
        torch.manual_seed(seed)
        per_rank.append([list(b) for b in ld._batches()])
        assert len(ld) == len(per_rank[-1]) == 5
    torch.manual_seed(seed)
    torch.empty((), dtype=torch.int64).random_()
    order = list(torch.utils.data.RandomSampler(range(48)))
    order = order + order[:2]                                       # 48 -> 50 = 5 global batches of 10
    for k, (a, b) in enumerate(zip(*per_rank)):
        assert len(a) == len(b) == cl.BATCH and not set(a) & set(b)
        assert a + b == order[10 * k:10 * (k + 1)]
    # each rank draws for its own items only
    ld = _loader(fixture, "A", rank=1, world=2)
    np.random.seed(3)
    tri = ld.draw(per_rank[1][0])
    assert list(tri[:, 0]) == per_rank[1][0] and (tri[:, 2] != tri[:, 0]).all()
    assert (np.abs(tri[:, 1] - tri[:, 0]) <= cl.IDX_OFFSET).all()


def test_trial_modes_and_raw_frames(fixture):
    """mode 'val': item i is trial i, (1, t, 1, S, S) with its spikes (1, T, N), in order.  transform=None: uint8
    frames, untouched, in pretrain mode the reference's sorted frames at the triplets."""
    data = _session(fixture, "A")
    ld = _loader(fixture, "A", mode="val", batch_size=1, shuffle=False)
    got = list(ld)
    assert len(got) == 2
    for i, b in enumerate(got):
        assert b["ref"].shape == (1, 6, 1, 24, 24) and b["neural"].shape == (1, 5, 7)
        assert np.array_equal(b["neural"][0].numpy(), data["val_y"][i])
        assert np.abs(b["ref"][0].numpy() - cl.transform(data["val_X"][i], 24)).max() == 0.0
    raw = _loader(fixture, "A", mode="test", batch_size=1, shuffle=False, transform=None)
    b = next(iter(raw))
    assert b["ref"].dtype == torch.uint8 and np.array_equal(b["ref"][0].numpy(), data["test_X"][0])
    raw = _loader(fixture, "A", transform=None)
    _seed("A")
    b = next(iter(raw))
    video = np.concatenate([data[f"{s}_X"] for s in ("train", "val", "test")]).reshape(48, 1, 20, 28)
    tri = fixture["A/triplets"][0][:cl.BATCH]
    for k, view in enumerate(("ref", "pos", "neg")):
        assert b[view].dtype == torch.uint8
        assert np.array_equal(b[view].numpy(), video[fixture["A/sort"]][tri[:, k]])


def test_fewer_than_two_frames_is_an_error():
    one = np.zeros((1, 1, 1, 4, 4), np.uint8)
    none = np.zeros((0, 1, 1, 4, 4), np.uint8)
    data = {"train_X": one, "val_X": none, "test_X": none, "train_timestamp": np.zeros((1, 1)),
            "val_timestamp": np.zeros((0, 1)), "test_timestamp": np.zeros((0, 1))}
    from vspike.data import ContrastFrames
    with pytest.raises(ValueError, match="at least 2 frames"):
        ContrastFrames(data, device="cpu")
    with pytest.raises(ValueError, match="invalid mode"):
        ContrastFrames(data, mode="all", device="cpu")


def test_make_contrast_loader_mirrors_the_reference(fixture):
    from vspike.data import ContrastFrames, make_contrast_loader
    ld, one = make_contrast_loader(_session(fixture, "A"), mode="pretrain", batch_size=7, shuffle=True, size=24,
                                   idx_offset=3, device="cpu")
    assert one == 1 and isinstance(ld, ContrastFrames) and (ld.batch_size, ld.idx_offset, ld.size) == (7, 3, 24)
    assert ld.video.dtype == torch.uint8 and ld.video.shape == (48, 1, 20, 28)
