#!/usr/bin/env python
"""Generate tests/golden/contrast_loader.npz: what the reference's contrastive loader yields for seeded tiny sessions.

Run once, where the reference checkout is readable (torch on the CPU is all it needs):

    python scripts/gen_contrast_loader_fixture.py --reference /path/to/video-spike

The reference's `ContrastDataset` (src/loader/contrast.py) is taken out of its module by name with `ast` at run time,
into a namespace that holds torch, numpy and torch's Dataset (the module imports webdataset and torchvision at its
top and cannot be imported whole); no reference text is stored.  Its `transform` argument is the two torchvision
transforms of src/pretrain.py:60-66 restated as the torch calls they make on a float tensor,
`F.interpolate(x, (S, S), mode="bilinear", align_corners=False, antialias=True)` and `(x - 0.5) / 0.5`, and the
dataset runs under a real torch.utils.data.DataLoader(batch_size, shuffle=True) on the CPU.  The positive and
negative index of every item are read off the dataset's own `_select_pos_idx` / `_select_neg_idx` through wrappers
that only log what those return.

Per session of tests/contrast_loader_ref.py (A: 20 x 28, idx_offset mode, two epochs; B: 40 x 19, time_offset mode,
one epoch; both -> 24, splits of 4 / 2 / 2 trials of 6 frames, shuffled timestamps, batches of 5):
  <s>/<split>_X, _y, _timestamp   the session dict
  <s>/sort                        the dataset's frame order: np.argsort of the concatenated timestamps
  <s>/triplets                    (epochs, 48, 3) int64: ref, pos, neg of every item in the order the loader gave them
  <s>/next_draw                   (epochs,) numpy's global generator's next draw after each epoch
  <s>/ref_frames                  (48, 1, 24, 24) float32: the dataset's transform of every frame, in its own order;
                                  every batch the loader gave is checked here to be these frames at the triplets
  <s>/restatement                 (8, 1, 24, 24) float64: tests/contrast_loader_ref.transform of the first 8 of them
  <s>/d_ref                       the reference's largest distance to the restatement over all 48 frames
W: one batch of 2 at the workload's 110 x 166 -> 144 (idx_offset mode, 2 / 1 / 1 trials of one frame):
  W/video, W/sort, W/triplets, W/ref_frames (4 frames), W/restatement (frame 0), W/d_ref
and per geometry of contrast_loader_ref.EXTRA_GEOMETRIES, on contrast_loader_ref.extra_frames:
  extra/<H>x<W>_<S>/d_ref
"""
import argparse
import ast
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True          # never write into the reference checkout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import contrast_loader_ref as cl        # noqa: E402


def reference_class(reference):
    """The reference's ContrastDataset, compiled from its own file into a namespace with what its body uses."""
    path = os.path.join(reference, "src", "loader", "contrast.py")
    tree = ast.parse(open(path).read(), filename=path)
    defs = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ContrastDataset"]
    assert len(defs) == 1, path
    ns = {"np": np, "torch": torch, "Dataset": torch.utils.data.Dataset}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns["ContrastDataset"]


def make_transform(size):
    def transform(x):                   # (1, H, W) or (t, 1, H, W) float32, as torchvision's Resize + Normalize
        y = x[None] if x.dim() == 3 else x
        y = torch.nn.functional.interpolate(y, size=(size, size), mode="bilinear", align_corners=False, antialias=True)
        y = y[0] if x.dim() == 3 else y
        return (y - 0.5) / 0.5
    return transform


def logged(dataset):
    """Log (ref, pos, neg) per item from the dataset's own methods."""
    log = []
    pos_fn, neg_fn, cls = dataset._select_pos_idx, dataset._select_neg_idx, type(dataset)

    def pos(idx):
        r = pos_fn(idx)
        log.append([int(idx), int(r), -1])
        return r

    def neg(idx):
        r = neg_fn(idx)
        assert log[-1][0] == int(idx) and log[-1][2] == -1
        log[-1][2] = int(r)
        return r
    dataset._select_pos_idx, dataset._select_neg_idx = pos, neg
    return log


def run_epochs(dataset, ref_frames, batch, epochs, seed):
    log = logged(dataset)
    torch.manual_seed(seed)
    np.random.seed(seed)
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch, shuffle=True)
    triplets, draws = [], []
    for _ in range(epochs):
        del log[:]
        at = 0
        for b in loader:
            n = b["ref"].shape[0]
            tri = np.array(log[at:at + n], dtype=np.int64)
            for k, name in enumerate(("ref", "pos", "neg")):
                assert torch.equal(b[name], ref_frames[tri[:, k]]), "a batch is not the per-frame transform"
            at += n
        assert at == len(log) == len(dataset)
        triplets.append(np.array(log, dtype=np.int64))
        draws.append(cl.peek_numpy())
    return np.stack(triplets), np.array(draws)


def d_ref_of(frames_u8, size):
    """(torch's float32 result, the restatement, the largest distance) for (n, 1, H, W) uint8 frames."""
    x = torch.tensor(frames_u8, dtype=torch.float32).div_(255.0)
    got = make_transform(size)(x).numpy()
    want = cl.transform(frames_u8, size)
    return got, want, float(np.abs(got.astype(np.float64) - want).max())


def session_arrays(ContrastDataset, data, size, mode, batch, epochs, seed, keep):
    kw = dict(idx_offset=cl.IDX_OFFSET) if mode == "idx" else dict(idx_offset=cl.IDX_OFFSET, time_offset=cl.TIME_OFFSET)
    ds = ContrastDataset(data, mode="pretrain", transform=make_transform(size), device="cpu", **kw)
    stamps = np.concatenate([data[f"{s}_timestamp"] for s in ("train", "val", "test")], axis=0).reshape(-1)
    sort = np.argsort(stamps)
    video = np.concatenate([data[f"{s}_X"] for s in ("train", "val", "test")], axis=0)
    video = video.reshape((-1,) + video.shape[2:])
    assert np.array_equal(ds.timestamp, stamps[sort]), "the dataset keeps the sorted timestamps in pretrain mode"
    assert torch.equal(ds.video, torch.tensor(video[sort], dtype=torch.float32).div_(255.0))
    ref_frames = torch.stack([ds.transform(ds.video[i]) for i in range(len(ds))])
    triplets, draws = run_epochs(ds, ref_frames, batch, epochs, seed)
    got, want, d = d_ref_of(video[sort], size)
    assert np.array_equal(got, ref_frames.numpy())
    return {"sort": sort.astype(np.int64), "triplets": triplets, "next_draw": draws,
            "ref_frames": ref_frames.numpy(), "restatement": want[:keep], "d_ref": np.float64(d)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "contrast_loader.npz"))
    args = ap.parse_args()
    ContrastDataset = reference_class(args.reference)
    out = {}
    for name, g in cl.SESSIONS.items():
        data = cl.make_session(name)
        mode, epochs, seed = cl.EPOCHS[name]
        for k, v in data.items():
            out[f"{name}/{k}"] = v
        for k, v in session_arrays(ContrastDataset, data, g["S"], mode, cl.BATCH, epochs, seed, keep=8).items():
            out[f"{name}/{k}"] = v
        tri = out[f"{name}/triplets"]
        assert (tri[..., 2] != tri[..., 0]).all() and sorted(tri[0, :, 0]) == list(range(48))
        print(f"{name}: d_ref {out[f'{name}/d_ref']:.3e}, |pos - ref| up to {np.abs(tri[..., 1] - tri[..., 0]).max()}")
    # the workload's geometry: 4 frames, one batch of 2 recorded
    H, W, S = 110, 166, 144
    video = cl.noise_frames(H, W, 4, 303)
    data = {"train_X": video[:2, None], "val_X": video[2:3, None], "test_X": video[3:4, None],
            "train_y": np.zeros((2, 1, 1), np.float32), "val_y": np.zeros((1, 1, 1), np.float32),
            "test_y": np.zeros((1, 1, 1), np.float32),
            "train_timestamp": np.array([[0.3], [0.1]]), "val_timestamp": np.array([[0.4]]),
            "test_timestamp": np.array([[0.2]])}
    w = session_arrays(ContrastDataset, data, S, "idx", 2, 1, 13, keep=1)
    out["W/video"] = video
    for k in ("sort", "ref_frames", "restatement", "d_ref"):
        out[f"W/{k}"] = w[k]
    out["W/triplets"] = w["triplets"][:, :2]
    print(f"W: d_ref {w['d_ref']:.3e}")
    for (H, W, S) in cl.EXTRA_GEOMETRIES:
        _, _, d = d_ref_of(cl.extra_frames(H, W, S), S)
        out[f"extra/{H}x{W}_{S}/d_ref"] = np.float64(d)
        print(f"extra {H}x{W} -> {S}: d_ref {d:.3e}")
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")
    assert os.path.getsize(args.out) < (1 << 20)


if __name__ == "__main__":
    main()
