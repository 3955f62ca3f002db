"""Trial shards and a pinned, prefetching batch loader — the input side of the hot path.

Replaces, for this path, the reference's data pipeline: per-trial webdataset tars
(src/prepare_data.py:210-235: `video.mp4` 120 x 128 x 128 gray at 60 fps + `ap.pyd` (100, N) spike
counts, key `<eid>_<trial>`) read by `BaseDataset` (src/loader/base.py:21-41: mp4 decode, first
channel -> (T, 1, H, W), `.float()`), collated by a torch DataLoader into
`{'video': (B, T, 1, H, W) f32, 'ap': (B, 100, N) f32, 'eid': [...], '__key__': [...]}`.

MI355X-first changes:
  * decode once, offline: `write_shard` stores raw uint8 frames in fixed-size, 4 KiB-aligned
    records (libvspike `vs_shard_*`, C++), so a batch is a set of parallel positional reads;
  * frames stay uint8 through the H2D copy (1/4 of the reference's f32 bytes: 1.97 MB instead of
    7.9 MB per clip) — the VideoMAE plugin's K0 kernel reads uint8 directly;
  * reads land in pinned host buffers on a background thread, the H2D copy runs asynchronously on
    a copy stream, and the consumer's stream waits on an event, so loading overlaps the train step.
Batch order: a seeded per-epoch permutation (the reference's webdataset shard shuffle + 10000-sample
buffer, src/loader/base.py:21-23, is not reproduced; sample order is not part of parity).

The contrastive pretraining input (src/loader/contrast.py, src/loader/make.py:33-60) is `ContrastFrames` /
`make_contrast_loader` below: a session's video held on the device as uint8, a batch of (ref, pos, neg) frames made
by one vs_contrast_frames launch, and there the sample order IS the reference's, draw for draw.
"""
from __future__ import annotations

import ctypes
import queue
import threading
from typing import List, Sequence

import numpy as np
import torch

from . import _lib as L
from ._lib import lib


def _err() -> str:
    e = lib().vs_shard_last_error()
    return e.decode() if e else "unknown error"


def write_shard(path: str, video, ap, keys: Sequence[str]) -> None:
    """video (n, T, C, H, W) uint8, ap (n, rows, cols) float32, keys n strings (< 64 bytes)."""
    v = np.ascontiguousarray(np.asarray(video))
    a = np.ascontiguousarray(np.asarray(ap, dtype=np.float32))
    if v.dtype != np.uint8 or v.ndim != 5:
        raise ValueError("write_shard: video must be uint8 (n, T, C, H, W)")
    if a.ndim != 3 or a.shape[0] != v.shape[0] or len(keys) != v.shape[0]:
        raise ValueError("write_shard: ap (n, rows, cols) and n keys expected")
    kb = bytearray(64 * len(keys))
    for i, k in enumerate(keys):
        b = k.encode()
        if len(b) >= 64:
            raise ValueError(f"write_shard: key too long: {k!r}")
        kb[64 * i:64 * i + len(b)] = b
    n, T, C, H, W = v.shape
    rc = lib().vs_shard_write(path.encode(), n, T, C, H, W, a.shape[1], a.shape[2], v.ctypes.data, a.ctypes.data,
                              bytes(kb))
    if rc != 0:
        raise OSError(_err())


class TrialShard:
    """One shard file: `len()`, `key(i)`, and `read(idx, video_out, ap_out)` into host tensors."""

    def __init__(self, path: str):
        info = (L.c_i64 * 8)()
        h = lib().vs_shard_open(path.encode(), info)
        if not h:
            raise OSError(f"{path}: {_err()}")
        self._h = h
        self.path = path
        self.n, T, C, H, W, rows, cols, _ = (int(x) for x in info)
        self.video_shape = (T, C, H, W)
        self.ap_shape = (rows, cols)

    def __len__(self):
        return self.n

    def key(self, i: int) -> str:
        buf = ctypes.create_string_buffer(80)
        if lib().vs_shard_key(self._h, int(i), buf, 80) != 0:
            raise IndexError(_err())
        return buf.value.decode()

    def read(self, idx, video_out: torch.Tensor, ap_out: torch.Tensor, threads: int = 8) -> None:
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64))
        n = len(idx)
        if video_out.dtype != torch.uint8 or video_out.device.type != "cpu" or not video_out.is_contiguous() or \
                video_out.numel() < n * int(np.prod(self.video_shape)):
            raise ValueError("TrialShard.read: video_out must be a contiguous host uint8 tensor of the batch size")
        if ap_out.dtype != torch.float32 or ap_out.device.type != "cpu" or not ap_out.is_contiguous() or \
                ap_out.numel() < n * int(np.prod(self.ap_shape)):
            raise ValueError("TrialShard.read: ap_out must be a contiguous host float32 tensor of the batch size")
        rc = lib().vs_shard_read(self._h, idx.ctypes.data_as(ctypes.POINTER(L.c_i64)), n, video_out.data_ptr(),
                                 ap_out.data_ptr(), int(threads))
        if rc != 0:
            raise OSError(f"{self.path}: {_err()}")

    def close(self):
        if getattr(self, "_h", None):
            lib().vs_shard_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardLoader:
    """Batches of {'video': (B, T, C, H, W) uint8, 'ap': (B, rows, cols) f32 — on `device` —
    'eid': [...], '__key__': [...]} from one or more shards (all of one geometry).

    Data parallel: with `world` > 1, `batch_size` is the per-rank batch and every
    rank walks the SAME seeded per-epoch permutation of all records in global batches of
    `batch_size * world`; rank r takes slice r of each global batch, so the ranks' batches are
    disjoint and together cover the global batch.  An incomplete last global batch is dropped
    (`drop_last`) or filled from the start of the permutation (every rank then still gets the
    same number of full batches: no rank waits at the gradient all-reduce for one that ran out).
    The reference splits by trial file (src/utils/dataset_utils.py:50-88) and its supervised entry
    does not shard the loaders at all (src/train.py:61-64 prepares only model/optimizer/scheduler)."""

    def __init__(self, paths: Sequence[str], batch_size: int, shuffle: bool = True, seed: int = 0, device="cuda",
                 drop_last: bool = False, threads: int = 8, prefetch: int = 2, rank: int = 0, world: int = 1):
        self.shards: List[TrialShard] = [TrialShard(p) for p in paths]
        if not self.shards:
            raise ValueError("ShardLoader: no shards")
        g = {(s.video_shape, s.ap_shape) for s in self.shards}
        if len(g) != 1:
            raise ValueError("ShardLoader: shards differ in geometry")
        self.video_shape, self.ap_shape = self.shards[0].video_shape, self.shards[0].ap_shape
        self.index = [(si, r) for si, s in enumerate(self.shards) for r in range(len(s))]
        self.keys = [self.shards[si].key(r) for si, r in self.index]
        self.batch_size, self.shuffle, self.seed, self.drop_last = int(batch_size), shuffle, int(seed), drop_last
        self.device, self.threads, self.prefetch = torch.device(device), int(threads), max(1, int(prefetch))
        self.rank, self.world = int(rank), int(world)
        if not (0 <= self.rank < self.world):
            raise ValueError(f"ShardLoader: rank {rank} outside world {world}")
        if self.world > 1 and len(self.index) < self.batch_size * self.world and drop_last:
            raise ValueError("ShardLoader: fewer records than one global batch with drop_last")
        self.epoch = 0

    def __len__(self):
        n, g = len(self.index), self.batch_size * self.world
        return n // g if self.drop_last else -(-n // g)

    def rank_batches(self, epoch: int):
        """Record numbers of this rank's batches in `epoch` (deterministic; no side effects)."""
        order = np.arange(len(self.index))
        if self.shuffle:
            np.random.RandomState(self.seed + epoch).shuffle(order)
        bs, W = self.batch_size, self.world
        if W == 1:
            batches = [order[i:i + bs] for i in range(0, len(order), bs)]
            if self.drop_last and batches and len(batches[-1]) < bs:
                batches.pop()
            return batches
        g = bs * W
        n_glob = len(order) // g if self.drop_last else -(-len(order) // g)
        need = n_glob * g
        if need > len(order):                       # fill the last global batch from the start
            order = np.concatenate([order, np.resize(order, need - len(order))])
        return [order[k * g + self.rank * bs: k * g + (self.rank + 1) * bs] for k in range(n_glob)]

    def _order(self):
        batches = self.rank_batches(self.epoch)
        self.epoch += 1
        return batches

    def _host_slots(self):
        pin = self.device.type == "cuda"
        B = self.batch_size
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=pin)  # noqa: E731
        return [(mk((B,) + self.video_shape, torch.uint8), mk((B,) + self.ap_shape, torch.float32))
                for _ in range(self.prefetch + 1)]

    def _fill(self, rows, v, a):
        """Gather `rows` (global record numbers) into the host slot, one vs_shard_read per shard."""
        by_shard = {}
        for k, gi in enumerate(rows):
            si, r = self.index[gi]
            by_shard.setdefault(si, ([], []))
            by_shard[si][0].append(k)
            by_shard[si][1].append(r)
        for si, (pos, recs) in by_shard.items():
            if pos == list(range(pos[0], pos[0] + len(pos))):
                self.shards[si].read(recs, v[pos[0]:], a[pos[0]:], self.threads)
            else:                                   # rows of several shards interleave: stage, then place
                tv = torch.empty((len(recs),) + self.video_shape, dtype=torch.uint8)
                ta = torch.empty((len(recs),) + self.ap_shape, dtype=torch.float32)
                self.shards[si].read(recs, tv, ta, self.threads)
                v[pos] = tv
                a[pos] = ta

    def __iter__(self):
        batches = self._order()
        slots = self._host_slots()
        cuda = self.device.type == "cuda"
        copy_stream = torch.cuda.Stream(self.device) if cuda else None
        slot_done = [None] * len(slots)             # event: the slot's H2D copy has finished
        free, ready = queue.Queue(), queue.Queue()   # at most len(slots) items: slots gate the reader
        for s in range(len(slots)):
            free.put(s)
        stop = threading.Event()

        def reader():
            try:
                for rows in batches:
                    s = free.get()
                    if stop.is_set():
                        return
                    if slot_done[s] is not None:
                        slot_done[s].synchronize()
                    v, a = slots[s]
                    self._fill(rows, v, a)
                    ready.put((s, rows))
                ready.put(None)
            except BaseException as e:              # surfaced in the consumer
                ready.put(e)

        th = threading.Thread(target=reader, daemon=True)
        th.start()
        try:
            while True:
                item = ready.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                s, rows = item
                n = len(rows)
                v, a = slots[s]
                if cuda:
                    with torch.cuda.stream(copy_stream):
                        dv = v[:n].to(self.device, non_blocking=True)
                        da = a[:n].to(self.device, non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(copy_stream)
                    slot_done[s] = ev
                    cur = torch.cuda.current_stream(self.device)
                    cur.wait_event(ev)
                    dv.record_stream(cur)
                    da.record_stream(cur)
                else:
                    dv, da = v[:n].clone(), a[:n].clone()
                free.put(s)
                keys = [self.keys[i] for i in rows]
                yield {"video": dv, "ap": da, "eid": [k.split("_")[0] for k in keys], "__key__": keys}
        finally:
            stop.set()
            free.put(0)
            th.join(timeout=10)


# ----------------------------------------------------------------------------------------------------------------
# The contrastive pretraining loader
# ----------------------------------------------------------------------------------------------------------------
class ContrastBatch(dict):
    """{'ref', 'pos', 'neg'}: three (b, 1, S, S) views of one (3b, 1, S, S) buffer, kept as `.all`."""
    all: torch.Tensor = None


def _device_frames(data, device, transform):
    """(F, 1, H, W) frames on the device in their own dtype: uint8 stays uint8; anything else becomes float32 (the
    reference's `torch.tensor(video, dtype=float32)`), or uint8 without a transform (its `dtype=torch.uint8`)."""
    v = torch.as_tensor(data)
    if v.dim() != 5 or v.shape[2] != 1:
        raise ValueError("ContrastFrames: video splits must be (n, t, 1, H, W)")
    if v.dtype != torch.uint8:
        v = v.to(torch.float32 if transform else torch.uint8)
    return v.reshape((-1,) + tuple(v.shape[2:])).contiguous().to(device)


class ContrastFrames:
    """The reference's `ContrastDataset` under its `DataLoader` (src/loader/contrast.py, src/loader/make.py:33-60)
    as one iterable over a session's video that stays on the device, from the dict `load_h5_file` returns for the
    session: `train_X / val_X / test_X` (n, t, 1, H, W), `*_y`, `*_timestamp`.

    mode 'pretrain': the frames of the three splits (train, val, test) are stored once in their own dtype; the
    reference's timestamp sort is kept as an index map, the video is not permuted.  A batch is {'ref', 'pos', 'neg'},
    three (b, 1, S, S) float32 views of one buffer that ONE vs_contrast_frames launch over 3b indices fills
    (`fused(batch)` is that buffer, for ContrastTrainer.step_fused).  The host's work per batch is the index draw
    and one small upload; no frame crosses the host link after construction.

    Sampling is the reference's, draw for draw.  The batch order comes from torch's RandomSampler / BatchSampler
    (shuffle, no drop_last) seeded from torch's global generator exactly as a DataLoader seeds them (one draw for
    the iterator's base seed, one for the permutation).  For each item i of a batch, in order,
        pos = int(np.random.uniform(max(0, i - idx_offset), min(F, i + idx_offset + 1)))
        neg = int(np.random.uniform(0, F)), drawn again while it equals i
    from numpy's global generator, when the batch is made (not per epoch), so that generator stands where the
    reference's stands at every batch boundary (ContrastTrainer.validate draws from it between passes).
    With `time_offset` the positive is np.random.choice over the frames with |timestamp - timestamp[i]| <=
    time_offset.  A quirk of the reference is kept: its __init__ overwrites the timestamps with
    linspace(0, len - 1, len) "if timestamp is None", but in pretrain mode that name has just been rebound to the
    concatenated timestamps, so the real (sorted) timestamps are used there although make_contrast_loader never
    passes the argument; only the trial modes get the linspace, where nothing reads it.  The fixture pins this.
    Fewer than 2 frames is an error (the reference's negative draw would never end).

    mode 'train' / 'val' / 'test': item i is trial i, {'ref': (1, t, 1, S, S), 'neural': (1, T, N)} (batch_size 1,
    the form ContrastTrainer.validate takes), one launch per batch over the trials' frames, in order unless
    `shuffle`.

    transform=None: frames come back uint8 and untouched, as the reference's do (plain indexing, no kernel).

    Data parallel (`rank`, `world`, ShardLoader's convention): every rank walks the same permutation (seed torch's
    global generator alike on every rank) in global batches of batch_size * world, rank r takes slice r, and an
    incomplete last global batch is filled from the start of the permutation; each rank draws positives and
    negatives for its own items only, from its own numpy generator, as the reference's separate processes do.
    This is this project's rule: what `accelerate` does to the reference's DataLoader is not reproduced.

    frame_fn(video, idx, size, mean, std) -> frames replaces the kernel call (the CPU tests' seam)."""

    MODES = ("pretrain", "train", "val", "test")

    def __init__(self, data, mode="pretrain", batch_size=512, shuffle=True, size=144, idx_offset=4, time_offset=None,
                 transform=True, mean=0.5, std=0.5, device="cuda", rank=0, world=1, frame_fn=None):
        if mode not in self.MODES:
            raise ValueError(f"ContrastFrames: invalid mode {mode!r}")
        self.mode, self.batch_size, self.shuffle = mode, int(batch_size), bool(shuffle)
        self.size, self.idx_offset, self.time_offset = int(size), idx_offset, time_offset
        self.transform, self.mean, self.std = bool(transform), float(mean), float(std)
        self.device, self.rank, self.world = torch.device(device), int(rank), int(world)
        if self.batch_size < 1:
            raise ValueError("ContrastFrames: batch_size must be positive")
        if not (0 <= self.rank < self.world):
            raise ValueError(f"ContrastFrames: rank {rank} outside world {world}")
        self._frame_fn = frame_fn
        splits = ("train", "val", "test") if mode == "pretrain" else (mode,)
        videos = [np.asarray(data[f"{s}_X"]) for s in splits]
        if len({v.shape[1:] for v in videos}) != 1:
            raise ValueError("ContrastFrames: the splits differ in (t, 1, H, W)")
        self.video = _device_frames(np.concatenate(videos, axis=0) if len(videos) > 1 else videos[0], self.device,
                                    self.transform)
        self.frames_per_trial = int(videos[0].shape[1])
        self.num_frames = int(self.video.shape[0])
        if mode == "pretrain":
            stamps = np.concatenate([np.asarray(data[f"{s}_timestamp"]) for s in splits], axis=0).reshape(-1)
            if stamps.shape[0] != self.num_frames:
                raise ValueError("ContrastFrames: one timestamp per frame expected")
            if self.num_frames < 2:
                raise ValueError("ContrastFrames: pretraining needs at least 2 frames (no negative exists otherwise)")
            self.sort = np.argsort(stamps)                    # item i is stored frame sort[i]
            self.timestamp = stamps[self.sort]
            self.num_items = self.num_frames
        else:
            self.labels = torch.as_tensor(np.asarray(data[f"{mode}_y"]))
            self.num_items = int(videos[0].shape[0])
            self.timestamp = np.linspace(0, self.num_items - 1, self.num_items)
            self._arange = torch.arange(self.num_frames, dtype=torch.int64, device=self.device)

    def __len__(self):
        g = self.batch_size * self.world
        return -(-self.num_items // g)

    # ---- sampling (host) ----
    def _batches(self):
        """This rank's batches of item numbers for one pass, drawing from torch's global generator as a DataLoader
        over the dataset does."""
        from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
        items = range(self.num_items)
        sampler = RandomSampler(items) if self.shuffle else SequentialSampler(items)
        torch.empty((), dtype=torch.int64).random_()          # the DataLoader iterator's base seed
        if self.world == 1:
            yield from BatchSampler(sampler, self.batch_size, drop_last=False)
            return
        order = list(sampler)
        bs, g = self.batch_size, self.batch_size * self.world
        n_glob = -(-len(order) // g)
        order = (order * (1 + (n_glob * g) // len(order)))[:n_glob * g]     # fill from the start
        for k in range(n_glob):
            yield order[k * g + self.rank * bs: k * g + (self.rank + 1) * bs]

    def _select_pos(self, i: int) -> int:
        if self.time_offset is None:
            lo, hi = max(0, i - self.idx_offset), min(self.num_frames, i + self.idx_offset + 1)
            return int(np.random.uniform(lo, hi))
        valid = np.where(abs(self.timestamp - self.timestamp[i]) <= self.time_offset)[0]
        return int(np.random.choice(valid)) if valid.size > 0 else i

    def _select_neg(self, i: int) -> int:
        while True:
            j = int(np.random.uniform(0, self.num_frames))
            if j != i:
                return j

    def draw(self, items) -> np.ndarray:
        """(b, 3) item numbers ref, pos, neg for a batch of items, drawn in the reference's order."""
        out = np.empty((len(items), 3), dtype=np.int64)
        for k, i in enumerate(items):
            out[k] = (i, self._select_pos(i), self._select_neg(i))
        return out

    # ---- frames (device) ----
    def _frames(self, idx: torch.Tensor) -> torch.Tensor:
        if not self.transform:
            return self.video[idx]
        if self._frame_fn is not None:
            return self._frame_fn(self.video, idx, self.size, self.mean, self.std)
        from . import ops
        return ops.contrast_frames(self.video, idx, self.size, self.mean, self.std, check_idx=False)

    def _upload(self, idx: np.ndarray) -> torch.Tensor:
        if idx.size and (idx.min() < 0 or idx.max() >= self.num_frames):
            raise IndexError("ContrastFrames: frame index out of range")
        t = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64))
        if self.device.type != "cuda":
            return t
        return t.pin_memory().to(self.device, non_blocking=True)

    def fused(self, batch) -> torch.Tensor:
        """The (3b, 1, S, S) buffer [ref | pos | neg] behind a pretrain batch."""
        x = getattr(batch, "all", None)
        if x is None:
            raise ValueError("ContrastFrames.fused: not a batch of this loader's pretrain mode")
        return x

    def __iter__(self):
        t = self.frames_per_trial
        for items in self._batches():
            items = [int(i) for i in items]
            if self.mode == "pretrain":
                tri = self.draw(items)
                x = self._frames(self._upload(self.sort[tri.T.reshape(-1)]))       # [ref | pos | neg]
                b = len(items)
                out = ContrastBatch(ref=x[:b], pos=x[b:2 * b], neg=x[2 * b:])
                out.all = x
                yield out
            else:
                if items == list(range(items[0], items[0] + len(items))):          # a run of trials: no upload
                    idx = self._arange[items[0] * t:(items[-1] + 1) * t]
                else:
                    idx = self._upload((np.asarray(items)[:, None] * t + np.arange(t)[None]).reshape(-1))
                x = self._frames(idx)
                yield {"ref": x.view((len(items), t) + tuple(x.shape[1:])),
                       "neural": self.labels[items].to(self.device, non_blocking=True)}


def make_contrast_loader(data, mode="pretrain", batch_size=512, shuffle=True, size=144, idx_offset=4, time_offset=None,
                         transform=True, device="cuda", rank=0, world=1, **kw):
    """The reference's make_contrast_loader (src/loader/make.py:33-60) on the loaded session dict `data` (where it
    takes the .h5 path and the session id): (loader, 1), as it returns.  transform: True = Resize((size, size)) +
    Normalize([0.5], [0.5]), the reference's (src/pretrain.py:60-66), on the device; None = raw uint8 frames."""
    return ContrastFrames(data, mode=mode, batch_size=batch_size, shuffle=shuffle, size=size, idx_offset=idx_offset,
                          time_offset=time_offset, transform=transform, device=device, rank=rank, world=world, **kw), 1
