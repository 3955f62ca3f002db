"""The contrastive loader at the workload's geometry: one session of 60,000 frames of 110 x 166 uint8 (the PCA bench's
session), b = 128 per view (384 frames per batch), S = 144.

* vs_contrast_frames over one batch's 384 indices (uint8 video, and the same frames as float32);
* the same batch as batched torch calls on the same GPU: index_select -> float -> / 255 -> F.interpolate(bilinear,
  antialias) -> (x - 0.5) / 0.5;
* the reference's literal form: per frame index, Resize, Normalize, then the DataLoader's stack (on a float32 video
  on the device, as its dataset holds it);
* torch's copy_ over the output's bytes (384 x 144 x 144 float32), the floor of anything that writes the batch;
* the host's draw per batch (RandomSampler order + the positive / negative draws + the index upload);
* ContrastTrainer's bf16 step fed by the loader (draw + kernel + step_fused) against the same step on ready-made
  tensors (scripts/contrast_bench.py's measurement).

Every figure is a median.  The kernel-sized ones time 10 calls between two events, enqueued behind a long matmul so
that the events see the device's time and not the host's launch rate; the same calls at the host's pace are
recorded beside them.
Prints one JSON line and writes it to profiles/contrast_loader_bench.json.
Usage: timeout -k 10 600 python scripts/contrast_loader_bench.py [--frames 60000] [--n 128] [--repeats 20] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-spike_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda"
H, W, S, T = 110, 166, 144, 120


def session(frames):
    """The loaded dict of one session: trials of 120 frames split 70 / 10 / 20 %, uint8 noise, one time per frame."""
    n = frames // T
    g = torch.Generator(device=DEV).manual_seed(3)
    video = torch.randint(0, 256, (n, T, 1, H, W), dtype=torch.uint8, device=DEV, generator=g).cpu().numpy()
    times = (np.arange(n * T) / 60.0).reshape(n, T)
    cut = (int(0.7 * n), int(0.8 * n))
    out = {}
    for name, sl in (("train", slice(0, cut[0])), ("val", slice(cut[0], cut[1])), ("test", slice(cut[1], n))):
        out[f"{name}_X"], out[f"{name}_timestamp"] = video[sl], times[sl]
        out[f"{name}_y"] = np.zeros((video[sl].shape[0], 100, 8), np.float32)
    return out


def torch_batched(video, idx):
    x = video.index_select(0, idx).float() / 255.0
    x = torch.nn.functional.interpolate(x, size=(S, S), mode="bilinear", align_corners=False, antialias=True)
    return (x - 0.5) / 0.5


def torch_per_frame(video_f32, idx_host):
    def one(i):
        x = video_f32[i]
        x = torch.nn.functional.interpolate(x[None], size=(S, S), mode="bilinear", align_corners=False, antialias=True)[0]
        return (x - 0.5) / 0.5
    return torch.stack([one(i) for i in idx_host])


def time_queued_us(fns, repeats, inner=10):
    """Median microseconds per call on the device: the `inner` calls are enqueued behind a long matmul, so the host
    is ahead of the GPU and the two events bracket back-to-back kernels, not the host's launch rate."""
    a = torch.randn(6144, 6144, device=DEV)
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a @ a
            s.record()
            for _ in range(inner):
                fn()
            e.record()
            torch.cuda.synchronize()
            us[k].append(1e3 * s.elapsed_time(e) / inner)
    return {k: round(statistics.median(v), 2) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60000)
    ap.add_argument("--n", type=int, default=128, help="frames per view")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrast_loader_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrast_loader_bench.py measures on the GPU; none is visible")
    from contrast_bench import _time_us, _trainer
    from vspike import _lib, ops
    from vspike.data import make_contrast_loader
    torch.manual_seed(0)
    np.random.seed(0)
    loader, _ = make_contrast_loader(session(a.frames), "pretrain", a.n, True, size=S, idx_offset=3, device=DEV)
    video, G = loader.video, 3 * a.n
    items = next(iter(loader._batches()))
    idx_host = loader.sort[loader.draw([int(i) for i in items]).T.reshape(-1)]
    idx = torch.from_numpy(idx_host).to(DEV)
    out = torch.empty(G, 1, S, S, device=DEV)
    got, want = ops.contrast_frames(video, idx, S), torch_batched(video, idx)
    dist = float((got - want).abs().max())
    sub = video[:4096].float()                               # the float32 runs: a slice, not 4.4 GB
    idx_sub = idx % 4096
    src, dst = torch.empty(G * S * S, device=DEV), torch.empty(G * S * S, device=DEV)
    fns = {
        "kernel_u8": lambda: ops.contrast_frames(video, idx, S, out=out, check_idx=False),
        "kernel_f32": lambda: ops.contrast_frames(sub, idx_sub, S, out=out, check_idx=False),
        "torch_batched_u8": lambda: torch_batched(video, idx),
        "copy_output_bytes": lambda: dst.copy_(src),
    }
    us = time_queued_us(fns, a.repeats)
    us_host = _time_us(fns, a.repeats)       # the same calls issued at the host's pace (scripts/contrast_bench.py's timer)
    # the per-frame form launches ~1,500 kernels: wall time of whole batches
    per_frame = []
    sub_host = [int(i) for i in idx_sub.cpu()]
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch_per_frame(sub, sub_host)
        torch.cuda.synchronize()
        per_frame.append(1e6 * (time.perf_counter() - t0))
    us["torch_per_frame_f32"] = round(statistics.median(per_frame), 1)
    # the host's share per batch: order + draws + upload (no kernel)
    draws = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        tri = loader.draw([int(i) for i in items])
        loader._upload(loader.sort[tri.T.reshape(-1)])
        draws.append(1e6 * (time.perf_counter() - t0))
    us["host_draw_and_upload"] = round(statistics.median(draws), 1)
    nbytes = {"read_u8": G * H * W, "written_f32": G * S * S * 4}
    rec = {"bench": "contrast_loader", "build_id": _lib.build_id(), "knobs": _lib.knobs_nondefault(),
           "device": torch.cuda.get_device_name(0),
           "config": {"frames": int(video.shape[0]), "H": H, "W": W, "S": S, "per_view": a.n, "batch_frames": G,
                      "repeats": a.repeats, "plan": ops.contrast_frames_plan(H, W, S)},
           "median_us": us, "median_us_at_the_hosts_launch_rate": us_host, "bytes": nbytes,
           "kernel_tb_per_s": round((nbytes["read_u8"] + nbytes["written_f32"]) / us["kernel_u8"] / 1e6, 3),
           "kernel_vs_torch_batched": round(us["torch_batched_u8"] / us["kernel_u8"], 2),
           "kernel_vs_torch_per_frame": round(us["torch_per_frame_f32"] / us["kernel_u8"], 1),
           "copy_over_kernel": round(us["copy_output_bytes"] / us["kernel_u8"], 3),
           "max_abs_distance_to_torch_batched": dist}
    # the bf16 step: ready-made tensors against batches from the loader (draw + upload + kernel + step_fused)
    tr = _trainer("bf16")
    views = [torch.randn(a.n, 1, S, S, device=DEV) for _ in range(3)]
    step = {}
    for name in ("ready_made", "from_loader"):
        it = iter(loader)
        run = (lambda: tr.step(*views)) if name == "ready_made" else \
            (lambda: (lambda b: tr.step_fused(loader.fused(b), a.n))(next(it)))
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                run()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / a.steps)
        step[name] = round(statistics.median(ms), 3)
    rec["bf16_step_ms"] = step
    rec["loader_share_of_step"] = round((step["from_loader"] - step["ready_made"]) / step["ready_made"], 4)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
