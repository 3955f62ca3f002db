"""The behaviour features at the workload's geometry: 400 trials, 119 flow frames (120 video frames) of 110 x 166 on one
MI355X: a 6.95 GB flow field and a 0.88 GB uint8 video.

* each kernel (vs_flow_median2, vs_flow_quantiles, vs_flow_clip_mean, vs_motion_energy) and the whole flow_features;
* torch's copy_ over the same input bytes (it also writes them: the time of reading AND writing the field once);
* the plain torch composition on the same GPU: medians as abs -> sort along the pixels -> the two middle elements;
  percentiles as abs -> sort along the trial -> the four ranks -> lerp; the clipped mean as clamp -> mean; the motion
  energy as float -> diff -> abs -> mean.  The compositions are checked against the kernels (medians and percentiles
  bit for bit, the means to 1e-6) before anything is timed.

Every figure is the median of `--repeats` runs between two device events after a warm-up run.
Prints one JSON line and writes it to --out (default profiles/flow_features_bench.json).
Usage: timeout -k 10 900 python scripts/flow_features_bench.py [--trials 400] [--repeats 5] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-spike_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DEV = "cuda"
FP, H, W = 119, 110, 166


def make_inputs(K):
    g = torch.Generator(device=DEV).manual_seed(7)
    video = torch.randint(0, 256, (K, FP + 1, H, W), dtype=torch.uint8, device=DEV, generator=g)
    flow = torch.empty(K, FP, H, W, 2, dtype=torch.float32, device=DEV)
    for k in range(K):                                       # a trial at a time: no second field-sized temporary
        scale = 0.2 + 3.0 * torch.rand(FP, 1, 1, 2, device=DEV, generator=g)
        flow[k] = torch.randn(FP, H, W, 2, device=DEV, generator=g) * scale
    return video, flow


def torch_medians(flow, chunk=50):
    K, n = flow.shape[0], H * W
    out = torch.empty(K, FP, 2, device=DEV)
    for k0 in range(0, K, chunk):
        s = flow[k0:k0 + chunk].abs().view(-1, FP, n, 2).sort(dim=2).values
        out[k0:k0 + chunk] = (s[:, :, (n - 1) // 2] + s[:, :, n // 2]) / 2
    return out


def torch_quantiles(flow, ranks, gammas, chunk=50):
    K, n = flow.shape[0], FP * H * W
    out = torch.empty(K, 2, 2, device=DEV)
    for k0 in range(0, K, chunk):
        s = flow[k0:k0 + chunk].abs().view(-1, n, 2).sort(dim=1).values
        for j, t in enumerate(gammas):
            a, b = s[:, ranks[2 * j]], s[:, ranks[2 * j + 1]]
            d = b - a
            out[k0:k0 + chunk, :, j] = a + d * t if t < 0.5 else b - d * (1 - t)
    return out


def torch_clip_mean(flow, bounds):
    lo, hi = bounds[:, None, None, None, :, 0], bounds[:, None, None, None, :, 1]
    return torch.minimum(torch.maximum(flow.abs(), lo), hi).mean(dim=(2, 3, 4))


def torch_motion_energy(video, chunk=100):
    out = torch.empty(video.shape[0], FP, device=DEV)
    for k0 in range(0, video.shape[0], chunk):
        v = video[k0:k0 + chunk].float()
        out[k0:k0 + chunk] = (v[:, 1:] - v[:, :-1]).abs().mean(dim=(2, 3))
    return out


def time_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_features_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "flow_features_bench needs a GPU"
    from vspike import behaviour, ops
    import flow_features_ref as fr

    K = args.trials
    video, flow = make_inputs(K)
    n = FP * H * W
    r10, r90 = fr.percentile_ranks(n, 10), fr.percentile_ranks(n, 90)
    ranks, gammas = [r10[0], r10[1], r90[0], r90[1]], [float(r10[2]), float(r90[2])]
    bounds = ops.flow_quantiles(flow)

    # the compositions compute what the kernels compute
    med_k, med_t = ops.flow_median2(flow, absolute=True), torch_medians(flow)
    checks = {"medians_bit_equal": bool(torch.equal(med_k, med_t)),
              "percentiles_max_abs_diff": float((bounds - torch_quantiles(flow, ranks, gammas)).abs().max()),
              "clip_mean_max_abs_diff": float((ops.flow_clip_mean(flow, bounds) - torch_clip_mean(flow, bounds)).abs().max()),
              "motion_energy_max_abs_diff": float((ops.motion_energy(video) - torch_motion_energy(video)).abs().max())}
    del med_k, med_t
    torch.cuda.empty_cache()

    flow_copy, video_copy = torch.empty_like(flow), torch.empty_like(video)
    ws = torch.empty(int(ops.lib().vs_flow_quantiles_workspace_bytes(K)), dtype=torch.uint8, device=DEV)
    ms = {
        "median2": time_ms(lambda: ops.flow_median2(flow, absolute=True), args.repeats),
        "median2_signed": time_ms(lambda: ops.flow_median2(flow, absolute=False), args.repeats),
        "quantiles": time_ms(lambda: ops.flow_quantiles(flow, workspace=ws), args.repeats),
        "clip_mean": time_ms(lambda: ops.flow_clip_mean(flow, bounds), args.repeats),
        "motion_energy_u8": time_ms(lambda: ops.motion_energy(video), args.repeats),
        "flow_features": time_ms(lambda: behaviour.flow_features(video, flow), args.repeats),
        "copy_flow": time_ms(lambda: flow_copy.copy_(flow), args.repeats),
        "copy_video": time_ms(lambda: video_copy.copy_(video), args.repeats),
    }
    del flow_copy, video_copy
    video_f32 = video.float()
    ms["motion_energy_f32"] = time_ms(lambda: ops.motion_energy(video_f32), args.repeats)
    del video_f32
    torch.cuda.empty_cache()
    ms["torch_medians"] = time_ms(lambda: torch_medians(flow), args.repeats)
    ms["torch_quantiles"] = time_ms(lambda: torch_quantiles(flow, ranks, gammas), args.repeats)
    ms["torch_clip_mean"] = time_ms(lambda: torch_clip_mean(flow, bounds), args.repeats)
    ms["torch_motion_energy"] = time_ms(lambda: torch_motion_energy(video), args.repeats)

    gb_flow, gb_video = flow.numel() * 4 / 1e9, video.numel() / 1e9
    res = {
        "bench": "flow_features", "device": torch.cuda.get_device_name(0), "trials": K, "flow_frames": FP, "H": H, "W": W,
        "flow_GB": round(gb_flow, 3), "video_GB": round(gb_video, 3), "repeats": args.repeats,
        "ms": {k: round(v, 3) for k, v in ms.items()},
        "read_GBps": {"median2": round(gb_flow / ms["median2"] * 1e3, 1),
                      "quantiles_per_pass": round(4 * gb_flow / ms["quantiles"] * 1e3, 1),
                      "clip_mean": round(gb_flow / ms["clip_mean"] * 1e3, 1),
                      "motion_energy_u8": round(gb_video / ms["motion_energy_u8"] * 1e3, 1),
                      "copy_flow_read_plus_write": round(2 * gb_flow / ms["copy_flow"] * 1e3, 1)},
        "vs_copy": {"median2": round(ms["median2"] / ms["copy_flow"], 2),
                    "quantiles": round(ms["quantiles"] / ms["copy_flow"], 2),
                    "clip_mean": round(ms["clip_mean"] / ms["copy_flow"], 2),
                    "motion_energy_u8": round(ms["motion_energy_u8"] / ms["copy_video"], 2)},
        "torch_over_kernel": {"median2": round(ms["torch_medians"] / ms["median2"], 2),
                              "quantiles": round(ms["torch_quantiles"] / ms["quantiles"], 2),
                              "clip_mean": round(ms["torch_clip_mean"] / ms["clip_mean"], 2),
                              "motion_energy_u8": round(ms["torch_motion_energy"] / ms["motion_energy_u8"], 2)},
        "checks": checks, "plan": ops.flow_plan(),
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
