"""BASELINE C5 with its temporal stage: VideoMAETemporal against the plain VideoMAE plugin, and the token
pool kernels against the parent kernels they replace (vs_avgpool3d, vs_avgpool3d_bwd + vs_cast).

One process, interleaved repeats (models and kernels alternate inside every repeat, so clock and
neighbour drift hits both sides alike); medians are reported.  Geometry: ViT-Base, 32 frames (16 time
steps of 196 tokens), n = 1024 neurons, 16 clips, compute_dtype fp8 and bf16; whole train steps
(forward, backward, FusedAdamW) with a trainable and with a frozen encoder.  Kernel shape: G = 16 * B
groups, S = 196, D = 768.  The copy ceiling is torch's copy_ over the same number of bytes moved.

Prints one JSON line and writes it to profiles/temporal_c5_bench.json.
Usage: timeout -k 10 600 python scripts/temporal_bench.py [--clips 16] [--steps 5] [--repeats 5] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-spike_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DEV = "cuda"
BACKBONE = {"image_size": 224, "patch_size": 16, "num_channels": 3, "num_frames": 32, "tubelet_size": 2,
            "hidden_size": 768, "num_hidden_layers": 12, "num_attention_heads": 12, "intermediate_size": 3072}


def _model(cls, dtype, freeze, n):
    from vspike import NAME2MODEL
    conf = {"model_class": cls, "freeze_encoder": freeze, "compute_dtype": dtype, "backbone": dict(BACKBONE),
            "temporal": {"num_layers": 2}, "encoder": {"output_dim": 64}, "decoder": {"output_dim": 100 * n}}
    return NAME2MODEL[cls](conf).to(DEV)


def _trainer(m):
    from vspike import FusedAdamW
    from vspike.trainer import Trainer
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-5, weight_decay=0.01, eps=1e-8)
    return Trainer(m, opt)


def bench_models(dtype, freeze, clips, n, steps, repeats, warmup=3):
    """clips/s (median over repeats of `steps` train steps) of both plugins, alternating per repeat."""
    g = torch.Generator(device=DEV).manual_seed(5)
    px = torch.randn(clips, 32, 3, 224, 224, device=DEV, generator=g)
    y = (torch.rand(clips, 100, n, device=DEV, generator=g) < 0.12).float()
    names = ("VideoMAETemporal", "VideoMAE")
    trainers = {k: _trainer(_model(k, dtype, freeze, n)) for k in names}
    for t in trainers.values():
        for _ in range(warmup):
            t.step(px, y)
    torch.cuda.synchronize()
    rates = {k: [] for k in names}
    for _ in range(repeats):
        for k in names:
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = trainers[k].step(px, y)
            torch.cuda.synchronize()
            rates[k].append(steps * clips / (time.perf_counter() - t0))
            assert torch.isfinite(loss).item(), k
    out = {k: {"clips_per_s": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
           for k, v in rates.items()}
    out["params"] = {k: sum(p.numel() for p in trainers[k].model.parameters() if p.requires_grad) for k in names}
    del trainers
    torch.cuda.empty_cache()
    return out


def _time_us(fns, repeats, inner=10):
    """Median microseconds per call of each fn: every repeat times `inner` back-to-back calls of each in turn."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns]
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(repeats):
        for (k, fn), (s, e) in zip(fns.items(), ev):
            s.record()
            for _ in range(inner):
                fn()
            e.record()
        torch.cuda.synchronize()
        for k, (s, e) in zip(fns, ev):
            us[k].append(1e3 * s.elapsed_time(e) / inner)
    return {k: round(statistics.median(v), 2) for k, v in us.items()}


def bench_kernels(clips, repeats):
    from vspike import ops
    from vspike._lib import check, lib, stream
    G, S, D = 16 * clips, 196, 768
    x = torch.randn(G * S, D, device=DEV)
    pos = ops.sinusoid_table(16, D, DEV)
    out, out_lp = torch.empty(G, D, device=DEV), torch.empty(G, D, device=DEV, dtype=torch.bfloat16)
    dpool = torch.randn(G, D, device=DEV)
    dx, dx_lp = torch.empty(G * S, D, device=DEV), torch.empty(G * S, D, device=DEV, dtype=torch.bfloat16)
    old_out, old_dx = torch.empty_like(out), torch.empty_like(dx)      # the parent kernels' outputs

    def avgpool3d():                               # (N, voxels, C) = (G, S, D): the same layout
        check(lib().vs_avgpool3d(G, S, D, x.data_ptr(), old_out.data_ptr(), stream()), "vs_avgpool3d")

    def avgpool3d_bwd():
        check(lib().vs_avgpool3d_bwd(G, S, D, dpool.data_ptr(), old_dx.data_ptr(), stream()), "vs_avgpool3d_bwd")
    fwd_bytes = 4.0 * G * D * (S + 2)
    bwd_bytes = G * D * (4.0 + 6.0 * S)
    src = torch.empty(int(bwd_bytes) // 2, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    src_f = torch.empty(int(fwd_bytes) // 2, dtype=torch.uint8, device=DEV)
    dst_f = torch.empty_like(src_f)

    def old_bwd():
        avgpool3d_bwd()
        ops.cast(old_dx, dx_lp)

    res = _time_us({
        "token_pool_fwd": lambda: ops.token_pool_fwd(x, S, out, pos=pos, out_lp=out_lp),
        "avgpool3d": avgpool3d,
        "copy_fwd_bytes": lambda: dst_f.copy_(src_f),
        "token_pool_bwd": lambda: ops.token_pool_bwd(dpool, S, dx, dx_lp),
        "avgpool3d_bwd_plus_cast": old_bwd,
        "copy_bwd_bytes": lambda: dst.copy_(src),
    }, repeats)
    # what the new kernels compute, checked here against the old ones at the timed size
    ops.token_pool_fwd(x, S, out)
    avgpool3d()
    fwd_diff = float((out - old_out).abs().max())
    ops.token_pool_bwd(dpool, S, dx, dx_lp)
    avgpool3d_bwd()
    bwd_equal = bool(torch.equal(dx, old_dx) and torch.equal(dx_lp, old_dx.to(torch.bfloat16)))
    torch.cuda.synchronize()
    return {"shape": {"G": G, "S": S, "D": D}, "median_us": res, "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
            "fwd_speedup_vs_avgpool3d": round(res["avgpool3d"] / res["token_pool_fwd"], 3),
            "bwd_speedup_vs_avgpool3d_bwd_plus_cast": round(res["avgpool3d_bwd_plus_cast"] / res["token_pool_bwd"], 3),
            "fwd_fraction_of_copy": round(res["copy_fwd_bytes"] / res["token_pool_fwd"], 3),
            "bwd_fraction_of_copy": round(res["copy_bwd_bytes"] / res["token_pool_bwd"], 3),
            "fwd_TBps": round(fwd_bytes / res["token_pool_fwd"] / 1e6, 3),
            "bwd_TBps": round(bwd_bytes / res["token_pool_bwd"] / 1e6, 3),
            "fwd_max_abs_diff_vs_avgpool3d": fwd_diff, "bwd_bitwise_equal_avgpool3d_bwd_plus_cast": bwd_equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--neurons", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_c5_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("temporal_bench.py measures on the GPU; none is visible")
    from vspike import _lib
    rec = {"bench": "temporal_c5", "build_id": _lib.build_id(), "knobs": _lib.knobs_nondefault(),
           "device": torch.cuda.get_device_name(0),
           "config": {"clips": a.clips, "neurons": a.neurons, "frames": 32, "tokens": 3136, "time_steps": 16,
                      "temporal_layers": 2, "steps": a.steps, "repeats": a.repeats},
           "kernels": bench_kernels(a.clips, max(a.repeats, 20)), "models": {}}
    for dtype in ("fp8", "bf16"):
        for freeze in (False, True):
            key = f"{dtype}_{'frozen' if freeze else 'trainable'}_encoder"
            rec["models"][key] = bench_models(dtype, freeze, a.clips, a.neurons, a.steps, a.repeats)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
