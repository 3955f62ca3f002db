"""The ContrastViT pretraining step at the reference geometry: ViT-Base, 144 x 144 gray frames, n = 128 per view
(384 images, 31,488 token rows; config/model/contrast_vit.yaml + the reference's train_batch_size).

* images/s of the fused step (ContrastTrainer.step: one 3n forward, vs_info_nce, one backward, FusedAdamW) in
  bf16 and fp32, kernel timers off (median over repeats);
* per-class kernel times of one step with the timers on (side stream off, so every launch is timed alone),
  with the attention kernels' share at 82 tokens;
* the three new kernel families (csrc/contrast.hip) beside torch's copy_ over the same algorithmic bytes, and
  their summed share of the bf16 step.

Prints one JSON line and writes it to profiles/contrast_bench.json.
Usage: timeout -k 10 900 python scripts/contrast_bench.py [--n 128] [--steps 5] [--repeats 3] [--out PATH]
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


def _trainer(dtype):
    from vspike import NAME2MODEL, FusedAdamW
    from vspike.config import load_run_config
    from vspike.trainer import ContrastTrainer
    cfg = load_run_config(os.path.join(ROOT, "video-spike_amd", "config", "model", "contrast_vit.yaml"),
                          os.path.join(ROOT, "video-spike_amd", "config", "train", "vmae_video.yaml"))
    conf = dict(cfg.model)
    conf["compute_dtype"] = dtype
    m = NAME2MODEL[conf["model_class"]](conf).to(DEV)
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-5, weight_decay=0.01, eps=1e-8)
    return ContrastTrainer(m, opt)


def _views(n):
    g = torch.Generator(device=DEV).manual_seed(5)
    return [torch.randn(n, 1, 144, 144, device=DEV, generator=g) for _ in range(3)]


def bench_step(dtype, n, steps, repeats, warmup=2):
    from vspike import _lib as L, ops
    tr, views = _trainer(dtype), _views(n)
    for _ in range(warmup):
        tr.step(*views)
    torch.cuda.synchronize()
    rates = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            res = tr.step(*views)
        torch.cuda.synchronize()
        rates.append(steps * 3 * n / (time.perf_counter() - t0))
    assert torch.isfinite(res["loss"]).item()
    out = {"images_per_s": round(statistics.median(rates), 1), "min": round(min(rates), 1), "max": round(max(rates), 1),
           "ms_per_step": round(1e3 * 3 * n / statistics.median(rates), 3), "loss": round(float(res["loss"]), 5)}
    # one instrumented step: every launch bracketed by events, dW products in order on the main stream
    tr.model.set_side_stream(False)
    tr.step(*views)
    torch.cuda.synchronize()
    ops.timing_enable((1 << len(L.TIMER_NAMES)) - 1)
    L.dispatch_reset()
    tr.step(*views)
    torch.cuda.synchronize()
    classes = {}
    for i, name in enumerate(L.TIMER_NAMES):
        launches, ms = ops.timing_collect(i)
        if launches:
            classes[name] = {"launches": launches, "ms": round(ms, 4)}
    ops.timing_enable(0)
    total = sum(c["ms"] for c in classes.values())
    attn = sum(classes.get(k, {"ms": 0.0})["ms"] for k in ("attn_fwd", "attn_bwd"))
    out["timed_step"] = {"kernel_ms_total": round(total, 3), "classes": classes,
                         "attention_ms": round(attn, 3), "attention_share": round(attn / total, 4),
                         "dispatch": {k: v for k, v in L.dispatch_counts().items() if v}}
    del tr
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


def bench_kernels(n, repeats):
    """The new kernels at G = 3n images, P = 81, D = 768, E = 3 (bf16 step: bf16 copies written), each beside a
    plain copy over the bytes a perfect kernel moves (the library's own algorithmic-byte count)."""
    from vspike import ops
    G, P, D, E = 3 * n, 81, 768, 3
    z = lambda *s, dt=torch.float32: torch.randn(*s, device=DEV).to(dt)  # noqa: E731
    patches, cls, table, x = z(G * P, D), z(D), z(P + 1, D), z(G, P + 1, D)
    dx, d_cls, d_patch = z(G, P + 1, D), z(D), z(G * P, D, dt=torch.bfloat16)
    gamma, beta, w, b = z(D), z(D), z(E, D), z(E)
    h, mean, rstd, z_raw, nrm, zz = z(G, D), z(G), z(G), z(G, E), z(G), z(G, E)
    dz, dx_lp = z(G, E), z(G, P + 1, D, dt=torch.bfloat16)
    dw, db, dg, dbt = z(E, D), z(E), z(D), z(D)
    hws = torch.empty(ops.embed_head_bwd_workspace_bytes(G, D, E) // 4 + 4, device=DEV)
    ref, pos, neg = z(n, E), z(n, E), z(n, E)
    out, dr, dp, dq = z(3), z(n, E), z(n, E), z(n, E)
    nws = torch.empty(ops.info_nce_workspace_bytes(n, n) // 8 + 2, dtype=torch.float64, device=DEV)
    ops.embed_head_fwd(x, (P + 1) * D, gamma, beta, 1e-12, w, b, h, mean, rstd, z_raw, nrm, zz)
    nbytes = {
        "cls_embed_fwd": 4.0 * D * (G * P + G * (P + 1) + 2),
        "cls_embed_bwd": G * D * 4.0 + D * 4.0 + G * P * D * 6.0,
        "embed_head_fwd": 4.0 * (G * (2 * D + 2 * E + 3) + 2 * D + E * (D + 1)),
        "embed_head_bwd": G * (P + 1) * D * 6.0 + 4.0 * G * (D + 2 * E + 3) + 4.0 * D * (E + 1) + 4.0 * (G * D + E * D + E + 2 * D),
        "info_nce": 4.0 * E * 3 * n + 12 + 4.0 * E * 3 * n,
    }
    fns = {
        "cls_embed_fwd": lambda: ops.cls_embed_fwd(patches, cls, table, x),
        "cls_embed_bwd": lambda: ops.cls_embed_bwd(dx, d_cls, d_patch),
        "embed_head_fwd": lambda: ops.embed_head_fwd(x, (P + 1) * D, gamma, beta, 1e-12, w, b, h, mean, rstd, z_raw, nrm, zz),
        "embed_head_bwd": lambda: ops.embed_head_bwd(dz, x, (P + 1) * D, h, mean, rstd, z_raw, nrm, gamma, w, dx, dx_lp=dx_lp,
                                                    dw=dw, db=db, dgamma=dg, dbeta=dbt, workspace=hws),
        "info_nce": lambda: ops.info_nce(ref, pos, neg, out, d_ref=dr, d_pos=dp, d_neg=dq, workspace=nws),
    }
    copies = {}
    for k, nb in nbytes.items():
        src = torch.empty(max(int(nb) // 2, 16), dtype=torch.uint8, device=DEV)
        dst = torch.empty_like(src)
        copies["copy_" + k] = (lambda s=src, d=dst: d.copy_(s))
    res = _time_us({**fns, **copies}, repeats)
    return {"shape": {"G": G, "P": P, "D": D, "E": E, "n": n}, "median_us": res, "bytes": nbytes,
            "fraction_of_copy": {k: round(res["copy_" + k] / res[k], 3) for k in fns},
            "new_kernels_us_per_step": round(sum(res[k] for k in fns), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128, help="images per view (the reference's train_batch_size)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrast_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrast_bench.py measures on the GPU; none is visible")
    from vspike import _lib
    rec = {"bench": "contrast_vit", "build_id": _lib.build_id(), "knobs": _lib.knobs_nondefault(),
           "device": torch.cuda.get_device_name(0),
           "config": {"n": a.n, "images": 3 * a.n, "tokens": 82, "token_rows": 3 * a.n * 82, "embed_size": 3,
                      "steps": a.steps, "repeats": a.repeats},
           "kernels": bench_kernels(a.n, max(a.repeats, 20)), "step": {}}
    for dtype in ("bf16", "fp32"):
        rec["step"][dtype] = bench_step(dtype, a.n, a.steps, a.repeats)
    rec["new_kernels_share_of_bf16_step"] = round(
        rec["kernels"]["new_kernels_us_per_step"] / (1e3 * rec["step"]["bf16"]["ms_per_step"]), 5)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
