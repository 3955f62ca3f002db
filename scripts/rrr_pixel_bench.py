"""The RRR baseline straight from the pixels at the session the contrast loader and the PCA are measured on:
110 x 166 uint8 frames (C = 18,260), K = 400 / 100 trials, F = 120 frames of which T = 100 are used, N = 512,
r = 3, y float32 (src/train_rrr.py --input_mod whisker-video).  The method is scripts/rrr_wide_bench.py's.

* microseconds per vs_rrr_pixel_loss_grad call, with gradients and loss only (device events around `--calls`
  back-to-back calls, median of `--repeats` windows, alternating with the baseline), the float64 flop rate of its two
  products per bin (2 x 2 K T (C+1) N flops; loss only: one product), vs_rrr_pixel_score on the validation split and
  vs_rrr_pixel_stats on the training split;
* two float64 torch.bmm calls of the two per-bin products' shapes: the library's rate on the same flops (its
  operands alone are 27 GB);
* the whole 20-closure fit (RRRGD.fit on PixelFeatures), host clock around a synchronise, with
  torch.cuda.max_memory_allocated over it;
* the materialised route: the standardised float64 X [K, T, C+1] plus the torch einsum + autograd closure, one call
  and the whole fit, with their peak memory; the two routes are compared on the same inputs first (1e-12).  If it
  does not fit, the JSON says so;
* at C = 768 (same K, F, T, N, r): the pixel entry on uint8 frames against vs_rrr_wide_loss_grad on the
  materialised X.

Prints one JSON line and writes it to profiles/rrr_pixel_bench.json.
Usage: timeout -k 10 900 python scripts/rrr_pixel_bench.py [--calls 3] [--repeats 3] [--out PATH]
"""
import argparse
import gc
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

from rrr_bench import DEV, event_us, torch_loss_grad  # noqa: E402
from rrr_wide_bench import torch_fit  # noqa: E402


def make_inputs(K, Kv, F, T, N, C, r):
    g = torch.Generator(device=DEV).manual_seed(3)
    X = torch.randint(0, 256, (K, F, C), device=DEV, dtype=torch.uint8, generator=g)
    Xv = torch.randint(0, 256, (Kv, F, C), device=DEV, dtype=torch.uint8, generator=g)
    idx = np.sort(np.random.RandomState(0).choice(F - 1, T, replace=False))
    y = torch.randn(K, T, N, device=DEV, generator=g)
    gt = torch.poisson(torch.full((Kv, T, N), 0.6, device=DEV), generator=g)
    U = torch.randn(N, C, r, device=DEV, dtype=torch.float64, generator=g) / (T * r) ** 0.5 / (C / 768.0) ** 0.5
    V = torch.randn(r, T, device=DEV, dtype=torch.float64, generator=g) / (T * r) ** 0.5
    b = 0.1 * torch.randn(N, 1, T, device=DEV, dtype=torch.float64, generator=g)
    return X, Xv, idx, y, gt, U, V, b


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, n


def peak_gb(fn):
    """(result, peak bytes allocated while fn ran beyond what was allocated before it, in GB)."""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, (torch.cuda.max_memory_allocated() - base) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rrr_pixel_bench.json"))
    ap.add_argument("--shape", type=int, nargs=7, default=[400, 100, 120, 100, 512, 18260, 3],
                    metavar=("K", "KVAL", "F", "T", "N", "C", "R"))
    ap.add_argument("--narrow-c", type=int, default=768)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rrr_pixel_bench needs a GPU")
    from vspike import _lib as L, ops
    from vspike.rrr import RRRGD, PixelFeatures
    K, Kv, F, T, N, C, r = a.shape
    l2 = 100.0
    X, Xv, idx, y, gt, U, V, b = make_inputs(K, Kv, F, T, N, C, r)
    mean, std = ops.rrr_pixel_stats(X)
    feats, feats_v = PixelFeatures(X, idx, mean, std), PixelFeatures(Xv, idx, mean, std)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    dU, dV, db = (torch.zeros_like(t) for t in (U, V, b))
    need = ops.rrr_pixel_loss_grad_workspace_bytes(K, T, N, C, r)
    ws = torch.empty(need // 8 + 2, dtype=torch.float64, device=DEV)

    def pixel():
        ops.rrr_pixel_loss_grad(X, feats.idx, mean, std, y, U, V, b, l2, loss, dU=dU, dV=dV, db=db, workspace=ws)

    def loss_only():
        ops.rrr_pixel_loss_grad(X, feats.idx, mean, std, y, U, V, b, l2, loss, workspace=ws)

    def stats():
        ops.rrr_pixel_stats(X, mean=mean, std=std)

    bps, r2 = (torch.zeros(N, dtype=torch.float64, device=DEV) for _ in range(2))
    out2 = torch.zeros(2, dtype=torch.float64, device=DEV)
    pred = torch.zeros(Kv, T, N, dtype=torch.float64, device=DEV)
    mean_y = 0.5 + torch.rand(T, N, dtype=torch.float64, device=DEV)
    std_y = 0.5 + torch.rand(T, N, dtype=torch.float64, device=DEV)
    sws = torch.empty(ops.rrr_pixel_score_workspace_bytes(Kv, T, N) // 8 + 2, dtype=torch.float64, device=DEV)

    def score():
        ops.rrr_pixel_score(Xv, feats.idx, mean, std, U, V, b, mean_y, std_y, gt, bps, r2, out2, pred=pred,
                            workspace=sws)
    for fn in (pixel, loss_only, score, stats):
        event_us(fn, 1)
    t_p, t_lo, t_sc, t_st = [], [], [], []
    for _ in range(a.repeats):
        t_p.append(event_us(pixel, a.calls))
        t_lo.append(event_us(loss_only, a.calls))
        t_sc.append(event_us(score, a.calls))
        t_st.append(event_us(stats, a.calls))
    us_p, us_lo, us_sc, us_st = (statistics.median(t) for t in (t_p, t_lo, t_sc, t_st))
    flops = 2 * 2.0 * K * T * (C + 1) * N

    # the whole fit from the pixels, with its peak memory (the video, y and the statistics are there already)
    def fit_pixel():
        return RRRGD(r, l2).fit({"s": (feats, y)}).func_evals
    wall_ms(fit_pixel)
    (ms_fit, evals), fit_peak = peak_gb(lambda: wall_ms(fit_pixel))
    resident_gb = (X.numel() + y.numel() * 4 + 2 * mean.numel() * 8) / 1e9
    res = {
        "bench": "rrr_pixel", "arch": torch.cuda.get_device_properties(0).gcnArchName, "build_id": L.build_id(),
        "knobs": L.knobs_nondefault(),
        "shape": {"K_train": K, "K_val": Kv, "F": F, "T": T, "N": N, "C": C, "r": r, "X": "uint8", "y": "float32"},
        "workspace_bytes": need, "standardisation": "true division at the operand load",
        "loss_grad_us": round(us_p, 1), "loss_grad_us_windows": [round(t, 1) for t in t_p],
        "loss_grad_f64_tflops": round(flops / us_p * 1e-6, 2),
        "loss_only_us": round(us_lo, 1), "loss_only_f64_tflops": round(0.5 * flops / us_lo * 1e-6, 2),
        "score_us": round(us_sc, 1), "stats_us": round(us_st, 1),
        "stats_gbs": round(2.0 * X.numel() / us_st * 1e-3, 1),
        "fit_ms": round(ms_fit, 1), "fit_func_evals": int(evals), "fit_kernel_share": round(20 * us_p * 1e-3 / ms_fit, 3),
        "fit_peak_gb_beyond_inputs": round(fit_peak, 3), "inputs_resident_gb": round(resident_gb, 3),
        "calls_per_window": a.calls, "repeats": a.repeats,
    }

    # the library on the same flops: the two per-bin products as batched float64 GEMMs
    try:
        A1 = torch.randn(T, K, C + 1, device=DEV, dtype=torch.float64)
        B1 = torch.randn(T, C + 1, N, device=DEV, dtype=torch.float64)
        A2 = A1.transpose(1, 2).contiguous()
        B2 = torch.randn(T, K, N, device=DEV, dtype=torch.float64)
        O1 = torch.empty(T, K, N, device=DEV, dtype=torch.float64)
        O2 = torch.empty(T, C + 1, N, device=DEV, dtype=torch.float64)

        def bmm2():
            torch.bmm(A1, B1, out=O1)
            torch.bmm(A2, B2, out=O2)
        event_us(bmm2, 1)
        us_b = statistics.median(event_us(bmm2, a.calls) for _ in range(a.repeats))
        res.update({"torch_bmm_f64_two_products_us": round(us_b, 1), "torch_bmm_f64_tflops": round(flops / us_b * 1e-6, 2),
                    "loss_grad_over_bmm": round(us_p / us_b, 2),
                    "torch_bmm_operand_gb": round(sum(t.numel() for t in (A1, B1, A2, B2, O1, O2)) * 8 / 1e9, 1)})
        del A1, B1, A2, B2, O1, O2
    except torch.cuda.OutOfMemoryError as e:
        res["torch_bmm_f64_two_products_us"] = f"does not fit: {str(e)[:80]}"

    # the materialised route: float64 X and the torch closure
    try:
        Xm, mat_peak = peak_gb(feats.materialise)
        pixel()
        (tl, tU, tV, tb), call_peak = peak_gb(lambda: torch_loss_grad(Xm, y, U, V, b, l2))
        agree = {"loss": float((loss[0] - tl).abs() / tl.abs()), "dU": float((dU - tU).norm() / tU.norm()),
                 "dV": float((dV - tV).norm() / tV.norm()), "db": float((db - tb).norm() / tb.norm())}
        assert max(agree.values()) <= 1e-12, agree
        del tl, tU, tV, tb
        event_us(lambda: torch_loss_grad(Xm, y, U, V, b, l2), 1)
        us_c = statistics.median(event_us(lambda: torch_loss_grad(Xm, y, U, V, b, l2), a.calls) for _ in range(a.repeats))
        (ms_c, evals_c), fit_c_peak = peak_gb(lambda: wall_ms(lambda: torch_fit(Xm, y, r, l2)))
        res.update({"materialised_X_gb": round(Xm.numel() * 8 / 1e9, 2), "materialise_peak_gb": round(mat_peak, 2),
                    "torch_f64_composition_us": round(us_c, 1), "speedup_vs_torch_composition": round(us_c / us_p, 2),
                    "torch_f64_composition_peak_gb_beyond_X": round(call_peak, 2),
                    "agreement_with_torch_composition": agree,
                    "fit_ms_torch_closure": round(ms_c, 1), "fit_torch_closure_func_evals": int(evals_c),
                    "fit_torch_closure_peak_gb_with_X": round(fit_c_peak + Xm.numel() * 8 / 1e9, 2)})
        del Xm
    except torch.cuda.OutOfMemoryError as e:
        res["materialised_route"] = f"does not fit: {str(e)[:80]}"
    gc.collect()
    torch.cuda.empty_cache()

    # C = 768: the pixel entry on uint8 frames against the wide entry on the materialised X
    Cn = a.narrow_c
    X, Xv, idx, y, gt, U, V, b = make_inputs(K, Kv, F, T, N, Cn, r)
    mean, std = ops.rrr_pixel_stats(X)
    feats = PixelFeatures(X, idx, mean, std)
    Xm = feats.materialise()
    dU, dV, db = (torch.zeros_like(t) for t in (U, V, b))
    wU, wV, wb = (torch.zeros_like(t) for t in (U, V, b))
    wloss = torch.zeros(1, dtype=torch.float64, device=DEV)
    ws = torch.empty(ops.rrr_pixel_loss_grad_workspace_bytes(K, T, N, Cn, r) // 8 + 2, dtype=torch.float64, device=DEV)
    wws = torch.empty(ops.rrr_wide_loss_grad_workspace_bytes(K, T, N, Cn) // 8 + 2, dtype=torch.float64, device=DEV)

    def pixel_n():
        ops.rrr_pixel_loss_grad(X, feats.idx, mean, std, y, U, V, b, l2, loss, dU=dU, dV=dV, db=db, workspace=ws)

    def wide_n():
        ops.rrr_wide_loss_grad(Xm, y, U, V, b, l2, wloss, dU=wU, dV=wV, db=wb, workspace=wws)
    event_us(pixel_n, 2)
    event_us(wide_n, 2)
    agree_n = {"loss": float((loss[0] - wloss[0]).abs() / wloss[0].abs()), "dU": float((dU - wU).norm() / wU.norm()),
               "dV": float((dV - wV).norm() / wV.norm()), "db": float((db - wb).norm() / wb.norm())}
    assert max(agree_n.values()) <= 1e-12, agree_n
    t_pn, t_wn = [], []
    for _ in range(a.repeats):
        t_pn.append(event_us(pixel_n, 10))
        t_wn.append(event_us(wide_n, 10))
    us_pn, us_wn = statistics.median(t_pn), statistics.median(t_wn)
    res.update({"narrow_C": Cn, "narrow_pixel_loss_grad_us": round(us_pn, 1), "narrow_wide_loss_grad_us": round(us_wn, 1),
                "narrow_pixel_over_wide": round(us_pn / us_wn, 2), "narrow_agreement_with_wide": agree_n,
                "narrow_pixel_workspace_bytes": ws.numel() * 8, "narrow_wide_workspace_bytes": wws.numel() * 8})
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
