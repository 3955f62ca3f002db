"""The RRR baseline at one session of ViT-Base embeddings: K = 400 / 100 trials, T = 100, N = 512, C = 768, r = 3,
y float32 (src/train_rrr.py --input_mod vit).

* microseconds per vs_rrr_wide_loss_grad call, with gradients and loss only (device events around `--calls`
  back-to-back calls, median of `--repeats` windows, alternating with the baselines), and the float64 flop rate of
  its two products per bin (2 x 2 K T (C+1) N flops; loss only: one product);
* the same loss and gradients as the float64 torch einsum + autograd closure on the same GPU in the same process
  (the only alternative a user had before); the two are compared on the same inputs first (1e-12);
* two float64 torch.bmm calls of the two per-bin products' shapes ([T, K, C+1] x [T, C+1, N] and
  [T, C+1, K] x [T, K, N]): the library's rate on the same flops;
* the whole 20-closure fit (RRRGD.fit) against the torch closure driving the same L-BFGS, host clock around a
  synchronise; vs_rrr_wide_score on the validation split; vs_gauss_smooth_time (sigma 2) on y against copy_ over
  the same bytes.

Prints one JSON line and writes it to profiles/rrr_wide_bench.json.
Usage: timeout -k 10 900 python scripts/rrr_wide_bench.py [--calls 10] [--repeats 5] [--out PATH]
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

import torch  # noqa: E402

import numpy as np  # noqa: E402

from rrr_bench import DEV, event_us, make_inputs, torch_loss_grad  # noqa: E402


def torch_fit(X, y, r, l2):
    """RRRGD.fit of one session with the torch composition as the closure (same initialisation, same L-BFGS)."""
    K, T, C1 = X.shape
    N = y.shape[2]
    rs = np.random.RandomState(0)
    U = torch.from_numpy(rs.normal(size=(N, C1 - 1, r)) / np.sqrt(T * r)).to(DEV).requires_grad_(True)
    V = torch.from_numpy(rs.normal(size=(r, T)) / np.sqrt(T * r)).to(DEV).requires_grad_(True)
    b = y.mean(0).t().unsqueeze(1).contiguous().requires_grad_(True)
    opt = torch.optim.LBFGS([U, b, V])

    def closure():
        opt.zero_grad()
        beta = torch.cat((U @ V, b), 1)
        loss = ((torch.einsum("ktc,nct->ktn", X, beta) - y) ** 2).sum() + l2 * (beta ** 2).sum()
        loss.backward()
        return loss
    opt.step(closure)
    return opt.state[U]["func_evals"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rrr_wide_bench.json"))
    ap.add_argument("--shape", type=int, nargs=6, default=[400, 100, 100, 512, 768, 3],
                    metavar=("K", "KVAL", "T", "N", "C", "R"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rrr_wide_bench needs a GPU")
    from vspike import _lib as L, ops
    from vspike.rrr import RRRGD
    K, Kv, T, N, C, r = a.shape
    l2 = 100.0
    X, Xv, y, gt, U, V, b = make_inputs(K, Kv, T, N, C, r)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    dU, dV, db = (torch.zeros_like(t) for t in (U, V, b))
    need = ops.rrr_wide_loss_grad_workspace_bytes(K, T, N, C)
    ws = torch.empty(need // 8 + 2, dtype=torch.float64, device=DEV)

    def wide():
        ops.rrr_wide_loss_grad(X, y, U, V, b, l2, loss, dU=dU, dV=dV, db=db, workspace=ws)

    def loss_only():
        ops.rrr_wide_loss_grad(X, y, U, V, b, l2, loss, workspace=ws)

    def composed():
        torch_loss_grad(X, y, U, V, b, l2)

    # the same numbers first
    wide()
    tl, tU, tV, tb = torch_loss_grad(X, y, U, V, b, l2)
    agree = {"loss": float((loss[0] - tl).abs() / tl.abs()), "dU": float((dU - tU).norm() / tU.norm()),
             "dV": float((dV - tV).norm() / tV.norm()), "db": float((db - tb).norm() / tb.norm())}
    assert max(agree.values()) <= 1e-12, agree
    # the library on the same flops: the two per-bin products as batched float64 GEMMs
    A1, B1 = torch.randn(T, K, C + 1, device=DEV, dtype=torch.float64), torch.randn(T, C + 1, N, device=DEV,
                                                                                   dtype=torch.float64)
    A2, B2 = torch.randn(T, C + 1, K, device=DEV, dtype=torch.float64), torch.randn(T, K, N, device=DEV,
                                                                                   dtype=torch.float64)
    O1, O2 = torch.empty(T, K, N, device=DEV, dtype=torch.float64), torch.empty(T, C + 1, N, device=DEV,
                                                                                dtype=torch.float64)

    def bmm2():
        torch.bmm(A1, B1, out=O1)
        torch.bmm(A2, B2, out=O2)
    for fn in (wide, loss_only, composed, bmm2):
        event_us(fn, 3)
    t_w, t_lo, t_c, t_b = [], [], [], []
    for _ in range(a.repeats):                                           # alternating windows
        t_w.append(event_us(wide, a.calls))
        t_lo.append(event_us(loss_only, a.calls))
        t_c.append(event_us(composed, a.calls))
        t_b.append(event_us(bmm2, a.calls))
    us_w, us_lo, us_c, us_b = (statistics.median(t) for t in (t_w, t_lo, t_c, t_b))
    flops = 2 * 2.0 * K * T * (C + 1) * N

    # the score and the smoothing
    bps, r2 = (torch.zeros(N, dtype=torch.float64, device=DEV) for _ in range(2))
    out2 = torch.zeros(2, dtype=torch.float64, device=DEV)
    pred = torch.zeros(Kv, T, N, dtype=torch.float64, device=DEV)
    mean_y = 0.5 + torch.rand(T, N, dtype=torch.float64, device=DEV)
    std_y = 0.5 + torch.rand(T, N, dtype=torch.float64, device=DEV)
    sws = torch.empty(ops.rrr_wide_score_workspace_bytes(Kv, T, N) // 8 + 2, dtype=torch.float64, device=DEV)
    smoothed, ycopy = torch.empty_like(y), torch.empty_like(y)

    def score():
        ops.rrr_wide_score(Xv, U, V, b, mean_y, std_y, gt, bps, r2, out2, pred=pred, workspace=sws)

    def smooth():
        ops.gauss_smooth_time(y, 2, out=smoothed)

    def copy():
        ycopy.copy_(y)
    for fn in (score, smooth, copy):
        event_us(fn, 3)
    us_score = statistics.median(event_us(score, a.calls) for _ in range(a.repeats))
    t_s, t_cp = [], []
    for _ in range(a.repeats):
        t_s.append(event_us(smooth, a.calls))
        t_cp.append(event_us(copy, a.calls))
    us_smooth, us_copy = statistics.median(t_s), statistics.median(t_cp)

    # the whole fit: host clock around a synchronise (L-BFGS reads the loss on the host after every closure)
    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, n

    def fit_wide():
        return RRRGD(r, l2).fit({"s": (X, y)}).func_evals
    wall_ms(fit_wide)
    wall_ms(lambda: torch_fit(X, y, r, l2))
    fit_w, fit_c, evals = [], [], set()
    for _ in range(a.repeats):
        ms, n = wall_ms(fit_wide)
        fit_w.append(ms)
        evals.add(int(n))
        ms, n = wall_ms(lambda: torch_fit(X, y, r, l2))
        fit_c.append(ms)
        evals.add(int(n))
    ms_w, ms_c = statistics.median(fit_w), statistics.median(fit_c)
    res = {
        "bench": "rrr_wide", "arch": torch.cuda.get_device_properties(0).gcnArchName, "build_id": L.build_id(),
        "knobs": L.knobs_nondefault(),
        "shape": {"K_train": K, "K_val": Kv, "T": T, "N": N, "C": C, "r": r, "y": "float32"},
        "workspace_bytes": need,
        "loss_grad_us": round(us_w, 1), "loss_grad_us_windows": [round(t, 1) for t in t_w],
        "loss_grad_f64_tflops": round(flops / us_w * 1e-6, 2),
        "loss_only_us": round(us_lo, 1), "loss_only_f64_tflops": round(0.5 * flops / us_lo * 1e-6, 2),
        "torch_f64_composition_us": round(us_c, 1), "torch_f64_composition_us_windows": [round(t, 1) for t in t_c],
        "speedup_vs_torch_composition": round(us_c / us_w, 2),
        "agreement_with_torch_composition": agree,
        "torch_bmm_f64_two_products_us": round(us_b, 1), "torch_bmm_f64_tflops": round(flops / us_b * 1e-6, 2),
        "loss_grad_over_bmm": round(us_w / us_b, 2),
        "score_us": round(us_score, 1),
        "gauss_smooth_us": round(us_smooth, 1), "copy_same_bytes_us": round(us_copy, 1),
        "gauss_smooth_over_copy": round(us_smooth / us_copy, 2),
        "fit_ms": round(ms_w, 1), "fit_ms_torch_closure": round(ms_c, 1), "fit_func_evals": sorted(evals),
        "fit_kernel_share": round(20 * us_w * 1e-3 / ms_w, 3),
        "calls_per_window": a.calls, "repeats": a.repeats,
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
