"""The reduced-rank regression validation at one session of the workload's size: K = 400 / 100 trials, T = 100,
N = 512, C = 3, r = 3, y float32 (what ContrastTrainer.validate fits after every pass over the data).

* microseconds per vs_rrr_loss_grad call (device events around `--calls` back-to-back calls, median of `--repeats`
  windows, alternating with the baseline), its algorithmic bytes (y + X once) and the rate they give, beside the
  machine's measured 1:1 copy rate (profiles/r03_v7_store_rate.txt: 5.19 TB/s of bytes moved) and
  torch's copy_ over the same number of bytes in this process;
* the baseline: the same loss and gradients as a plain float64 torch composition (U @ V, cat, einsum, autograd)
  run by PyTorch on the same GPU in the same process: what pointing the reference's RRRGD at the device gives;
  the two are compared on the same inputs first (1e-12);
* the whole fit (RRR.fit: one L-BFGS step of 20 closures, each ending in a host synchronisation for
  `float(loss)`), fused and with the torch composition as the closure, host clock around a synchronise;
* vs_rrr_score on the validation split.

Prints one JSON line and writes it to profiles/rrr_bench.json.
Usage: timeout -k 10 600 python scripts/rrr_bench.py [--calls 50] [--repeats 5] [--out PATH]
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
COPY_RATE_TBS = 5.19          # profiles/r03_v7_store_rate.txt, copy 1:1 (bytes read + bytes written)


def make_inputs(K, Kv, T, N, C, r):
    g = torch.Generator(device=DEV).manual_seed(3)
    def X_(k):
        x = torch.randn(k, T, C + 1, device=DEV, dtype=torch.float64, generator=g)
        x[:, :, C] = 1.0
        return x
    X, Xv = X_(K), X_(Kv)
    y = torch.randn(K, T, N, device=DEV, generator=g)
    gt = torch.poisson(torch.full((Kv, T, N), 0.6, device=DEV), generator=g)
    U = torch.randn(N, C, r, device=DEV, dtype=torch.float64, generator=g) / (T * r) ** 0.5
    V = torch.randn(r, T, device=DEV, dtype=torch.float64, generator=g) / (T * r) ** 0.5
    b = 0.1 * torch.randn(N, 1, T, device=DEV, dtype=torch.float64, generator=g)
    return X, Xv, y, gt, U, V, b


def torch_loss_grad(X, y, U, V, b, l2):
    """The reference's closure as torch ops: beta, einsum, residual, both sums, backward."""
    U, V, b = (t.detach().requires_grad_(True) for t in (U, V, b))
    beta = torch.cat((U @ V, b), 1)
    loss = ((torch.einsum("ktc,nct->ktn", X, beta) - y) ** 2).sum() + l2 * (beta ** 2).sum()
    loss.backward()
    return loss.detach(), U.grad, V.grad, b.grad


def event_us(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def torch_fit(X, y, r, l2):
    """RRR.fit with the torch composition as the closure (same initialisation, same L-BFGS)."""
    from vspike.rrr import init_params
    K, T, C1 = X.shape
    N = y.shape[2]
    U0, V0 = init_params(T, N, C1 - 1, r)
    U = torch.from_numpy(U0).to(DEV).requires_grad_(True)
    V = torch.from_numpy(V0).to(DEV).requires_grad_(True)
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
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rrr_bench.json"))
    ap.add_argument("--shape", type=int, nargs=6, default=[400, 100, 100, 512, 3, 3],
                    metavar=("K", "KVAL", "T", "N", "C", "R"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rrr_bench needs a GPU")
    from vspike import _lib as L, ops
    from vspike.rrr import RRR
    K, Kv, T, N, C, r = a.shape
    l2 = 100.0
    X, Xv, y, gt, U, V, b = make_inputs(K, Kv, T, N, C, r)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    dU, dV, db = (torch.zeros_like(t) for t in (U, V, b))
    ws = torch.empty(ops.rrr_loss_grad_workspace_bytes(K, T, N, C) // 8 + 2, dtype=torch.float64, device=DEV)

    def fused():
        ops.rrr_loss_grad(X, y, U, V, b, l2, loss, dU=dU, dV=dV, db=db, workspace=ws)

    def composed():
        torch_loss_grad(X, y, U, V, b, l2)

    # the same numbers first
    fused()
    tl, tU, tV, tb = torch_loss_grad(X, y, U, V, b, l2)
    agree = {"loss": float((loss[0] - tl).abs() / tl.abs()), "dU": float((dU - tU).norm() / tU.norm()),
             "dV": float((dV - tV).norm() / tV.norm()), "db": float((db - tb).norm() / tb.norm())}
    assert max(agree.values()) <= 1e-12, agree
    nbytes = y.numel() * y.element_size() + X.numel() * 8
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=DEV)       # copy_ moving `nbytes` in total
    dst = torch.empty_like(src)
    for fn in (fused, composed, lambda: dst.copy_(src)):                 # warm-up of every timed shape
        event_us(fn, 5)
    t_f, t_c, t_copy = [], [], []
    for _ in range(a.repeats):                                           # alternating windows
        t_f.append(event_us(fused, a.calls))
        t_c.append(event_us(composed, a.calls))
        t_copy.append(event_us(lambda: dst.copy_(src), a.calls))
    us_f, us_c, us_copy = (statistics.median(t) for t in (t_f, t_c, t_copy))

    # loss-only mode and the score
    def loss_only():
        ops.rrr_loss_grad(X, y, U, V, b, l2, loss, workspace=ws)
    bps, r2 = (torch.zeros(N, dtype=torch.float64, device=DEV) for _ in range(2))
    out2 = torch.zeros(2, dtype=torch.float64, device=DEV)
    pred = torch.zeros(Kv, T, N, dtype=torch.float64, device=DEV)
    mean_y = 0.5 + torch.rand(T, N, dtype=torch.float64, device=DEV)
    std_y = 0.5 + torch.rand(T, N, dtype=torch.float64, device=DEV)
    sws = torch.empty(ops.rrr_score_workspace_bytes(Kv, N) // 8 + 2, dtype=torch.float64, device=DEV)

    def score():
        ops.rrr_score(Xv, U, V, b, mean_y, std_y, gt, bps, r2, out2, pred=pred, workspace=sws)
    for fn in (loss_only, score):
        event_us(fn, 5)
    us_lo = statistics.median(event_us(loss_only, a.calls) for _ in range(a.repeats))
    us_score = statistics.median(event_us(score, a.calls) for _ in range(a.repeats))

    # the whole fit: host clock around a synchronise (L-BFGS reads the loss on the host after every closure)
    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, n
    wall_ms(lambda: RRR(r, l2).fit(X, y).func_evals)
    wall_ms(lambda: torch_fit(X, y, r, l2))
    fit_f, fit_c, evals = [], [], set()
    for _ in range(a.repeats):
        ms, n = wall_ms(lambda: RRR(r, l2).fit(X, y).func_evals)
        fit_f.append(ms)
        evals.add(int(n))
        ms, n = wall_ms(lambda: torch_fit(X, y, r, l2))
        fit_c.append(ms)
        evals.add(int(n))
    ms_f, ms_c = statistics.median(fit_f), statistics.median(fit_c)
    arch = torch.cuda.get_device_properties(0).gcnArchName
    res = {
        "bench": "rrr", "arch": arch, "build_id": L.build_id(), "knobs": L.knobs_nondefault(),
        "shape": {"K_train": K, "K_val": Kv, "T": T, "N": N, "C": C, "r": r, "y": "float32"},
        "loss_grad_us": round(us_f, 2), "loss_grad_us_windows": [round(t, 2) for t in t_f],
        "loss_grad_bytes": nbytes, "loss_grad_tbs": round(nbytes / us_f * 1e-6, 3),
        "copy_same_bytes_us": round(us_copy, 2), "loss_grad_over_copy": round(us_f / us_copy, 2),
        "copy_rate_profile_tbs": COPY_RATE_TBS,
        "loss_grad_over_profile_copy": round(us_f / (nbytes / (COPY_RATE_TBS * 1e6)), 2),
        "torch_f64_composition_us": round(us_c, 2), "torch_f64_composition_us_windows": [round(t, 2) for t in t_c],
        "speedup_vs_torch_composition": round(us_c / us_f, 2),
        "agreement_with_torch_composition": agree,
        "loss_only_us": round(us_lo, 2),
        "score_us": round(us_score, 2),
        "fit_ms": round(ms_f, 2), "fit_ms_torch_closure": round(ms_c, 2), "fit_func_evals": sorted(evals),
        "fit_kernel_share": round(20 * us_f * 1e-3 / ms_f, 3),
        "calls_per_window": a.calls, "repeats": a.repeats,
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
