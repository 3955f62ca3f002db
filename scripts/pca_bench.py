"""The PCA video embedding at one session of whisker video: M = 60,000 frames of D = 18,260 pixels (500 trials x 120
frames of 110 x 166, config/model/linear_whisker-video.yaml), k = 5, l = 15; uint8 and float32 pixels.

* microseconds per call of vs_pca_colmean, vs_pca_project (L = 15 and L = 5) and vs_pca_gram_apply (L = 15): device
  events around `--calls` back-to-back calls, median of `--repeats` windows, alternating with the yardsticks;
* torch's copy_ over the same bytes of X (the stream yardstick: one read and one write of X, so a kernel that only
  reads X has half its traffic);
* the same two products as torch.matmul in float32 on a centred float32 copy of X (which the kernels never make):
  Y = Xc Q and W = Xc^T Y, the library's rate on the same flops;
* the whole fit (PCA.fit, host clock around a synchronise), its steps, and where the time goes: the kernels (per-call
  times x calls), the float64 QR / eigh / residual plumbing of a step (timed on operands of the fit's shapes) and
  the rest (launches, the stop test's wait on the stream, the host);
* sklearn's PCA(5).fit on the host's CPUs on the float32 matrix, for context (skipped with --no-sklearn).

Prints one JSON line and writes it to profiles/pca_bench.json.
Usage: timeout -k 10 900 python scripts/pca_bench.py [--calls 5] [--repeats 5] [--shape M D] [--out PATH]
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

from rrr_bench import DEV, event_us  # noqa: E402


def make_video(M, D, seed=0):
    """[M, D] uint8 on the device: 8 smooth latents times random maps around a mean image, plus noise."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    t = torch.linspace(0, 1, M, device=DEV).unsqueeze(1)
    lat = torch.sin(2 * torch.pi * (1.0 + 0.7 * torch.arange(8, device=DEV)) * t * 40)        # [M, 8]
    maps = torch.randn(8, D, device=DEV, generator=g)
    gains = torch.tensor([30.0, 20.0, 13.0, 9.0, 6.0, 2.0, 1.5, 1.0], device=DEV)
    out = torch.empty(M, D, dtype=torch.uint8, device=DEV)
    mean = 128.0 + 30.0 * torch.randn(D, device=DEV, generator=g)
    for m0 in range(0, M, 8192):                                                             # bounded scratch
        m1 = min(m0 + 8192, M)
        f = mean + (lat[m0:m1] * gains) @ maps + 8.0 * torch.randn(m1 - m0, D, device=DEV, generator=g)
        out[m0:m1] = f.round().clamp_(0, 255).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", type=int, nargs=2, default=[60000, 18260], metavar=("M", "D"))
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pca_bench needs a GPU")
    from vspike import _lib as L, ops
    from vspike.pca import PCA, linalg_device, start_block
    M, D = a.shape
    k, l = 5, 15
    X8 = make_video(M, D)
    res = {"bench": "pca", "arch": torch.cuda.get_device_properties(0).gcnArchName, "build_id": L.build_id(),
           "knobs": L.knobs_nondefault(), "shape": {"M": M, "D": D, "k": k, "l": l},
           "workspace_bytes": {"colmean": ops.pca_colmean_workspace_bytes(M, D),
                               "project": ops.pca_project_workspace_bytes(M, D, l),
                               "gram_apply": ops.pca_gram_apply_workspace_bytes(M, D, l)},
           "calls_per_window": a.calls, "repeats": a.repeats}
    Q = torch.linalg.qr(start_block(D, l))[0].to(DEV).contiguous()
    Q5 = Q[:, :k].contiguous()
    W = torch.empty(D, l, dtype=torch.float64, device=DEV)
    Y = torch.empty(M, l, dtype=torch.float64, device=DEV)
    Y5 = torch.empty(M, k, dtype=torch.float64, device=DEV)
    ws = torch.empty(ops.pca_gram_apply_workspace_bytes(M, D, l) // 8 + 2, dtype=torch.float64, device=DEV)
    cws = torch.empty(ops.pca_colmean_workspace_bytes(M, D) // 8 + 2, dtype=torch.float64, device=DEV)
    mu = torch.empty(D, dtype=torch.float64, device=DEV)
    for name, X in (("uint8", X8), ("float32", X8.float())):
        nbytes = X.numel() * X.element_size()
        dst = torch.empty_like(X)
        fns = {"colmean": lambda: ops.pca_colmean(X, mu=mu, workspace=cws),
               "project_l15": lambda: ops.pca_project(X, mu, Q, Y=Y, workspace=ws),
               "project_k5": lambda: ops.pca_project(X, mu, Q5, Y=Y5, workspace=ws),
               "gram_apply_l15": lambda: ops.pca_gram_apply(X, mu, Q, W=W, workspace=ws),
               "copy_same_bytes": lambda: dst.copy_(X)}
        if name == "float32":
            # the library on the same flops: needs the centred copy the kernels never make
            ops.pca_colmean(X, mu=mu, workspace=cws)
            Xc = torch.empty_like(X)
            torch.sub(X, mu.float(), out=Xc)
            Qf, Yf, Wf = Q.float(), torch.empty(M, l, device=DEV), torch.empty(D, l, device=DEV)

            def mm2():
                torch.matmul(Xc, Qf, out=Yf)
                torch.matmul(Xc.t(), Yf, out=Wf)
            fns["torch_matmul_f32_two_products"] = mm2
        for fn in fns.values():
            event_us(fn, 2)
        t = {kk: [] for kk in fns}
        for _ in range(a.repeats):                                        # alternating windows
            for kk, fn in fns.items():
                t[kk].append(event_us(fn, a.calls))
        us = {kk: statistics.median(v) for kk, v in t.items()}
        if name == "float32":
            agree = float((Wf.double() - W).norm() / W.norm())
        r = {f"{kk}_us": round(v, 1) for kk, v in us.items()}
        r["X_bytes"] = nbytes
        r["gram_apply_us_windows"] = [round(v, 1) for v in t["gram_apply_l15"]]
        r["gram_apply_read_tb_s"] = round(2 * nbytes / us["gram_apply_l15"] * 1e-6, 3)   # X is read twice
        r["project_read_tb_s"] = round(nbytes / us["project_l15"] * 1e-6, 3)
        r["colmean_read_tb_s"] = round(nbytes / us["colmean"] * 1e-6, 3)
        r["copy_tb_s"] = round(2 * nbytes / us["copy_same_bytes"] * 1e-6, 3)             # read + write
        r["gram_apply_over_copy"] = round(us["gram_apply_l15"] / us["copy_same_bytes"], 2)
        r["gram_apply_f32_tflops"] = round(2 * 2.0 * M * D * 16 / us["gram_apply_l15"] * 1e-6, 1)   # 16 MFMA columns
        if name == "float32":
            r["gram_apply_over_torch_matmul"] = round(us["gram_apply_l15"] / us["torch_matmul_f32_two_products"], 2)
            r["W_against_torch_matmul_rel"] = agree
            del Xc, Qf, Yf, Wf
        # the float64 plumbing of one step on the fit's shapes
        p = PCA(k)
        p._where = linalg_device(X.device)

        def small():
            theta, S = p._eigh_desc(Q.t() @ W)
            Sk = S[:, :k]
            torch.linalg.vector_norm(W @ Sk - (Q @ Sk) * theta[:k], dim=0) / theta[0]
            p._qr(W)
        ops.pca_gram_apply(X, mu, Q, W=W, workspace=ws)
        event_us(small, 2)
        small_us = statistics.median(event_us(small, a.calls) for _ in range(a.repeats))
        # the whole fit
        del dst
        fits, iters = [], set()
        for i in range(a.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = PCA(k).fit(X)
            torch.cuda.synchronize()
            if i:
                fits.append((time.perf_counter() - t0) * 1e3)
            iters.add(p.n_iter_)
        fit_ms, n = statistics.median(fits), max(iters)
        kern_ms = (us["colmean"] + n * us["gram_apply_l15"] + us["project_l15"]) * 1e-3
        small_ms = (n + 2) * small_us * 1e-3
        r.update({"fit_ms": round(fit_ms, 1), "fit_ms_runs": [round(v, 1) for v in fits], "fit_steps": sorted(iters),
                  "fit_converged": bool(p.converged_), "fit_last_residuals": [float(v) for v in p.residuals_],
                  "small_linalg_on": p.timing_["linalg"], "small_linalg_step_us": round(small_us, 1),
                  "fit_share_kernels": round(kern_ms / fit_ms, 3), "fit_share_small_linalg": round(small_ms / fit_ms, 3),
                  "fit_share_rest_sync_launch_host": round(1 - (kern_ms + small_ms) / fit_ms, 3),
                  "fit_host_wait_on_stop_test_ms": round(p.timing_["wait_s"] * 1e3, 1)})
        if name == "float32" and not a.no_sklearn:
            try:
                from sklearn.decomposition import PCA as SkPCA
                host = X.cpu().numpy()
                t0 = time.perf_counter()
                sk = SkPCA(n_components=k).fit(host)
                r["sklearn_fit_s"] = round(time.perf_counter() - t0, 2)
                r["sklearn_solver"] = sk._fit_svd_solver
                r["sklearn_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
                sv = p.singular_values_.cpu().numpy()
                r["singular_values_against_sklearn_rel"] = float(abs(sv - sk.singular_values_).max() / sv[0])
                del host
            except ImportError:
                r["sklearn_fit_s"] = None
        res[name] = r
        del X
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
