"""Benchmark: clips/sec of the full video->spike TRAIN step (BASELINE config C2 at N=1).

Workload (BASELINE.json configs[1]): ViT-Tiny/16 encoder (d192, 3 heads, 12 layers, tubelet 2)
on 16x224x224 clips (1568 tokens) -> Linear(1568*192 -> 64) -> Linear(64 -> 100*128) log-rates,
PoissonNLL mean, full backward INCLUDING the encoder (freeze_encoder: false), fused AdamW +
OneCycleLR step, bf16 compute / f32 accumulate, synthetic data (random pixels, Poisson spike
targets) resident in HBM.  Batch: the reference's own training config, `train_batch_size: 128`
(config/train/vmae_video.yaml:20 in the reference and in this repo) clips per process — the
reference trains through accelerate, whose prepared DataLoader gives every process a batch of
that size (src/train.py:61-64, split_batches off).  One process per GPU; for N > 1 each rank
trains its own 128 clips and gradients are all-reduced over RCCL (weak scaling).  `--batch 16`
is the configuration rounds 1-2 reported.  `--model vmae_video --neurons 512` runs C3 (ViT-Base,
the reference plugin's own width).

A plain run (`bench.py --gpus 1 --steps N --warmup W`) does only what the headline figure needs:
it sets up, warms up, times the N steps, writes its outputs if `--dump-outputs DIR` is given and
prints the line; `roofline`, `cpu_baseline`, `parity`, `c3` and `c4` are null in it.  `--full` adds
everything else listed below (each part still has its own `--no-*` / `--profile-steps 0` switch).

`--dump-outputs DIR`: what the last timed step handed its caller, as float32 `DIR/<name>.npy`:
`loss` (the step's return value), `losses` (every timed step's) and the trained state the step
updates in place, one file per parameter tensor (`param_<name>`; a tensor past its share of the
64 MB budget is cut to a fixed, seeded sample of its elements, in index order).  Model, clips and
targets are seeded, so the same arguments give the same inputs in every run and build.

Prints ONE JSON line (rank 0):
  * `value` = clips/s over EXACTLY `--steps` train steps, timers off, barrier + synchronize on
    both sides, max over ranks; `ms_per_step` = milliseconds per timed step;
  * the rest needs `--full`:
  * `roofline`: a SEPARATE instrumented pass (`--profile-steps`, after the timed region) brackets
    every launch with hipEvents on its own launch stream (libvspike timers: one per kernel class,
    and one per Linear product of the ViT block — fwd / dX / dW of qkv, proj, fc1, fc2) and sums
    their algorithmic bytes / flops; the dominant entry is the one with the most kernel time per
    step, reported against its bound (HBM bytes for GEMMs, LayerNorm, AdamW; MFMA flops for
    attention), with every entry listed under `all`; `pmc` cross-checks attention with the
    committed rocprofv3 MFMA-busy counters;
  * `cpu_baseline`: the CPU fp32 oracle (oracle/cpu_ref.py, a torch-CPU restatement of the same
    step) on the host cores, per BASELINE.md's plan (median of 5 after a warm-up, fwd and fwd+bwd,
    B=1 and B=4), bounded in time;
  * `parity`: one fwd+bwd of the WHOLE benched batch (the timed step's dispatch) at the initial
    weights against the same oracle (micro-batches of 8 clips whose gradients accumulate into the
    full-batch gradient): log-rates, loss and every gradient.
"""
import argparse
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "video-spike_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3
PEAK_FP8_TFLOPS = 5000.0    # MI355X dense fp8 (block-scaled MFMA), MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0       # HBM3E spec (MI355X_MICROARCH.md); 6.3 TB/s is the measured copy rate
# timer classes whose launches map one-to-one onto kernels that the committed PMC traffic summary
# (scripts/traffic_summary.py) groups; the per-product GEMM timers share kernel templates
TRAFFIC_CLASSES = ("attn_fwd", "attn_bwd", "ln_fwd", "ln_bwd", "adamw")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1,
                    help="ranks (one process per GPU).  Without WORLD_SIZE in the environment, N > 1 starts N "
                         "child ranks under torch.distributed.run before this process touches the GPU")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend of the gradient exchange (nccl = RCCL on ROCm; gloo lets "
                         "several ranks share one GPU, for tests)")
    ap.add_argument("--loss", default="poisson", choices=["poisson", "mse"], help="training.loss")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="beside the timed steps: the instrumented roofline pass, the CPU baseline, the full-batch "
                         "parity check against the CPU oracle and the C3 / C4 sub-records (off: a plain run sets up, "
                         "warms up, times --steps steps and prints the line)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last one computed (its loss, every timed step's loss, "
                         "the updated parameters) to DIR/<name>.npy, float32, at most 64 MB in all")
    ap.add_argument("--profile-steps", type=int, default=10,
                    help="instrumented steps after the timed region (run under --full)")
    ap.add_argument("--batch", type=int, default=None,
                    help="clips per GPU (default: the train config's train_batch_size, 128 = the reference's)")
    ap.add_argument("--neurons", type=int, default=128)
    ap.add_argument("--model", default="vmae_tiny", help="config/model/<name>.yaml")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp8"],
                    help="fp8: BASELINE C5's precision — the ViT block's four Linear forwards on MX-FP8 "
                         "(vs_gemm_mxfp8), the rest bf16")
    ap.add_argument("--frames", type=int, default=None, help="clip length (16 = C2/C3; 32 = C5's encoder)")
    ap.add_argument("--freeze", action="store_true", help="reference default: encoder frozen (head-only training)")
    ap.add_argument("--lr", type=float, default=None,
                    help="override the config's max lr (throughput-neutral).  The synthetic C3 setup (random-init "
                         "ViT-Base, 1.2 M-wide head) diverges at the config's 5e-5 in fp32 and bf16 alike "
                         "(scripts/c3_curve.py), and non-finite scores send attention down its safe-softmax redo")
    ap.add_argument("--cpu-seconds", type=float, default=30.0, help="budget of the CPU-oracle baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-cpu-timing", action="store_true",
                    help="keep the full-batch CPU-oracle parity leg, skip only the timed CPU baseline (big configs)")
    ap.add_argument("--no-c3", action="store_true",
                    help="skip the C3 sub-record (ViT-Base/16 at 128 clips, n = 512) the default C2 run appends")
    ap.add_argument("--c3-batch", type=int, default=None, help="C3 sub-record clips per GPU (default: the train config's 128)")
    ap.add_argument("--c3-steps", type=int, default=10)
    ap.add_argument("--c3-warmup", type=int, default=3)
    ap.add_argument("--c3-profile-steps", type=int, default=2)
    ap.add_argument("--c3-check-clips", type=int, default=8,
                    help="C3 check: clips of the benched batch whose loss is back-propagated and checked (0: none)")
    ap.add_argument("--c3-b16-steps", type=int, default=20, help="timed steps of the C3 16-clips/GPU point (0: skip)")
    ap.add_argument("--no-c4", action="store_true",
                    help="skip the C4 sub-record (R3D-18, 32x112x112 clips, n = 256, fp32) the default C2 run appends")
    ap.add_argument("--c4-batch", type=int, default=16, help="C4 sub-record clips per GPU")
    ap.add_argument("--c4-steps", type=int, default=10)
    ap.add_argument("--c4-warmup", type=int, default=2)
    ap.add_argument("--c4-profile-steps", type=int, default=2)
    ap.add_argument("--graph", action="store_true",
                    help="time the step as a hipGraph replay (vspike.graph.GraphedStep; N=1 only).  Off by default: "
                         "on MI355X the replay measured 6.20 vs 5.62 ms/step eager (DESIGN.md section 7)")
    return ap.parse_args()


def _progress(msg):
    """Heartbeat on stderr (the JSON line stays the only stdout line): long CPU phases (baseline,
    full-batch parity) print every few seconds so a supervisor can tell them from a hang."""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def _cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _cpu_share():
    """CPUs this process may actually use: the scheduler affinity, capped by a cgroup v2 cpu.max quota
    (the GPU box gives a job a 16-CPU share of a 256-CPU host: os.cpu_count() counts the host)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def _pin_threads(n):
    """Pin this process to n CPUs of its affinity set (the oracle's OpenMP pool then stays on the
    same cores for every cell); returns the previous set, or None where affinity is unavailable."""
    if not hasattr(os, "sched_getaffinity"):
        return None
    old = os.sched_getaffinity(0)
    try:
        os.sched_setaffinity(0, sorted(old)[:max(1, n)])
    except OSError:
        return None
    return old


def cpu_baseline(cfg, params, pixels, target, seconds, reps=10):
    """BASELINE.md CPU plan (BASELINE.md:37): the oracle (torch-CPU fp32 restatement of the step) per
    clip, fwd and fwd+bwd at B=1 and B=4.  Round 4's harness ran each cell's 5 repetitions back to
    back and left B=1 fwd+bwd FASTER than B=1 fwd (cells measured minutes apart under different
    host load / clock).  Now: the process is pinned to its CPU share (one core per OpenMP thread),
    every cell gets two warm-ups (allocator growth, first-touch page faults, oneDNN primitive
    creation), then `reps` ROUNDS each run all four cells once in a rotating order, so every cell
    sees the same host conditions; a cell's value is the median over the rounds.  Thread counts:
    the CPU share (affinity / cgroup quota; OMP_NUM_THREADS on the box) and os.cpu_count() as
    BASELINE.md asks; the latter is skipped when one B=1 forward at that count takes more than 4x
    the share's (oversubscription: the box's 256-CPU count vs its 16-CPU quota), and recorded so.
    `value` is the best fwd+bwd rate per clip over the cells (thread count x batch 1 / 4: VERDICT r5
    item 8); cells report median, min and max and are checked for monotonicity (fwd+bwd dearer than
    fwd at each batch)."""
    from oracle import cpu_ref
    share = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or _cpu_share()
    counts = [share] + ([os.cpu_count()] if (os.cpu_count() or 0) != share else [])
    P = cpu_ref.to_torch(params)
    t_start = time.perf_counter()
    per_count, loss4, skipped = {}, None, {}
    cells = [(1, "fwd"), (1, "fwd_bwd"), (4, "fwd"), (4, "fwd_bwd")]
    for threads in counts:
        torch.set_num_threads(threads)
        old_aff = _pin_threads(threads) if threads == share else None
        res = {}

        def cell(B, mode):
            px, y = pixels[:B], target[:B]

            def run():
                if mode == "fwd":
                    with torch.no_grad():
                        return cpu_ref.poisson_nll_mean(cpu_ref.videomae_plugin_forward(px, P, cfg, False), y)
                loss = cpu_ref.poisson_nll_mean(cpu_ref.videomae_plugin_forward(px, P, cfg, False), y)
                loss.backward()
                for p in P.values():
                    p.grad = None
                return loss.detach()
            return run
        if threads != share and threads > 4 * share:
            # the GPU box: os.cpu_count() counts the 256-CPU host, the job's quota is 16 CPUs; a probe
            # forward at 256 threads took 42 s there (r05) — recorded as skipped without running it
            skipped[str(threads)] = (f"os.cpu_count() = {threads} threads on a {share}-CPU share: oversubscribed "
                                     "(the process's CPU quota is smaller than the host's count), not run")
            continue
        if threads != share:   # probe: one B=1 forward against the share's median
            t0 = time.perf_counter()
            cell(1, "fwd")()
            probe = time.perf_counter() - t0
            _progress(f"cpu baseline, {threads} threads: probe B=1 fwd {probe:.2f} s")
            if probe > 4 * per_count[str(share)]["B1_fwd"]["max"] or time.perf_counter() - t_start > seconds:
                skipped[str(threads)] = (f"one B=1 forward took {probe:.2f} s against "
                                         f"{per_count[str(share)]['B1_fwd']['s_per_clip']:.2f} s on {share} threads "
                                         "(oversubscribed: the process's CPU quota is smaller than the host's count)")
                continue
        runs = {c: cell(*c) for c in cells}
        for c in cells:                                              # warm-ups
            for _ in range(2):
                loss = runs[c]()
            if c == (4, "fwd"):
                loss4 = float(loss)
        ts = {c: [] for c in cells}
        for r in range(reps):                                        # interleaved rounds
            order = cells[r % len(cells):] + cells[:r % len(cells)]
            for c in order:
                t0 = time.perf_counter()
                runs[c]()
                ts[c].append((time.perf_counter() - t0) / c[0])
            if (r + 1) % 2 == 0:
                _progress(f"cpu baseline, {threads} threads: round {r + 1}/{reps}")
        for (B, mode), t in ts.items():
            res[f"B{B}_{mode}"] = {"s_per_clip": round(statistics.median(t), 4), "min": round(min(t), 4),
                                   "max": round(max(t), 4), "runs": len(t)}
            _progress(f"cpu baseline, {threads} threads, B={B} {mode}: {res[f'B{B}_{mode}']}")
        if old_aff is not None:
            os.sched_setaffinity(0, old_aff)
        c = lambda k: res[k]["s_per_clip"]  # noqa: E731
        # fwd+bwd must cost more than fwd at each batch (the per-clip cost across batches is the CPU's
        # own batching effect: on the box B=4 runs the forward cheaper per clip and the backward dearer
        # per clip than B=1 — the eager attention's B*H*N^2 probabilities leave the caches)
        res["fwd_bwd_over_fwd"] = {"B1": round(c("B1_fwd_bwd") / c("B1_fwd"), 2), "B4": round(c("B4_fwd_bwd") / c("B4_fwd"), 2)}
        res["monotone"] = bool(c("B1_fwd_bwd") > c("B1_fwd") and c("B4_fwd_bwd") > c("B4_fwd"))
        per_count[str(threads)] = res
    torch.set_num_threads(share)           # the rest of the run (parity oracle) on the process's share
    elapsed = time.perf_counter() - t_start
    # `value`: the CPU's best per-clip training rate over the measured cells (thread count x batch).  The
    # B = 4 backward is the dearer one per clip on the box: autograd keeps every layer's B x H x N^2 f32
    # attention probabilities (118 MB per layer at B = 4, 1.4 GB over 12 layers, vs 29 MB at B = 1) and
    # the backward's softmax' / matmul reads of them run from DRAM instead of the caches
    # (scripts/cpu_baseline_profile.py), so B = 1 is the fair CPU rate there
    best, best_b = min(((k, b) for k in per_count for b in (1, 4)),
                       key=lambda kb: per_count[kb[0]][f"B{kb[1]}_fwd_bwd"]["s_per_clip"])
    value = 1.0 / per_count[best][f"B{best_b}_fwd_bwd"]["s_per_clip"]
    out = {"value": round(value, 4), "unit": "clips/sec", "cores": int(best), "kind": "port",
           "sample": f"oracle/cpu_ref.py torch-CPU fp32 train fwd+bwd, the faster per clip of batch 1 and 4 (batch "
                     f"{best_b}), median of {reps} interleaved rounds (all four cells per round) after 2 warm-ups per "
                     f"cell, {best} threads pinned to {best} cores; {elapsed:.1f} s of CPU work in all",
           "batch": best_b,
           "host": {"cpu_model": _cpu_model_name(), "nproc": os.cpu_count(), "cpu_share": _cpu_share(),
                    "omp_num_threads": os.environ.get("OMP_NUM_THREADS")},
           "detail": per_count, "skipped": skipped}
    return out, loss4


def _reference_grads(model):
    """Gradients of the plugin under the reference's parameter names (numpy, f32)."""
    from vspike.layout import modern_name
    out = {}
    for name, which, slot, rows in model.layout.hf_items():
        flat = model.enc_flat.grad if which == "enc" else model.head_flat.grad
        if flat is None:
            continue
        t = (model.layout.enc if which == "enc" else model.layout.head).view(flat, slot)
        out[modern_name(name)] = (t if rows is None else t[rows]).detach().float().cpu().numpy()
    return out


# bf16 bars of the full-batch check: about 2x the worst values measured at the bench geometry
# (r03 on MI355X at 128 clips: log-rates 3.4e-3, loss 1.8e-5, worst gradient 4.6e-3); a failed check
# makes bench.py exit non-zero after printing its line
PARITY_TOL = {"fp32": {"log_rates": 1e-4, "loss": 1e-5, "grad": 1e-3},
              "bf16": {"log_rates": 7e-3, "loss": 1e-4, "grad": 1e-2},
              # MX-FP8 forward products (3 mantissa bits): oracle/tolerances.py, the bars tests/test_gpu_c5.py
              # uses too (filled in by full_batch_parity, which imports the oracle package)
              "fp8": None}


def full_batch_parity(ccfg, params, pixels, target, gpu, args, what=None):
    """The benched step's fwd+bwd (whole batch, initial weights) vs the CPU fp32 oracle on the same
    clips: log-rates (max abs error / max |ref|), loss (relative) and every gradient (norm-relative)."""
    import numpy as np
    from oracle import cpu_ref
    t0 = time.perf_counter()
    P = cpu_ref.to_torch(params)
    loss_fn = cpu_ref.poisson_nll_mean if args.loss == "poisson" else (lambda x, y: ((x - y) ** 2).mean())
    # micro-batches of 8 clips (eager attention keeps every layer's N x N probabilities: a whole
    # 128-clip batch would hold ~100 GB; one clip at a time past ViT-Tiny's 1,568 x 192, where a clip
    # takes tens of CPU seconds): each micro-batch's mean loss weighted by its share of the batch, so
    # the accumulated .grad is the full-batch gradient and the summed loss the full mean.  The fp8
    # model is checked against the same oracle with the MX-FP8 round trip on the four block
    # products' operands (cpu_ref.mx_matmul), at the MX bars
    mb = 8 if ccfg.num_tokens * ccfg.hidden_size <= 1568 * 384 else 1
    mm = cpu_ref.mx_matmul if args.dtype == "fp8" else None
    B, outs, loss = pixels.shape[0], [], 0.0
    for i in range(0, B, mb):
        ref = cpu_ref.videomae_plugin_forward(pixels[i:i + mb], P, ccfg, False, mm=mm)
        part = loss_fn(ref, target[i:i + mb]) * (ref.shape[0] / B)
        part.backward()
        loss += float(part)
        outs.append(ref.detach())
        _progress(f"parity: CPU oracle clips {i}..{min(i + mb, B) - 1} of {B}")
    plain = None
    if mm is not None:   # the same clips through the plain fp32 oracle (log-rates only): the distance the
        with torch.no_grad():   # MX-aware reference removes
            P0 = {k: v.detach() for k, v in P.items()}
            po = torch.cat([cpu_ref.videomae_plugin_forward(pixels[i:i + mb], P0, ccfg, False)
                            for i in range(0, B, mb)]).numpy()
        plain = float(np.abs(gpu["log_rates"].numpy() - po).max() / max(np.abs(po).max(), 1e-30))
        _progress(f"parity: plain fp32 oracle log-rates {plain:.3e}")
    secs = time.perf_counter() - t0
    ref_out = torch.cat(outs).numpy()
    e_out = float(np.abs(gpu["log_rates"].numpy() - ref_out).max() / max(np.abs(ref_out).max(), 1e-30))
    e_loss = abs(gpu["loss"] - loss) / abs(loss)
    errs = {}
    for k, g in gpu["grads"].items():
        r = P[k].grad
        if r is None:
            continue
        r = r.detach().numpy().reshape(g.shape)
        errs[k] = float(np.linalg.norm((g - r).ravel()) / max(np.linalg.norm(r.ravel()), 1e-30))
    worst = max(errs, key=errs.get) if errs else None
    tol = getattr(args, "tol", None) or PARITY_TOL[args.dtype]
    if tol is None:   # fp8: the MX-aware reference's bars at the bench geometry (oracle/tolerances.py)
        from oracle.tolerances import FP8_MX12_GRAD, FP8_MX12_LOSS, FP8_MX12_OUT
        tol = {"log_rates": FP8_MX12_OUT, "loss": FP8_MX12_LOSS, "grad": FP8_MX12_GRAD}
    ok = e_out < tol["log_rates"] and e_loss < tol["loss"] and (not errs or errs[worst] < tol["grad"])
    return {"what": (what or f"one fwd+bwd of the whole benched batch ({pixels.shape[0]} clips, the timed step's "
                             "dispatch) at the initial weights") + ": HIP path vs the CPU fp32 oracle (oracle/cpu_ref.py" +
                    (", the four block products on MX-FP8 round trips: cpu_ref.mx_matmul)" if mm else ")"),
            "log_rates_maxrel": round(e_out, 7), "loss_rel": round(e_loss, 8), "n_grads": len(errs),
            "worst_grad": worst, "worst_grad_rel": round(errs[worst], 6) if worst else None,
            "tolerance": tol, "ok": bool(ok), "cpu_seconds": round(secs, 1),
            **({"plain_fp32_log_rates_maxrel": round(plain, 7)} if plain is not None else {})}


def _traffic_lookup(kind, launches_per_step):
    """HBM bytes per timed call of a kernel class from the newest committed PMC summary
    (scripts/pmc_traffic.sh: separate FETCH_SIZE / WRITE_SIZE passes, FETCH doubled per the gfx950
    correction), with the file it came from; None when no summary covers that class."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_traffic.json")))
    for f in reversed(files):
        try:
            d = json.load(open(f))
            op = d["ops"][kind]
            if "bytes_per_step" in op:
                return round(op["bytes_per_step"] / launches_per_step, 0), os.path.relpath(f, ROOT)
            return round(op["traffic_bytes"], 0), os.path.relpath(f, ROOT)
        except (KeyError, ValueError, OSError):
            continue
    return None, None


def _pmc_lookup(kind):
    """MFMA-busy fraction of an attention kernel from the newest committed PMC summary
    (scripts/pmc_attn.sh passes -> scripts/pmc_json.py: SQ_VALU_MFMA_BUSY_CYCLES over 1024 SIMDs x
    GRBM_GUI_ACTIVE / 8), the executed-MFMA cross-check of the hipEvent roofline."""
    kern = {"attn_fwd": ("attn_fwd_bf16_kernel",),
            "attn_bwd": ("attn_bwd_bf16_pp_kernel", "attn_bwd_bf16_kernel")}.get(kind)
    if kern is None:
        return None
    clock = None   # effective clock under the kernel (scripts/attn_clock.py: GRBM cycles / duration)
    for f in reversed(sorted(glob.glob(os.path.join(ROOT, "profiles", "*_attn_clock.json")))):
        try:
            for name, e in json.load(open(f))["kernels"].items():
                if any(k in name for k in kern):
                    clock = {"clock_ghz": e["clock_ghz"], "clock_source": os.path.relpath(f, ROOT)}
                    break
        except (KeyError, ValueError, OSError):
            continue
        if clock:
            break
    for f in reversed(sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_attn.json")))):
        try:
            d = json.load(open(f))
            for name, e in d["kernels"].items():
                if any(k in name for k in kern) and "mfma_busy_frac" in e:
                    return {**(clock or {}), "mfma_busy_frac": round(e["mfma_busy_frac"], 4), "source": os.path.relpath(f, ROOT),
                            "note": "executed MFMA cycles (the backward's dQ pass recomputes S and dP: 7 products "
                                    "executed for the 5 credited)" if kind == "attn_bwd" else "executed MFMA cycles "
                                    "(incl. the row-sum MFMAs)"}
        except (KeyError, ValueError, OSError):
            continue
    return None


def launch_ranks(args) -> int:
    """`bench.py --gpus N` started without a launcher: run N ranks of this script under
    torch.distributed.run (one process per GPU, 127.0.0.1 rendezvous) as CHILD processes and return
    their exit code.  Called before anything initialises the GPU in this process (no re-exec)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "16")
    return subprocess.call(cmd, env=env)


def _param_digest(model, dev):
    """Per-rank fingerprint of the trainable state after the steps (f64 sums of every flat buffer
    and of its squares): replicas that stayed in sync agree exactly."""
    vals = []
    for p in model.parameters():
        d = p.detach().double()
        vals += [d.sum(), (d * d).sum()]
    return torch.stack(vals).to(dev)


def _setup(spec, dev, rank):
    """Model, config, criterion and the synthetic batch of one workload (spec: model, neurons, dtype,
    frames, freeze, lr, loss, batch)."""
    from vspike import load_run_config, make_criterion
    cfg_dir = os.path.join(ROOT, "video-spike_amd", "config")
    config = load_run_config(os.path.join(cfg_dir, "model", spec["model"] + ".yaml"),
                             os.path.join(cfg_dir, "train", "vmae_video.yaml"))
    config["model"]["decoder"]["output_dim"] = 100 * spec["neurons"]       # src/train.py:41
    config["model"]["compute_dtype"] = spec["dtype"]
    if spec.get("frames"):
        bbk = dict(config["model"].get("backbone") or {})
        bbk["num_frames"] = spec["frames"]
        config["model"]["backbone"] = bbk
    config["model"]["freeze_encoder"] = bool(spec["freeze"])
    if spec.get("lr") is not None:
        config["optimizer"]["lr"] = spec["lr"]
    config["training"]["loss"] = spec["loss"]
    criterion = make_criterion(config)
    torch.manual_seed(1234)                      # identical replicas (GradExchange also broadcasts)
    from vspike import NAME2MODEL
    model = NAME2MODEL[config["model"]["model_class"]](config["model"]).to(dev)
    bb = model.backbone
    B = spec["batch"] if spec.get("batch") else int(config["training"]["train_batch_size"])
    g = torch.Generator(device=dev).manual_seed(100 + rank)             # each rank its own clips
    pixels = torch.randn(B, bb.num_frames, bb.num_channels, bb.image_size, bb.image_size, device=dev, generator=g)
    lam = torch.exp(torch.randn(B, 100, spec["neurons"], device=dev, generator=g) - 2.0).clamp(0.01, 5.0)
    target = torch.poisson(lam, generator=g)
    return config, criterion, model, B, pixels, target


def _barrier_sync(world):
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()


DUMP_BUDGET_BYTES = 56 << 20     # of float32 parameter samples; with the losses well under 64 MB in all


def _dump_outputs(dump_dir, losses, model):
    """`--dump-outputs`: what the last timed step handed its caller, as float32 .npy files: the loss it
    returned (`loss`), every timed step's (`losses`), and the parameters it updated in place
    (`param_<name>`, flat).  A tensor larger than its equal share of the budget is cut to a fixed
    sample: indices drawn once from a CPU generator seeded with 0 (the same in every run and build),
    sorted, so two dumps compare element by element."""
    import numpy as np
    os.makedirs(dump_dir, exist_ok=True)
    ls = torch.stack([x.detach().float().reshape(()) for x in losses]).cpu().numpy().astype(np.float32)
    np.save(os.path.join(dump_dir, "loss.npy"), ls[-1:])
    np.save(os.path.join(dump_dir, "losses.npy"), ls)
    params = list(model.named_parameters())
    share = max(1, DUMP_BUDGET_BYTES // 4 // max(1, len(params)))
    for name, p in params:
        flat = p.detach().reshape(-1)
        if flat.numel() > share:
            gen = torch.Generator().manual_seed(0)
            idx = torch.randint(0, flat.numel(), (share,), generator=gen).sort().values
            flat = flat[idx.to(flat.device)]
        np.save(os.path.join(dump_dir, "param_" + name.replace(".", "_") + ".npy"),
                flat.float().cpu().numpy().astype(np.float32))


def _train_and_time(model, config, criterion, pixels, target, world, rank, dev, steps, warmup, profile_steps,
                    graph=False, tag="", instrument=True, dump_dir=None):
    """W warm-up steps, EXACTLY `steps` timed steps between barrier + synchronize (max over ranks),
    then the instrumented pass (per-kernel hipEvent timers, dW products in order).  `instrument`
    off skips that pass; the learning-rate schedule still spans `profile_steps`, so the timed steps
    compute the same either way.  `dump_dir`: rank 0 writes the last timed step's outputs there."""
    from vspike import ops
    from vspike import _lib as L
    from vspike.dp import GradExchange
    from vspike.trainer import build_optimizer, Trainer
    total = warmup + steps + profile_steps + (1 if profile_steps > 0 else 0)  # + the pass's re-warm step
    opt, sched = build_optimizer(model, config, total_steps=total, world=world)
    exchange = GradExchange(model) if world > 1 else None
    trainer = Trainer(model, opt, sched, criterion=criterion, exchange=exchange)
    for _ in range(warmup):
        trainer.step(pixels, target)
    _barrier_sync(world)
    if rank == 0:
        _progress(f"{tag}warm-up done ({warmup} steps); timing {steps} steps")
    L.dispatch_reset()
    step_fn = trainer.step
    if graph:
        if world > 1:
            raise SystemExit("bench.py --graph: the data-parallel exchange is not captured (N=1 only)")
        from vspike.graph import GraphedStep
        graphed = GraphedStep(trainer, pixels, target)     # the capture counts one step's dispatch
        step_fn = graphed.step
        _barrier_sync(world)
    L.attn_redo_count(reset=True)            # (synchronising: before the clock starts)
    t0 = time.perf_counter()
    losses = []
    for _ in range(steps):
        losses.append(step_fn(pixels, target))
    _barrier_sync(world)
    elapsed = time.perf_counter() - t0
    redo = L.attn_redo_count(reset=True) / (1 if graph else steps)
    if world > 1:
        t = torch.tensor([elapsed], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    final_loss = float(losses[-1].item())
    dispatch = {k: round(v / (1 if graph else steps), 2) for k, v in L.dispatch_counts().items() if v}
    replicas_equal = None
    if world > 1:   # every rank ends with the same weights (the exchange kept the replicas in sync)
        hi = _param_digest(model, dev)
        lo = -hi
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)       # max and min over ranks agree iff all equal
        dist.all_reduce(lo, op=dist.ReduceOp.MAX)
        replicas_equal = bool(torch.equal(hi, -lo))
    if dump_dir and rank == 0:
        _dump_outputs(dump_dir, losses, model)

    # ---- instrumented pass (not part of `value`): every kernel class timed on its own stream
    kern = {}
    if instrument and profile_steps > 0:
        # side stream off for this pass: a weight-gradient product overlapped with the main stream's
        # kernels is timed from its launch to its end, including the time it waits for CUs that an
        # attention launch holds (2-3x its own duration); in order, every launch is timed alone
        serial = hasattr(model, "set_side_stream")
        if serial:
            model.set_side_stream(False)
        trainer.step(pixels, target)
        _barrier_sync(world)
        ops.timing_enable((1 << len(L.TIMER_NAMES)) - 1)
        for _ in range(profile_steps):
            trainer.step(pixels, target)
        _barrier_sync(world)
        for tid, name in enumerate(L.TIMER_NAMES):
            kern[name] = ops.timing_collect(tid, with_bytes=True)
        ops.timing_enable(0)
        if serial:
            model.set_side_stream(True)
    return {"elapsed": elapsed, "final_loss": final_loss, "dispatch": dispatch, "replicas_equal": replicas_equal,
            "kern": kern, "trainer": trainer, "attn_redo_per_step": redo}


def _roofline(kern, profile_steps, bb, B, dtype):
    """Per-kernel-class entries against their bounds, and the dominant one (most kernel time per step)."""
    N, H, Lyr = bb.num_tokens, bb.num_attention_heads, bb.num_hidden_layers
    D0, F0 = bb.hidden_size, bb.intermediate_size
    fwd_flop = 4.0 * B * H * N * N * 64                 # QK^T + PV per launch (one layer)
    peak_mfma = PEAK_F32_TFLOPS if dtype == "fp32" else PEAK_BF16_TFLOPS   # fp8: attention + backward are bf16
    roof_all = {}
    for name, (n, ms, nbytes) in kern.items():
        if not n:
            continue
        per_step = n / profile_steps
        avg_s = ms / n / 1e3
        if name in ("attn_fwd", "attn_bwd"):
            work = fwd_flop if name == "attn_fwd" else 2.5 * fwd_flop      # BASELINE.md convention
            ach = work / avg_s / 1e12
            ent = {"bound": "mfma", "unit": "TFLOP/s", "achieved": round(ach, 2), "peak": peak_mfma,
                   "frac": round(ach / peak_mfma, 4), "work_per_launch": work}
        else:
            ach = nbytes / (ms / 1e3) / 1e9                                 # bytes-weighted over launches
            ent = {"bound": "hbm", "unit": "GB/s", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS,
                   "frac": round(ach / PEAK_HBM_GBS, 4), "work_per_launch": round(nbytes / n, 0)}
            prod = {"fwd_qkv": 3 * D0 * D0, "fwd_proj": D0 * D0, "fwd_fc1": F0 * D0, "fwd_fc2": D0 * F0,
                    "dx_qkv": 3 * D0 * D0, "dx_proj": D0 * D0, "dx_fc1": F0 * D0, "dx_fc2": D0 * F0,
                    "dw_qkv": 3 * D0 * D0, "dw_proj": D0 * D0, "dw_fc1": F0 * D0, "dw_fc2": D0 * F0}.get(name)
            if prod is not None:
                # the product's MFMA side (2 M N K flop per launch) against the peak of its dtype (the fp8
                # forward products: the 5 PF MX-FP8 peak)
                fl = 2.0 * B * N * prod
                pk = PEAK_FP8_TFLOPS if (dtype == "fp8" and name.startswith("fwd_")) else peak_mfma
                tf = fl * Lyr / (ms / profile_steps / 1e3) / 1e12   # one product per layer per step
                ent.update({"mfma_flop_per_launch": fl, "mfma_tflops": round(tf, 2), "mfma_peak": pk,
                            "mfma_frac": round(tf / pk, 4)})
            if name in ("fwd_mlp", "dx_mlp"):
                # the fused MLP kernels sit near the ridge (~300 flop/B): their MFMA side as well
                # (fwd: h2 W1^T and a W2^T; dx: h2 W1^T recomputed and dy W2 = 4 M D F flop per launch)
                fl = 4.0 * B * N * D0 * F0
                tf = fl * Lyr / (ms / profile_steps / 1e3) / 1e12
                ent.update({"mfma_flop_per_launch": fl, "mfma_tflops": round(tf, 2),
                            "mfma_frac": round(tf / peak_mfma, 4)})
        ent.update({"ms_per_step": round(ms / profile_steps, 4), "launches_per_step": round(per_step, 2),
                    "avg_launch_us": round(1e3 * ms / n, 2)})
        roof_all[name] = ent
    if not roof_all:
        return roof_all, None
    dom = max(roof_all, key=lambda k: roof_all[k]["ms_per_step"])
    r = roof_all[dom]
    traffic, tsrc = _traffic_lookup(dom, r["launches_per_step"]) if dom in TRAFFIC_CLASSES else (None, None)
    roofline = {"bound": r["bound"], "kernel": dom, "achieved": r["achieved"], "peak": r["peak"], "unit": r["unit"],
                "frac": r["frac"], "traffic": traffic, "traffic_source": tsrc,
                "avg_launch_ms": round(r["avg_launch_us"] / 1e3, 4), "work_per_launch": r["work_per_launch"],
                "timing": f"hipEvents per launch on the launch stream, {profile_steps} instrumented steps "
                          "(weight-gradient products in order on the main stream: each launch timed alone)",
                "pmc": _pmc_lookup(dom), "all": roof_all}
    return roof_all, roofline


def _train_flops_per_clip(bb, neurons):
    """Algorithmic train FLOPs per clip (BASELINE.md convention: train = 3 x forward)."""
    N, Lyr, D, F, K = bb.num_tokens, bb.num_hidden_layers, bb.hidden_size, bb.intermediate_size, bb.patch_dim
    fwd_clip = Lyr * (2 * N * D * 3 * D + 2 * N * D * D + 4 * N * D * F + 4 * N * N * D) + 2 * N * K * D \
        + 2 * N * D * 64 + 2 * 64 * 100 * neurons
    return 3.0 * fwd_clip


def _oracle_cfg(bb):
    from oracle import cpu_ref
    return cpu_ref.ViTCfg(**{k: getattr(bb, k) for k in ("image_size", "patch_size", "num_channels", "num_frames",
                                                         "tubelet_size", "hidden_size", "num_hidden_layers",
                                                         "num_attention_heads", "intermediate_size",
                                                         "layer_norm_eps")})


# bars of the C3 sub-record's check (bf16, ViT-Base: 12 layers of d = 768, 8 clips' gradients through the
# 128-clip dispatch): about 2x the values measured on MI355X in r06 (log-rates 5.3e-3, loss 7.7e-5, worst of
# 186 gradients 8.7e-3, encoder layer 9's key weight); C2's bars at 128 clips of ViT-Tiny are 7e-3 / 1e-4 / 1e-2
C3_CHECK_TOL = {"log_rates": 1e-2, "loss": 2e-4, "grad": 2e-2}


def c3_subrecord(args, world, rank, dev):
    """BASELINE C3 in the same run: ViT-Base/16 (the reference plugin's own width,
    /root/reference/src/model/videomae.py:7,13) at the reference's 128 clips per process
    (config/train/vmae_video.yaml:20), n = 512, encoder trainable, bf16: timed steps at the benched
    dispatch; a fwd + bwd check against the CPU oracle: the whole 128-clip batch
    runs forward and backward through the benched dispatch with the loss taken over its first
    `--c3-check-clips` clips (the backward then carries those clips' gradient through every benched
    kernel, zeros elsewhere), and the oracle runs those clips one at a time: log-rates, loss and EVERY
    gradient at C2's bf16 bars; and the DP=8 per-GPU point (global 128 = 16 clips
    per GPU) as `b16`.  lr 5e-8: the synthetic C3 setup diverges at the config's 5e-5 (DESIGN.md section
    1), which the throughput does not depend on."""
    spec = {"model": "vmae_video", "neurons": 512, "dtype": "bf16", "frames": None, "freeze": False,
            "lr": 5e-8, "loss": "poisson", "batch": args.c3_batch}
    config, criterion, model, B, pixels, target = _setup(spec, dev, rank)
    bb = model.backbone
    check = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline and args.c3_check_clips > 0:
        nchk = min(args.c3_check_clips, B)
        init = {k: v.detach().cpu().numpy() for k, v in model.reference_state_dict(modern_names=True).items()}
        out0 = model(pixels)
        loss0 = criterion(out0[:nchk], target[:nchk])
        loss0.backward()
        gpu = {"loss": float(loss0), "log_rates": out0[:nchk].detach().float().cpu(), "grads": _reference_grads(model)}
        model.zero_grad(set_to_none=True)
        del out0, loss0
        chk_args = argparse.Namespace(dtype="bf16", loss="poisson", tol=C3_CHECK_TOL)
        check = full_batch_parity(_oracle_cfg(bb), init, pixels[:nchk].cpu(), target[:nchk].cpu(), gpu, chk_args,
                                  what=f"fwd of the whole benched {B}-clip batch and bwd of the Poisson loss over its first "
                                       f"{nchk} clips, at the benched dispatch and the initial weights (every gradient)")
        del init, gpu
        _progress(f"C3 check: {check}")
    run = _train_and_time(model, config, criterion, pixels, target, world, rank, dev, args.c3_steps, args.c3_warmup,
                          args.c3_profile_steps, tag="C3: ")
    roof_all, roofline = _roofline(run["kern"], args.c3_profile_steps, bb, B, "bf16")
    clips = world * B * args.c3_steps
    out = {"metric": "clips/sec (16-frame 224x224) train step", "value": round(clips / run["elapsed"], 3),
           "unit": "clips/sec", "n_gpus": world, "steps": args.c3_steps, "warmup": args.c3_warmup,
           "ms_per_step": round(1e3 * run["elapsed"] / args.c3_steps, 3), "dtype": "bf16",
           "config": {"workload": f"C3 ViT-Base/16 {bb.num_frames}x{bb.image_size}x{bb.image_size} -> 512 neurons, "
                                  "encoder+head fwd+bwd+AdamW", "model": "vmae_video", "global_batch": B * world,
                      "clips_per_gpu": B, "seq_len": bb.num_tokens, "parallelism": f"dp{world}", "lr": 5e-8},
           "model_tflops": round(_train_flops_per_clip(bb, 512) * clips / run["elapsed"] / 1e12, 2),
           "check": check, "final_loss": round(run["final_loss"], 6), "replicas_equal": run["replicas_equal"],
           "dispatch_per_step": run["dispatch"],
           "products": {k: {f: v[f] for f in ("ms_per_step", "avg_launch_us", "mfma_frac") if f in v}
                        for k, v in roof_all.items()},
           "roofline": {k: roofline[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac",
                                                 "avg_launch_ms")} if roofline else None}
    out["mfma_util_pct"] = round(100.0 * out["model_tflops"] / PEAK_BF16_TFLOPS, 2)
    del run, model, pixels, target
    if args.c3_b16_steps > 0:
        # the DP=8 per-GPU batch of the reference config (global 128 over 8 GPUs = 16 clips per GPU),
        # timed on this GPU alone: what each rank of the driver's 8-GPU C3 run would compute per step
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        config, criterion, model, B16, pixels, target = _setup({**spec, "batch": 16}, dev, rank)
        r16 = _train_and_time(model, config, criterion, pixels, target, world, rank, dev, args.c3_b16_steps,
                              args.c3_warmup, 0, tag="C3 b16: ")
        out["b16"] = {"value": round(world * B16 * args.c3_b16_steps / r16["elapsed"], 3), "unit": "clips/sec",
                      "clips_per_gpu": B16, "steps": args.c3_b16_steps, "warmup": args.c3_warmup,
                      "ms_per_step": round(1e3 * r16["elapsed"] / args.c3_b16_steps, 3),
                      "what": "SURVEY.md 8(d): C3's per-GPU batch under DP=8 (global 128, vmae_video.yaml:20), one GPU"}
        del r16, model, pixels, target
    return out


PEAK_F32 = PEAK_F32_TFLOPS


def r3d_flops(cfg, B):
    """Algorithmic FLOPs of one R3D-18 train step on B clips: per conv 2 Mo Co K (forward), the same
    for dW, and for dX (every conv but the stem: the pixels need no gradient); the head is negligible.
    Returns (forward, dX, dW)."""
    from vspike.r3d import r3d_convs

    def out(shape, c):
        return tuple((shape[i] + 2 * c.p[i] - c.k[i]) // c.s[i] + 1 for i in range(3))

    def flops(o, c):
        return 2.0 * B * o[0] * o[1] * o[2] * c.co * c.k[0] * c.k[1] * c.k[2] * c.ci_ref
    convs = {c.name: c for c in r3d_convs(cfg)}
    stem = convs["stem.0"]
    cur = out((cfg.num_frames, cfg.image_size, cfg.image_size), stem)
    fwd, dx = flops(cur, stem), 0.0
    for li, nb in enumerate(cfg.layers):
        for b in range(nb):
            pre = f"layer{li + 1}.{b}."
            o = out(cur, convs[pre + "conv1.0"])
            names = [pre + "conv1.0", pre + "conv2.0"] + ([pre + "downsample.0"] if pre + "downsample.0" in convs else [])
            for nm in names:
                f = flops(o, convs[nm])
                fwd += f
                dx += f
            cur = o
    return fwd, dx, fwd


def c4_subrecord(args, world, rank, dev):
    """BASELINE C4 in the same run: the R3D-18 encoder (32 x 112 x 112 clips, n = 256, fp32; the R3D
    plugin, vspike/r3d.py — no reference counterpart) under the reference head:
    timed train steps (fwd + bwd + AdamW, training-mode BatchNorm) and a full-batch fwd + bwd check
    against the CPU oracle's restatement (parity unpinned: there is no reference code for this
    encoder).  The conv kernels are implicit GEMMs on the exact-f32 MFMA: reported against the f32
    MFMA peak (157.3 TF) and with their operand bytes."""
    spec = {"model": "r3d18", "neurons": 256, "dtype": "fp32", "frames": None, "freeze": False,
            "lr": None, "loss": "poisson", "batch": args.c4_batch}
    config, criterion, model, B, pixels, target = _setup(spec, dev, rank)
    cfg = model.backbone
    check = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import cpu_ref
        sd = {k: v.detach().cpu() for k, v in model.reference_state_dict().items()}
        model.keep_relu_masks = True      # the oracle below takes the same ReLU decisions (see cpu_ref)
        out0 = model(pixels)
        masks = {k: v.cpu() for k, v in model.relu_masks.items()}
        model.keep_relu_masks, model.relu_masks = False, None
        loss0 = criterion(out0, target)
        loss0.backward()
        lay = model.layout
        g_enc, g_head = model.enc_flat.grad, model.head_flat.grad
        gpu_grads = {}
        for c in lay.convs:
            gpu_grads[c.name + ".weight"] = lay.enc.view(g_enc, c.name + ".weight")[..., :c.ci_ref].permute(
                0, 4, 1, 2, 3).cpu()
            bn = c.name[:-2] + ".1"
            for suf in (".weight", ".bias"):
                gpu_grads[bn + suf] = lay.enc.view(g_enc, bn + suf).cpu()
        for ref_name, slot in (("encoder.weight", "enc_w"), ("encoder.bias", "enc_b"), ("decoder.weight", "dec_w"),
                               ("decoder.bias", "dec_b")):
            gpu_grads[ref_name] = lay.head.view(g_head, slot).cpu()
        gl, gloss = out0.detach().cpu(), float(loss0.detach())
        model.zero_grad(set_to_none=True)
        model.load_reference_state_dict(sd)          # undo the check's running-statistics update
        del out0, loss0
        t0 = time.perf_counter()
        ccfg = cpu_ref.R3DCfg(num_frames=cfg.num_frames, image_size=cfg.image_size, num_channels=cfg.num_channels)
        # the oracle in f64: training-mode BatchNorm over 16 x 100,352 voxels makes torch's f32 CPU
        # backward itself drift by ~5e-3 of the conv gradients' norms (measured r05), so f32-vs-f32
        # would not say which side is off
        P = {k: v.double().clone().requires_grad_() for k, v in sd.items()
             if not k.endswith(("running_mean", "running_var"))}
        flips = {}
        ref = cpu_ref.r3d18_forward(pixels.cpu().double(), P, ccfg, relu_masks=masks, mask_log=flips)
        rloss = cpu_ref.poisson_nll_mean(ref, target.cpu().double())
        rloss.backward()
        e_out = float((gl - ref.detach()).abs().max() / ref.detach().abs().max())
        e_loss = abs(gloss - float(rloss)) / abs(float(rloss))
        errs = {k: float((gpu_grads[k].double() - P[k].grad.double()).norm() / P[k].grad.double().norm())
                for k in gpu_grads}
        # torch's own f32 CPU kernels against the same f64 result: the scale of f32 rounding on these
        # strongly cancelling BatchNorm-path gradients (the bars below are relative to it)
        P32 = {k: v.clone().requires_grad_() for k, v in sd.items() if not k.endswith(("running_mean", "running_var"))}
        cpu_ref.poisson_nll_mean(cpu_ref.r3d18_forward(pixels.cpu(), P32, ccfg, relu_masks=masks),
                                 target.cpu()).backward()
        nflip = sum(f[0] for f in flips.values())
        tie = max((f[1] / f[2] for f in flips.values() if f[0]), default=0.0)
        del masks
        e32 = {k: float((P32[k].grad.double() - P[k].grad.double()).norm() / P[k].grad.double().norm())
               for k in gpu_grads}
        del P32
        worst_conv = max((k for k in errs if not k.endswith((".1.weight", ".1.bias"))), key=errs.get)
        worst_bn = max((k for k in errs if k.endswith((".1.weight", ".1.bias"))), key=errs.get)
        tol = {"log_rates": 1e-4, "loss": 1e-5, "grad_conv_head": 1e-3, "grad_bn_affine": 3e-3,
               "grad_rule": "a gradient passes at its bar or at 3x torch-f32's distance from f64, the larger",
               "relu_tie": 1e-5}
        check = {"what": f"one fwd+bwd of the whole benched batch ({B} clips, training-mode BatchNorm) at the initial "
                         "weights vs the CPU oracle's R3D-18 restatement run in f64 (oracle/cpu_ref.py r3d18_forward), "
                         "conditioned on the plugin's ReLU decisions (the flipped ones must be rounding-level ties: "
                         "|pre-activation| < relu_tie of the unit's max); parity UNPINNED: the reference has no CNN "
                         "encoder",
                 "relu_flips": nflip, "relu_flip_max_rel": tie,
                 "log_rates_maxrel": round(e_out, 8), "loss_rel": round(e_loss, 9),
                 "worst_conv_head_grad": worst_conv, "worst_conv_head_grad_rel": round(errs[worst_conv], 6),
                 "worst_conv_head_grad_torch_f32_rel": round(e32[worst_conv], 6),
                 "worst_bn_grad": worst_bn, "worst_bn_grad_rel": round(errs[worst_bn], 6),
                 "worst_bn_grad_torch_f32_rel": round(e32[worst_bn], 6), "tolerance": tol,
                 "ok": bool(e_out < tol["log_rates"] and e_loss < tol["loss"] and tie < tol["relu_tie"] and all(
                     errs[k] <= max(tol["grad_bn_affine"] if k.endswith((".1.weight", ".1.bias"))
                                    else tol["grad_conv_head"], 3.0 * e32[k]) for k in errs)),
                 "cpu_seconds": round(time.perf_counter() - t0, 1)}
        del P, ref, rloss
        _progress(f"C4 check: {check}")
    run = _train_and_time(model, config, criterion, pixels, target, world, rank, dev, args.c4_steps, args.c4_warmup,
                          args.c4_profile_steps, tag="C4: ")
    fwd, dxf, dwf = r3d_flops(cfg, B)
    clips = world * B * args.c4_steps
    step_s = run["elapsed"] / args.c4_steps
    kern = {}
    for name in ("conv_fwd", "conv_dx", "conv_dw", "bn", "adamw", "gemm"):
        n, ms, work = run["kern"].get(name, (0, 0.0, 0.0))
        if not n:
            continue
        per_step_ms = ms / args.c4_profile_steps
        ent = {"ms_per_step": round(per_step_ms, 3), "launches_per_step": round(n / args.c4_profile_steps, 1)}
        if name.startswith("conv_"):
            tf = work / (ms / 1e3) / 1e12          # the conv timers carry flops
            ent.update({"bound": "mfma_f32", "tflops": round(tf, 2), "peak": PEAK_F32, "frac": round(tf / PEAK_F32, 4)})
        else:
            gbs = work / (ms / 1e3) / 1e9
            ent.update({"bound": "hbm", "gbs": round(gbs, 1), "peak": PEAK_HBM_GBS, "frac": round(gbs / PEAK_HBM_GBS, 4)})
        kern[name] = ent
    total_tf = (fwd + dxf + dwf) / step_s / 1e12
    out = {"metric": f"clips/sec ({cfg.num_frames}-frame {cfg.image_size}x{cfg.image_size}) train step",
           "value": round(clips / run["elapsed"], 3), "unit": "clips/sec", "n_gpus": world, "steps": args.c4_steps,
           "warmup": args.c4_warmup, "ms_per_step": round(1e3 * step_s, 3), "dtype": "fp32",
           "config": {"workload": f"C4 R3D-18 {cfg.num_frames}x{cfg.image_size}x{cfg.image_size} -> 256 neurons, "
                                  "encoder+head fwd+bwd+AdamW (training-mode BatchNorm)", "model": "r3d18",
                      "global_batch": B * world, "clips_per_gpu": B, "parallelism": f"dp{world}"},
           "model_tflops": round(total_tf, 2), "f32_mfma_util_pct": round(100 * total_tf / PEAK_F32, 2),
           "check": check, "final_loss": round(run["final_loss"], 6), "replicas_equal": run["replicas_equal"],
           "dispatch_per_step": run["dispatch"], "kernels": kern}
    del run, model
    return out


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = torch.cuda.device_count()
    if world > ndev and args.backend == "nccl":
        raise SystemExit(f"bench.py: {world} ranks but {ndev} visible GPU(s): RCCL needs one GPU per rank "
                         "(--backend gloo shares a device)")
    dev = torch.device("cuda", local % max(ndev, 1))
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")

    from vspike import _lib as L

    spec = {"model": args.model, "neurons": args.neurons, "dtype": args.dtype, "frames": args.frames,
            "freeze": args.freeze, "lr": args.lr, "loss": args.loss, "batch": args.batch}
    config, criterion, model, B, pixels, target = _setup(spec, dev, rank)
    bb = model.backbone
    do_cpu = args.full and rank == 0 and world == 1 and not args.no_cpu_baseline
    parity = None
    L.dispatch_reset()
    if do_cpu:
        # in-run parity of the BENCHED dispatch: one fwd+bwd of the whole batch (M = B * tokens rows,
        # the same kernels the timed step runs) at the initial weights, against the CPU oracle below
        init_params = {k: v.detach().cpu().numpy() for k, v in model.reference_state_dict(modern_names=True).items()}
        out0 = model(pixels)
        loss0 = criterion(out0, target)
        loss0.backward()
        gpu_par = {"loss": float(loss0), "log_rates": out0.detach().float().cpu(),
                   "grads": _reference_grads(model)}
        model.zero_grad(set_to_none=True)
        del out0, loss0

    run = _train_and_time(model, config, criterion, pixels, target, world, rank, dev, args.steps, args.warmup,
                          args.profile_steps, graph=args.graph, instrument=args.full, dump_dir=args.dump_outputs)
    elapsed, final_loss, replicas_equal, dispatch = run["elapsed"], run["final_loss"], run["replicas_equal"], \
        run["dispatch"]
    redo = run["attn_redo_per_step"]
    clips = world * B * args.steps
    value = clips / elapsed
    N = bb.num_tokens
    peak_mfma = PEAK_F32_TFLOPS if args.dtype == "fp32" else PEAK_BF16_TFLOPS
    _, roofline = _roofline(run["kern"], args.profile_steps, bb, B, args.dtype)
    step_tflops = _train_flops_per_clip(bb, args.neurons) * B * world * args.steps / elapsed / 1e12

    cpu = None
    if do_cpu:
        ccfg = _oracle_cfg(bb)
        if not args.no_cpu_timing:
            cpu, _ = cpu_baseline(ccfg, init_params, pixels[:4].cpu(), target[:4].cpu(), args.cpu_seconds)
        parity = full_batch_parity(ccfg, init_params, pixels.cpu(), target.cpu(), gpu_par, args)

    c3 = None
    # the C3 / C4 sub-records are single-GPU evidence (N = 1 only): at N > 1 a rank that failed inside one
    # while the others sit in its collectives would hang the multi-GPU run the driver times
    want_c3 = (args.full and not args.no_c3 and args.model == "vmae_tiny" and args.dtype == "bf16" and not args.graph and
               not args.freeze and args.loss == "poisson" and world == 1)
    if want_c3:
        del run, model, pixels, target
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        try:
            c3 = c3_subrecord(args, world, rank, dev)
        except Exception as exc:       # recorded in the line; the C2 measurement stands on its own
            c3 = {"error": f"{type(exc).__name__}: {exc}"}
            _progress(f"C3 sub-record failed: {c3['error']}")

    c4 = None
    if args.full and not args.no_c4 and args.model == "vmae_tiny" and args.dtype == "bf16" and not args.graph and not args.freeze \
            and args.loss == "poisson" and world == 1:
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        try:
            c4 = c4_subrecord(args, world, rank, dev)
        except Exception as exc:
            c4 = {"error": f"{type(exc).__name__}: {exc}"}
            _progress(f"C4 sub-record failed: {c4['error']}")

    if rank == 0:
        workload = ("C5 ViT-Base/16 encoder (no temporal transformer: no reference code)"
                    if bb.hidden_size == 768 and bb.num_frames == 32 else
                    "C3 ViT-Base/16" if bb.hidden_size == 768 else "C2 ViT-Tiny/16" if bb.hidden_size == 192
                    else f"ViT d{bb.hidden_size}")
        line = {
            "metric": f"clips/sec ({bb.num_frames}-frame {bb.image_size}x{bb.image_size}) train step", "value": round(value, 3), "unit": "clips/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic (randn pixels, Poisson targets), random-init",
            "config": {"workload": f"{workload} {bb.num_frames}x{bb.image_size}x{bb.image_size} -> {args.neurons} "
                                   f"neurons, {'head only (encoder frozen)' if args.freeze else 'encoder+head'} "
                                   "fwd+bwd+AdamW",
                       "model": args.model, "global_batch": B * world, "clips_per_gpu": B, "seq_len": N,
                       "parallelism": f"dp{world}"},
            "mfma_util_pct": round(100.0 * step_tflops / peak_mfma, 2),
            "model_tflops": round(step_tflops, 2),
            "roofline": roofline, "cpu_baseline": cpu, "parity": parity, "final_loss": round(final_loss, 6),
            "lr": float(config["optimizer"]["lr"]), "loss": args.loss, "backend": args.backend if world > 1 else None,
            "replicas_equal": replicas_equal, "build_id": L.build_id(), "dispatch_per_step": dispatch,
            "knobs_nondefault": L.knobs_nondefault(),
            # the attention forward's fast pass (no running max) re-runs a workgroup under the safe
            # softmax when a query's scores leave its band: how often that happened in the timed steps
            "attn_redo": {"workgroups_per_step": redo,
                          "of": bb.num_hidden_layers * B * bb.num_attention_heads * ((N + 127) // 128),
                          "logit_scale_sweep": "profiles/r05_attn_logit_scale.txt"},
            "c3": c3, "c4": c4,
        }
        if args.graph:
            line["step_mode"] = "hipGraph replay (vspike.graph.GraphedStep)"
        print(json.dumps(line), flush=True)
        if parity is not None and not parity["ok"]:
            print(f"bench.py: PARITY FAILED for the benched dispatch: {json.dumps(parity)}", file=sys.stderr, flush=True)
    if world > 1:
        dist.destroy_process_group()
    if parity is not None and not parity["ok"]:
        sys.exit(3)


if __name__ == "__main__":
    main()
