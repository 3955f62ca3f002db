"""Time vs_attn32_fwd / vs_attn32_bwd (bf16) at the MAE decoder's shape against (a) a copy_ that moves the same
number of bytes and (b) torch's SDPA at the same shape, on one GPU.

The work is launch- and bandwidth-bound (1.8 GFLOP forward at B = 128, H = 16, N = 82), so the copy is the yardstick;
SDPA is the alternative a user would reach for.  Each candidate is timed with device events over `--iters` back-to-back
calls after a warm-up, `--rounds` times, alternating the candidates inside a round; the median round is reported and
the spread (min, max) kept.

    python scripts/attn32_bench.py --out profiles/attn32_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-spike_amd"))


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=82)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn32_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn32_bench: needs a GPU (no fallback)")
    from vspike import _lib, ops
    B, H, N = a.batch, a.heads, a.tokens
    D, M = 32 * H, a.batch * a.tokens
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(M, 3 * D, generator=g).to(bf).to(dev)
    do = torch.randn(M, D, generator=g).to(bf).to(dev)
    o = torch.empty(M, D, dtype=bf, device=dev)
    lse = torch.empty(B, H, N, device=dev)
    dqkv = torch.empty(M, 3 * D, dtype=bf, device=dev)
    ws = torch.empty(ops.attn32_bwd_workspace_bytes(B, N, H) // 4 + 64, device=dev)
    fwd_bytes = 4 * M * D * 2 + B * H * N * 4               # Q, K, V in, O out, lse out
    bwd_bytes = 8 * M * D * 2 + B * H * N * 4               # Q, K, V, O, dO in, dQ, dK, dV out, lse in
    # a copy_ moves its bytes twice (read + write): half the kernel's bytes as the source
    src_f = torch.empty(fwd_bytes // 4, dtype=bf, device=dev).normal_()
    src_b = torch.empty(bwd_bytes // 4, dtype=bf, device=dev).normal_()
    dst_f, dst_b = torch.empty_like(src_f), torch.empty_like(src_b)
    q, k, v = (t.contiguous().requires_grad_() for t in qkv.view(B, N, 3, H, 32).permute(2, 0, 3, 1, 4))
    d4 = do.view(B, N, H, 32).permute(0, 2, 1, 3).contiguous()
    sdpa = torch.nn.functional.scaled_dot_product_attention
    cands = {
        "attn32_fwd": lambda: ops.attn32_fwd(qkv, o, lse, B, N, H),
        "attn32_bwd": lambda: ops.attn32_bwd(qkv, o, do, lse, dqkv, ws, B, N, H),
        "copy_fwd_bytes": lambda: dst_f.copy_(src_f),
        "copy_bwd_bytes": lambda: dst_b.copy_(src_b),
    }
    notes = {}
    try:
        with torch.no_grad():
            sdpa(q, k, v)
        out = sdpa(q, k, v)
        torch.autograd.grad(out, (q, k, v), d4, retain_graph=True)
        torch.cuda.synchronize()

        def sdpa_fwd():
            with torch.no_grad():
                sdpa(q, k, v)
        cands["sdpa_fwd"] = sdpa_fwd
        cands["sdpa_bwd"] = lambda: torch.autograd.grad(out, (q, k, v), d4, retain_graph=True)
    except Exception as e:                                   # recorded, not hidden: the comparison is then missing
        notes["sdpa_error"] = f"{type(e).__name__}: {e}"[:300]
    ops.attn32_fwd(qkv, o, lse, B, N, H)
    for fn in cands.values():                                # warm-up: code objects, allocator
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cands}
    for _ in range(a.rounds):
        for name, fn in cands.items():
            samples[name].append(timed(fn, a.iters))
    res = {name: {"us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)} for name, v in samples.items()}
    med = lambda n: res[n]["us_median"]  # noqa: E731
    ratios = {"fwd_over_copy": med("attn32_fwd") / med("copy_fwd_bytes"),
              "bwd_over_copy": med("attn32_bwd") / med("copy_bwd_bytes")}
    if "sdpa_fwd" in res:
        ratios["fwd_over_sdpa"] = med("attn32_fwd") / med("sdpa_fwd")
        ratios["bwd_over_sdpa"] = med("attn32_bwd") / med("sdpa_bwd")
    doc = {"shape": {"B": B, "H": H, "N": N, "head_dim": 32, "dtype": "bf16"}, "iters": a.iters, "rounds": a.rounds,
           "bytes": {"fwd": fwd_bytes, "bwd": bwd_bytes},
           "gbytes_per_s": {"attn32_fwd": fwd_bytes / med("attn32_fwd") * 1e-3,
                            "attn32_bwd": bwd_bytes / med("attn32_bwd") * 1e-3,
                            "copy_fwd_bytes": fwd_bytes / med("copy_fwd_bytes") * 1e-3,
                            "copy_bwd_bytes": bwd_bytes / med("copy_bwd_bytes") * 1e-3},
           "us": res, "ratios_time_over_reference": ratios, "notes": notes,
           "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "knobs": _lib.knobs_nondefault()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(doc["us"]), json.dumps(ratios), json.dumps(notes))


if __name__ == "__main__":
    main()
