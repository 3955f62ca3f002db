"""Time the MAE plugin's pretraining step (config/model/mae.yaml: ViT-Base encoder on 20 of 81 patches, 512 x 8
decoder on 82 tokens; bf16, n = 128 images, one GPU) and every new kernel alone at that geometry.

    python scripts/mae_bench.py --out profiles/mae_bench.json

Step time: device events around `--steps` back-to-back ContrastTrainer.step_recon calls after a warm-up, `--rounds`
times, the median round reported.  Kernel times: device events around 200 back-to-back calls of each entry on
buffers of the step's shapes.  ContrastViT's recorded step (profiles/contrast_bench.json: 26.7 ms per 384 images) is
quoted beside it; it is not re-measured here.
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
    for _ in range(3):
        fn()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mae_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mae_bench: needs a GPU (no fallback)")
    from vspike import NAME2MODEL, FusedAdamW, _lib, ops
    from vspike.config import load_run_config
    from vspike.trainer import ContrastTrainer
    cfg = load_run_config(os.path.join(ROOT, "video-spike_amd", "config", "model", "mae.yaml"),
                          os.path.join(ROOT, "video-spike_amd", "config", "train", "vmae_video.yaml"))
    dev, bf, f32 = "cuda", torch.bfloat16, torch.float32
    m = NAME2MODEL[cfg.model.model_class](cfg.model).to(dev)
    tr = ContrastTrainer(m, FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4))
    G = a.batch
    x = torch.randn(G, m.num_channels, m.image_size, m.image_size, device=dev)
    for _ in range(a.warmup):
        tr.step_recon(x)
    torch.cuda.synchronize()
    step_us = [timed(lambda: tr.step_recon(x), a.steps) for _ in range(a.rounds)]
    ms = statistics.median(step_us) / 1e3

    # every new kernel alone, at the step's shapes
    P, D, Dd, K, H = m.num_patches, m.hidden_size, m.decoder_hidden_size, m.patch_dim, m.dec_stack.H
    Lk = int(P * (1 - m.config.mask_ratio))
    shuffle = torch.argsort(torch.rand(G, P, device=dev), dim=1)
    restore = torch.argsort(shuffle, dim=1).to(torch.int32).contiguous()
    keep = shuffle[:, :Lk].to(torch.int32).contiguous()
    R = lambda *s, dt=f32: torch.randn(*s, device=dev).to(dt)  # noqa: E731
    patches, cls, table, x0 = R(G * P, D), R(D), R(P + 1, D), R(G, Lk + 1, D)
    d_cls, d_patch = R(D), R(G * P, D, dt=bf)
    e, tok, tabd, xd = R(G, Lk + 1, Dd), R(Dd), R(P + 1, Dd), R(G, P + 1, Dd)
    d_e, d_tok = R(G, Lk + 1, Dd, dt=bf), R(Dd)
    ws_a = torch.empty(ops.mae_dec_assemble_bwd_workspace_bytes(G, Dd) // 4, device=dev)
    pred, d_pred, loss = R(G, P + 1, K), R(G, P + 1, K, dt=bf), torch.empty(1, device=dev)
    ws_l = torch.empty(ops.mae_recon_loss_workspace_bytes(G, P) // 4, device=dev)
    N, M = P + 1, G * (P + 1)
    qkv, do, o = R(M, 3 * Dd, dt=bf), R(M, Dd, dt=bf), torch.empty(M, Dd, dtype=bf, device=dev)
    lse, dqkv = torch.empty(G, H, N, device=dev), torch.empty(M, 3 * Dd, dtype=bf, device=dev)
    ws_q = torch.empty(ops.attn32_bwd_workspace_bytes(G, N, H) // 4 + 64, device=dev)
    ops.attn32_fwd(qkv, o, lse, G, N, H)
    kernels = {
        "vs_mae_embed_fwd": lambda: ops.mae_embed_fwd(patches, keep, cls, table, x0),
        "vs_mae_embed_bwd": lambda: ops.mae_embed_bwd(x0, restore, d_cls, d_patch),
        "vs_mae_dec_assemble_fwd": lambda: ops.mae_dec_assemble_fwd(e, restore, tok, tabd, xd),
        "vs_mae_dec_assemble_bwd": lambda: ops.mae_dec_assemble_bwd(xd, keep, restore, d_e, d_tok, ws_a),
        "vs_mae_recon_loss": lambda: ops.mae_recon_loss(pred, x, restore, Lk, m.patch_size, loss, d_pred, ws_l),
        "vs_attn32_fwd": lambda: ops.attn32_fwd(qkv, o, lse, G, N, H),
        "vs_attn32_bwd": lambda: ops.attn32_bwd(qkv, o, do, lse, dqkv, ws_q, G, N, H),
    }
    kus = {name: timed(fn, 200) for name, fn in kernels.items()}
    per_step = {k: (m.dec_stack.layers if "attn32" in k else 1) * v for k, v in kus.items()}
    doc = {"model": "config/model/mae.yaml", "dtype": "bf16", "images": G, "kept_patches": Lk, "decoder_tokens": N,
           "ms_per_step": ms, "ms_per_step_rounds": [u / 1e3 for u in step_us], "images_per_s": G / ms * 1e3,
           "contrast_vit_recorded": {"ms_per_step": 26.7, "images": 384, "source": "profiles/contrast_bench.json"},
           "kernel_us": kus, "new_kernels_us_per_step": sum(per_step.values()),
           "new_kernels_share_of_step": sum(per_step.values()) / (ms * 1e3),
           "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "knobs": _lib.knobs_nondefault()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
