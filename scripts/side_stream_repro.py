"""Reproduce the block executor's side-stream nondeterminism at a row count that is no multiple of 64.

The plain VideoMAE plugin in bf16, 15 clips x 81 tokens = 1,215 token rows, D = 128, 2 layers: forward + backward
from one fixed state, many times, with the weight-gradient products on the side stream and in order on the main
stream, under a competing load on another stream (it moves the relative timing of the two streams).  Reports how
many backwards differ from the first one and which gradient slots.  Observed on MI355X: 21 of 400 with the side
stream, 0 of 400 in order; the first differing values are one row of a LayerNorm backward's dx and 16 columns of
its dgamma (never dbeta), i.e. 64 bytes of the f32 input it re-reads.

Usage: timeout -k 10 300 python scripts/side_stream_repro.py [--iters 400]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-spike_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DEV = "cuda"
B, N_NEURONS = 15, 16
CONF = {"freeze_encoder": False, "compute_dtype": "bf16",
        "backbone": {"image_size": 48, "num_frames": 18, "hidden_size": 128, "num_hidden_layers": 2,
                     "num_attention_heads": 2, "intermediate_size": 256},
        "encoder": {"output_dim": 64}, "decoder": {"output_dim": 100 * N_NEURONS}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("side_stream_repro.py runs on the GPU; none is visible")
    from vspike import VideoMAE, _lib as L, poisson_nll_mean
    other = torch.cuda.Stream()
    big = torch.randn(2048, 2048, device=DEV)
    g = torch.Generator().manual_seed(3)
    px = torch.randn(B, 18, 3, 48, 48, generator=g).to(DEV)
    y = (torch.rand(B, 100, N_NEURONS, generator=g) < 0.12).float().to(DEV)

    def once(m, k):
        m.zero_grad(set_to_none=True)
        if k:
            with torch.cuda.stream(other):
                for _ in range(k):
                    torch.mm(big, big)
        loss = poisson_nll_mean(m(px), y)
        loss.backward()
        return loss.detach().clone(), m.enc_flat.grad.clone(), m.head_flat.grad.clone()

    print(f"build {L.build_id()}")
    for side in (True, False):
        torch.manual_seed(1)
        m = VideoMAE(CONF).to(DEV)
        with torch.no_grad():
            m.enc_flat.mul_(5.0)          # wide weights: activations of O(1..10)
        m.invalidate_lp()
        m.set_side_stream(side)
        base = once(m, 0)
        torch.cuda.synchronize()
        slots, hits = {}, 0
        for it in range(a.iters):
            r = once(m, (it % 5) * 2)
            hit = False
            for name, x, z in zip(("loss", "enc", "head"), base, r):
                if torch.equal(x, z):
                    continue
                hit = True
                if name != "enc":
                    slots[name] = slots.get(name, 0) + 1
                    continue
                for sname, s in m.layout.enc.slots.items():
                    if not torch.equal(x[s.offset:s.offset + s.numel], z[s.offset:s.offset + s.numel]):
                        slots[sname] = slots.get(sname, 0) + 1
            hits += hit
        torch.cuda.synchronize()
        print(f"VideoMAE rows {B * m.backbone.num_tokens} side_stream={side}: {hits} of {a.iters} backwards differ; "
              f"slots: {slots or 'none'}", flush=True)


if __name__ == "__main__":
    main()
