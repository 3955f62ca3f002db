#!/usr/bin/env python
"""Generate tests/golden/contrast_vit.npz: the ContrastViT plugin's pinned outputs.

Run once, where the reference checkout and `transformers` are importable:

    python scripts/gen_contrast_fixture.py --reference /path/to/video-spike

At run time it builds the installed HF `ViTMAEModel` (eager attention, mask_ratio 0.0) from a local config,
loads the seeded parameters of tests/contrast_ref.py (inputs and weights are re-derived from (seed, name) by
oracle/prng.py, so the fixture holds OUTPUTS only), runs the reference model's forward (vit_mae.py:36-44) on
the three views and the reference's own `loss_fn_` (src/utils/loss_utils.py), and stores per geometry:
z of the 3n images, (loss, pos_loss, neg_loss) with fix_temp true and with fix_temp false at temperature 0.3,
`cpu_ref.summarize` of every gradient (temperature's included in the second case), and the position table.
It asserts that the fixture is informative (embeddings spread out, loss away from ln n) and that two HF runs
with different patch shuffles agree to a tenth of the project's fp32 bars.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-spike_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import contrast_ref as cr                     # noqa: E402
from oracle import cpu_ref                    # noqa: E402
from vspike.contrast import _v5_name          # noqa: E402

# Every gradient is stored in summarised form (norm, 3 projections, first 512 values), never as a full tensor:
# compare_summary judges a full tensor element by element against |ref| of that element, which HF itself does
# not meet from one patch shuffle to the next (elements near zero move by 1e-7 absolute); the summarised form is
# judged against the tensor's norm / the leading values' maximum.  It also keeps the file small.
FULL_LIMIT = 0


def hf_model(geom):
    from transformers import ViTMAEConfig, ViTMAEModel
    c = cr.vit_cfg(geom)
    conf = ViTMAEConfig(hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers,
                        num_attention_heads=c.num_attention_heads, intermediate_size=c.intermediate_size,
                        hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                        layer_norm_eps=c.layer_norm_eps, image_size=c.image_size, patch_size=c.patch_size,
                        num_channels=c.num_channels, qkv_bias=True, mask_ratio=0.0, attn_implementation="eager")
    vit = ViTMAEModel(conf)
    params = cr.make_params(geom)
    if not vit.embeddings.position_embeddings.abs().max() > 0:
        # transformers 5.x leaves the table to from_pretrained's weight initialisation: run HF's own
        # sin-cos initialiser (4.38, the reference's pin, runs it in the constructor)
        vit.embeddings.patch_embeddings.projection._is_hf_initialized = False
        vit.embeddings.initialize_weights()
    own = vit.state_dict()
    table = own["embeddings.position_embeddings"].clone()
    assert table.abs().max() > 0.5 and not table[0, 0].any(), "HF's position table was not initialised"
    sd = {}
    for name, v in params.items():
        if name.startswith("vit."):
            key = _v5_name(name)[len("vit."):]
            if key not in own:                       # an older transformers: the reference's own spelling
                key = name[len("vit."):]
            sd[key] = torch.from_numpy(v)
    sd["embeddings.position_embeddings"] = table
    missing = set(own) - set(sd)
    assert not missing, missing
    vit.load_state_dict(sd, strict=True)
    vit.train()
    proj = torch.nn.Linear(c.hidden_size, cr.GEOMETRIES[geom]["embed_size"])
    with torch.no_grad():
        proj.weight.copy_(torch.from_numpy(params["proj.weight"]))
        proj.bias.copy_(torch.from_numpy(params["proj.bias"]))
    return vit, proj, table[0]


def ref_names(vit, proj, temperature):
    """reference parameter name -> tensor (the names of contrast_ref.param_shapes)."""
    own = dict(vit.named_parameters())
    out = {}
    c_names = cr.param_shapes(cr.vit_cfg("g1"), 3)
    for name in c_names:
        if name.startswith("vit."):
            key = _v5_name(name)[len("vit."):]
            out[name] = own[key] if key in own else own[name[len("vit."):]]
    out["proj.weight"], out["proj.bias"], out["temperature"] = proj.weight, proj.bias, temperature
    return out


def run(geom, loss_fn_, fix_temp, seed):
    """One reference step (three forwards, loss_fn_, backward) with HF's shuffle noise drawn from `seed`."""
    vit, proj, table = hf_model(geom)
    temperature = torch.nn.Parameter(torch.tensor(0.0 if fix_temp else cr.TEMPERATURE))
    gen = torch.Generator().manual_seed(seed)
    P = (cr.vit_cfg(geom).image_size // 16) ** 2

    def model(x):                                # vit_mae.py:36-44
        noise = torch.rand(x.shape[0], P, generator=gen)
        cls = vit(pixel_values=x, noise=noise).last_hidden_state[:, 0]
        z = proj(cls)
        z = z / z.norm(dim=-1, keepdim=True)
        return {"z": z, "temp": 1 / temperature.exp()}

    outs = [model(torch.from_numpy(cr.make_images(geom, w))) for w in ("ref", "pos", "neg")]
    res = loss_fn_(*outs, fix_temp=fix_temp)
    res["loss"].backward()
    grads = {n: (t.grad.detach().numpy().copy() if t.grad is not None else None)
             for n, t in ref_names(vit, proj, temperature).items()}
    z = torch.cat([o["z"] for o in outs]).detach().numpy()
    losses = np.array([float(res[k].detach()) for k in ("loss", "pos_loss", "neg_loss")], dtype=np.float64)
    return z, losses, grads, table.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VIDEO_SPIKE_REFERENCE"),
                    help="checkout of PPWangyc/video-spike (or set VIDEO_SPIKE_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "contrast_vit.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or VIDEO_SPIKE_REFERENCE) is required: loss_fn_ is imported from it")
    sys.path.insert(0, os.path.join(a.reference, "src"))
    from utils.loss_utils import loss_fn_
    torch.manual_seed(0)
    fx = {}
    for geom in cr.GEOMETRIES:
        n = cr.GEOMETRIES[geom]["n"]
        for tag, fix_temp in (("fix", True), ("tau", False)):
            z, losses, grads, table = run(geom, loss_fn_, fix_temp, seed=1)
            z2, losses2, grads2, _ = run(geom, loss_fn_, fix_temp, seed=2)      # another shuffle
            # informative: embeddings spread out, the loss away from its degenerate value ln n
            cos = z @ z.T
            off = cos[~np.eye(len(z), dtype=bool)]
            assert off.min() < 0.5, (geom, off.min())
            assert abs(losses[0] - np.log(n)) > 0.02, (geom, losses[0], np.log(n))
            # the shuffle does not matter: a tenth of the fp32 bars (z 1e-4 of max|z|, losses 1e-5, gradients 1e-3)
            assert np.abs(z - z2).max() <= 1e-5 * np.abs(z).max(), np.abs(z - z2).max()
            assert np.all(np.abs(losses - losses2) <= 1e-6 * np.abs(losses)), (losses, losses2)
            for name, g in grads.items():
                if not cr.trainable(name, fix_temp):
                    continue
                e = np.linalg.norm((g - grads2[name]).ravel()) / max(np.linalg.norm(g.ravel()), 1e-30)
                assert e <= 1e-4, (name, e)
            # the key bias has no gradient beyond rounding, under fix_temp `temperature` has none at all
            for name, g in grads.items():
                if name.endswith("key.bias"):
                    qn = np.linalg.norm(grads[name.replace("key.bias", "query.bias")])
                    assert np.linalg.norm(g) <= 1e-5 * qn, (name, np.linalg.norm(g), qn)
            assert (grads["temperature"] is None) == fix_temp
            fx[f"{geom}/{tag}/losses"] = losses
            for name, g in grads.items():
                if cr.trainable(name, fix_temp):
                    for k, v in cpu_ref.summarize(name, g, full_limit=FULL_LIMIT).items():
                        fx[f"{geom}/{tag}/{k}"] = v
            print(f"{geom}/{tag}: losses {losses}, ln n {np.log(n):.4f}, min off-diagonal cosine {off.min():.3f}, "
                  f"shuffle dz {np.abs(z - z2).max():.2e}")
        fx[f"{geom}/z"] = z.astype(np.float32)
        fx[f"{geom}/table"] = table.astype(np.float32)
    np.savez_compressed(a.out, **fx)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {len(fx)} arrays")


if __name__ == "__main__":
    main()
