#!/usr/bin/env python
"""Generate tests/golden/mae.npz: the MAE plugin's pinned outputs.

Run once, where the reference checkout and `transformers` are importable:

    python scripts/gen_mae_fixture.py --reference /path/to/video-spike

At run time it builds the installed HF `ViTMAEForPreTraining` (eager attention) from a local config, loads the seeded
parameters of tests/mae_ref.py (weights, images and noise are re-derived from (seed, name) by oracle/prng.py; the noise
is stored as well because the index plumbing depends on its exact bits), and runs it in float64 and in float32.  The
reference's `MAE` / `ViTMAE` classes are read from src/model/vit_mae/vit_mae.py by name with `ast` (the file imports
`wandb`) to check that they are what tests/mae_ref.py says they are: `MAE.forward` normalises the CLS latent without a
projection, and `ViTMAE.forward` passes `head_mask` and calls `forward_loss`, which transformers 5.x no longer has — so
its few lines are restated here: `last_hidden_state`, the decoder's logits and HF's own masked pixel loss.

Stored per geometry: noise, ids_restore, mask, latent, logits, recon_loss, z (float64 run, stored as float32; the loss
as float64), z at mask_ratio 0, `cpu_ref.summarize` of every gradient of the float64 run and of the float32 run (`f32/*`) -- summaries, not full
tensors: the encoder alone has 430k parameters per geometry and a committed file stays under 1 MiB -- and per gradient
the norm-relative distance of the float32 run from the float64 one (`hf32_err/*`: the reference's own error).
"""
import argparse
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-spike_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mae_ref as mr                          # noqa: E402
from oracle import cpu_ref                    # noqa: E402
from vspike.contrast import _V5               # noqa: E402

FULL_LIMIT = 0          # gradients in summarised form only (see scripts/gen_contrast_fixture.py)


def check_reference(path):
    """The reference's classes are the ones restated: read by name, never imported."""
    tree = ast.parse(open(os.path.join(path, "src", "model", "vit_mae", "vit_mae.py")).read())
    cls = {n.name: n for n in tree.body if isinstance(n, ast.ClassDef)}
    mae_src, vit_src = ast.unparse(cls["MAE"]), ast.unparse(cls["ViTMAE"])
    assert "cls_token / cls_token.norm(dim=-1, keepdim=True)" in mae_src and "proj" not in mae_src, mae_src
    assert "ViTMAEForPreTraining" in vit_src and "self.forward_loss(pixel_values, logits, mask)" in vit_src
    assert "latent[:, 0]" in vit_src and "self.decoder(latent, ids_restore)" in vit_src


def _hf_key(name, own):
    """reference (4.38) parameter name -> the installed transformers' name."""
    key = name[len("vit_mae."):]
    if key in own:
        return key
    key = key.replace("vit.encoder.layer.", "vit.layers.")
    for new, old in _V5:
        key = key.replace("." + old, "." + new)
    assert key in own, (name, key)
    return key


def hf_model(geom, dtype):
    from transformers import ViTMAEConfig, ViTMAEForPreTraining
    c, g = mr.vit_cfg(geom), mr.GEOMETRIES[geom]
    conf = ViTMAEConfig(hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers,
                        num_attention_heads=c.num_attention_heads, intermediate_size=c.intermediate_size,
                        hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                        layer_norm_eps=c.layer_norm_eps, image_size=c.image_size, patch_size=c.patch_size,
                        num_channels=c.num_channels, qkv_bias=True, mask_ratio=g["mask_ratio"], norm_pix_loss=False,
                        decoder_hidden_size=g["decoder_hidden_size"],
                        decoder_num_attention_heads=g["decoder_num_attention_heads"],
                        decoder_num_hidden_layers=g["decoder_num_hidden_layers"],
                        decoder_intermediate_size=g["decoder_intermediate_size"], attn_implementation="eager")
    model = ViTMAEForPreTraining(conf)
    own = model.state_dict()
    grid = c.image_size // c.patch_size
    sd = {_hf_key(n, own): torch.from_numpy(v) for n, v in mr.make_params(geom).items()}
    # the fixed tables of the reference's pin (4.38: [sin w | cos w | sin h | cos h]), whatever the installed
    # version initialises
    sd["vit.embeddings.position_embeddings"] = torch.from_numpy(mr._table64(c.hidden_size, grid)).float()[None]
    sd["decoder.decoder_pos_embed"] = torch.from_numpy(mr._table64(g["decoder_hidden_size"], grid)).float()[None]
    missing = set(own) - set(sd)
    assert not missing, missing
    model.load_state_dict(sd, strict=True)
    model.train()
    return model.to(dtype), {n: _hf_key(n, own) for n in mr.param_shapes(geom)}


def run(geom, dtype, mask_ratio=None):
    model, names = hf_model(geom, dtype)
    x = torch.from_numpy(mr.make_images(geom)).to(dtype)
    noise = torch.from_numpy(mr.make_noise(geom))
    if mask_ratio is not None:
        model.config.mask_ratio = mask_ratio
        model.vit.embeddings.config.mask_ratio = mask_ratio
        latent = model.vit(pixel_values=x, noise=noise).last_hidden_state
        return {"z": (latent[:, 0] / latent[:, 0].norm(dim=-1, keepdim=True)).detach().numpy()}
    # vit_mae.py:74-94 restated for transformers 5.x (module docstring)
    outputs = model.vit(pixel_values=x, noise=noise)
    latent, ids_restore, mask = outputs.last_hidden_state, outputs.ids_restore, outputs.mask
    logits = model.decoder(latent, ids_restore).logits
    loss = (((logits - model.patchify(x)) ** 2).mean(dim=-1) * mask).sum() / mask.sum()
    whole = model(pixel_values=x, noise=noise)                 # HF's own forward gives the same loss
    assert torch.equal(whole.loss, loss), (whole.loss, loss)
    cls_token = latent[:, 0]
    z = cls_token / cls_token.norm(dim=-1, keepdim=True)       # vit_mae.py:54
    loss.backward()
    own = dict(model.named_parameters())
    grads = {n: own[k].grad.detach().numpy().astype(np.float64) for n, k in names.items()}
    return {"z": z.detach().numpy(), "latent": latent.detach().numpy(), "logits": logits.detach().numpy(),
            "recon_loss": float(loss.detach()), "ids_restore": ids_restore.numpy(), "mask": mask.detach().numpy(),
            "grads": grads}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VIDEO_SPIKE_REFERENCE"),
                    help="checkout of PPWangyc/video-spike (or set VIDEO_SPIKE_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mae.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or VIDEO_SPIKE_REFERENCE) is required: its MAE / ViTMAE classes are checked")
    check_reference(a.reference)
    torch.manual_seed(0)
    fx = {}
    for geom in mr.GEOMETRIES:
        noise = mr.make_noise(geom)
        assert mr.noise_ok(noise, mr.len_keep(geom)), f"{geom}: choose another mae_ref.SEED"
        r64, r32 = run(geom, torch.float64), run(geom, torch.float32)
        z0 = run(geom, torch.float64, mask_ratio=0.0)["z"]
        assert np.array_equal(r64["ids_restore"], r32["ids_restore"])
        assert int(r64["mask"].sum()) == noise.shape[0] * (noise.shape[1] - mr.len_keep(geom))
        # informative: the loss is not the trivial one of logits = 0, and z moves with the mask
        assert abs(r64["recon_loss"] - 1.0) > 0.05, r64["recon_loss"]
        fx[f"{geom}/noise"] = noise
        fx[f"{geom}/ids_restore"] = r64["ids_restore"].astype(np.int32)
        fx[f"{geom}/mask"] = r64["mask"].astype(np.float32)
        for k in ("latent", "logits", "z"):
            fx[f"{geom}/{k}"] = r64[k].astype(np.float32)
        fx[f"{geom}/recon_loss"] = np.array([r64["recon_loss"], r32["recon_loss"]], dtype=np.float64)
        fx[f"{geom}/z_mask0"] = z0.astype(np.float32)
        worst = 0.0
        for name, g in r64["grads"].items():
            if name.endswith("key.bias"):
                # no gradient beyond rounding -- float32 rounding even here: HF's eager attention computes its
                # softmax in float32 whatever the model's dtype, so the "float64" run is float64 everywhere else
                qn = np.linalg.norm(r64["grads"][name.replace("key.bias", "query.bias")])
                assert np.linalg.norm(g) <= 1e-6 * max(qn, 1e-30), (name, np.linalg.norm(g), qn)
                continue
            for k, v in cpu_ref.summarize(name, g, full_limit=FULL_LIMIT).items():
                fx[f"{geom}/{k}"] = v
            for k, v in cpu_ref.summarize(name, r32["grads"][name], full_limit=FULL_LIMIT).items():
                fx[f"{geom}/f32/{k}"] = v
            e = np.linalg.norm((r32["grads"][name] - g).ravel()) / max(np.linalg.norm(g.ravel()), 1e-30)
            fx[f"{geom}/hf32_err/{name}"] = np.array([e])
            worst = max(worst, e)
        print(f"{geom}: recon_loss {r64['recon_loss']:.6f} (float32 run {r32['recon_loss']:.6f}), "
              f"|z - z_mask0| max {np.abs(r64['z'] - z0).max():.3f}, worst float32 gradient error {worst:.2e}")
    np.savez_compressed(a.out, **fx)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {len(fx)} arrays")


if __name__ == "__main__":
    main()
