"""CPU restatement of the MAE plugin (the reference's `MAE`, src/model/vit_mae/vit_mae.py:45-94, = HF
`ViTMAEForPreTraining` plus the normalised CLS latent) for the tests.

TEST INFRASTRUCTURE ONLY.  Composed from the pinned pieces of oracle/cpu_ref.py (`vit_layer`, `layer_norm`, `im2col`)
and tests/contrast_ref.py (the 2-D sin-cos table, the bf16 rounding emulation).  It is pinned: tests/golden/mae.npz holds
the outputs of the installed HF `ViTMAEForPreTraining` (scripts/gen_mae_fixture.py) for the parameters, images and
noise defined here.

    patches[g, p] = patch_p(image g) @ W.T + b + table[1 + p]
    shuffle = argsort(noise); restore = argsort(shuffle); keep = shuffle[:, :Lk], Lk = int(P (1 - mask_ratio))
    x[g, 0] = cls + table[0];  x[g, 1 + j] = patches[g, keep[g, j]];  x = encoder blocks(x);  latent = LayerNorm(x)
    z = latent[:, 0] / |latent[:, 0]|                                    (vit_mae.py:54: no projection)
    e = latent @ We.T + be;  xd[g, 0] = e[g, 0] + tabd[0]
    xd[g, 1 + p] = (restore[g, p] < Lk ? e[g, 1 + restore[g, p]] : mask_token) + tabd[1 + p]
    logits = (LayerNorm_d(decoder blocks(xd)) @ Wp.T + bp)[:, 1:]
    recon_loss = sum_masked mean_k (logits - patchify(image))^2 / #masked

The reference's own `ViTMAE.forward` (vit_mae.py:61-94) is not run by the generator: it passes `head_mask` to
`self.vit(...)` and calls `self.forward_loss(...)`, neither of which exists in transformers 5.x.  What it computes
is `ViTMAEForPreTraining.forward`'s loss and `last_hidden_state[:, 0]`, which is what the generator takes from HF.
"""
import numpy as np
import torch

import contrast_ref as cr
from oracle import cpu_ref, prng

SEED = 21
# g1: 9 patches, 2 kept (3 encoder tokens, 10 decoder tokens); g2: 81 patches, 32 kept (33 / 82 tokens: the decoder
# sequence of the 144^2 model, 64 + an 18-row tail).  Encoder 128 wide, 2 heads (head dim 64), 2 layers, MLP 256.
GEOMETRIES = {
    "g1": {"image_size": 48, "n": 4, "mask_ratio": 0.75, "decoder_hidden_size": 64, "decoder_num_attention_heads": 2,
           "decoder_num_hidden_layers": 2, "decoder_intermediate_size": 128},
    "g2": {"image_size": 144, "n": 3, "mask_ratio": 0.6, "decoder_hidden_size": 96, "decoder_num_attention_heads": 3,
           "decoder_num_hidden_layers": 1, "decoder_intermediate_size": 192},
}
ENC = "vit_mae.vit."
DEC = "vit_mae.decoder."


def vit_cfg(geom: str) -> cpu_ref.ViTCfg:
    return cpu_ref.ViTCfg(image_size=GEOMETRIES[geom]["image_size"], patch_size=16, num_channels=1, num_frames=1,
                          tubelet_size=1, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                          intermediate_size=256, layer_norm_eps=1e-12)


def dec_cfg(geom: str) -> cpu_ref.ViTCfg:
    g = GEOMETRIES[geom]
    return cpu_ref.ViTCfg(image_size=g["image_size"], patch_size=16, num_channels=1, num_frames=1, tubelet_size=1,
                          hidden_size=g["decoder_hidden_size"], num_hidden_layers=g["decoder_num_hidden_layers"],
                          num_attention_heads=g["decoder_num_attention_heads"],
                          intermediate_size=g["decoder_intermediate_size"], layer_norm_eps=1e-12)


def num_patches(geom: str) -> int:
    return (GEOMETRIES[geom]["image_size"] // 16) ** 2


def len_keep(geom: str, mask_ratio=None) -> int:
    r = GEOMETRIES[geom]["mask_ratio"] if mask_ratio is None else mask_ratio
    return int(num_patches(geom) * (1 - r))


def model_config(geom: str, compute_dtype: str = "fp32") -> dict:
    """The plugin's config (HF ViTMAEConfig field names) of a test geometry."""
    c, g = vit_cfg(geom), GEOMETRIES[geom]
    conf = {"model_class": "MAE", "compute_dtype": compute_dtype, "image_size": c.image_size,
            "patch_size": c.patch_size, "num_channels": c.num_channels, "hidden_size": c.hidden_size,
            "num_hidden_layers": c.num_hidden_layers, "num_attention_heads": c.num_attention_heads,
            "intermediate_size": c.intermediate_size, "layer_norm_eps": c.layer_norm_eps, "norm_pix_loss": False}
    conf.update({k: v for k, v in g.items() if k.startswith("decoder_") or k == "mask_ratio"})
    return conf


def _block_shapes(p: str, D: int, F: int):
    return {p + "attention.attention.query.weight": (D, D), p + "attention.attention.query.bias": (D,),
            p + "attention.attention.key.weight": (D, D), p + "attention.attention.key.bias": (D,),
            p + "attention.attention.value.weight": (D, D), p + "attention.attention.value.bias": (D,),
            p + "attention.output.dense.weight": (D, D), p + "attention.output.dense.bias": (D,),
            p + "intermediate.dense.weight": (F, D), p + "intermediate.dense.bias": (F,),
            p + "output.dense.weight": (D, F), p + "output.dense.bias": (D,),
            p + "layernorm_before.weight": (D,), p + "layernorm_before.bias": (D,),
            p + "layernorm_after.weight": (D,), p + "layernorm_after.bias": (D,)}


def param_shapes(geom: str):
    """The reference module's trainable names (transformers 4.38 spelling); the two fixed tables are not parameters."""
    c, d = vit_cfg(geom), dec_cfg(geom)
    D, Dd = c.hidden_size, d.hidden_size
    s = {ENC + "embeddings.cls_token": (1, 1, D),
         ENC + "embeddings.patch_embeddings.projection.weight": (D, c.num_channels, c.patch_size, c.patch_size),
         ENC + "embeddings.patch_embeddings.projection.bias": (D,)}
    for i in range(c.num_hidden_layers):
        s.update(_block_shapes(f"{ENC}encoder.layer.{i}.", D, c.intermediate_size))
    s.update({ENC + "layernorm.weight": (D,), ENC + "layernorm.bias": (D,),
              DEC + "decoder_embed.weight": (Dd, D), DEC + "decoder_embed.bias": (Dd,), DEC + "mask_token": (1, 1, Dd)})
    for i in range(d.num_hidden_layers):
        s.update(_block_shapes(f"{DEC}decoder_layers.{i}.", Dd, d.intermediate_size))
    K = c.patch_size ** 2 * c.num_channels
    s.update({DEC + "decoder_norm.weight": (Dd,), DEC + "decoder_norm.bias": (Dd,),
              DEC + "decoder_pred.weight": (K, Dd), DEC + "decoder_pred.bias": (K,)})
    return s


def make_params(geom: str, seed: int = SEED):
    """Seeded weights, drawn wide as in contrast_ref.make_params (N(0, 0.1), LayerNorm gains 1 + 0.1 N): with HF's
    N(0, 0.02) the attention is close to uniform and a comparison shows little.  `key.bias` is drawn non-zero: the
    restatement and the plugin ignore it, HF uses it, and the fixture shows that nothing depends on it."""
    out = {}
    for name, shape in param_shapes(geom).items():
        if name.endswith(("layernorm_before.weight", "layernorm_after.weight", "layernorm.weight", "decoder_norm.weight")):
            out[name] = prng.normal(seed, shape, name, std=0.1, mean=1.0)
        else:
            out[name] = prng.normal(seed, shape, name, std=0.1)
    return out


def make_images(geom: str, seed: int = SEED) -> np.ndarray:
    c, n = vit_cfg(geom), GEOMETRIES[geom]["n"]
    return prng.normal(seed, (n, c.num_channels, c.image_size, c.image_size), f"mae.{geom}.images")


def make_noise(geom: str, seed: int = SEED) -> np.ndarray:
    """HF's `noise` (n, P), float32 in [0, 1): a seeded permutation of the cells of a P-cell grid, each value
    jittered inside the middle half of its cell, so a row's values are at least 0.5 / P apart (81 independent
    uniform values are almost never 1e-3 apart: noise_ok)."""
    n, P = GEOMETRIES[geom]["n"], num_patches(geom)
    rank = np.argsort(prng.uniform(seed, n * P, f"mae.{geom}.noise.order").reshape(n, P), axis=1)
    cell = np.argsort(rank, axis=1).astype(np.float64)
    jitter = prng.uniform(seed, n * P, f"mae.{geom}.noise.jitter").reshape(n, P)
    return ((cell + 0.25 + 0.5 * jitter) / P).astype(np.float32)


def noise_ok(noise: np.ndarray, keep: int) -> bool:
    """The condition on the inputs: every row's values are at least 1e-3 apart (argsort is unambiguous, on any
    device) and every image has a masked patch."""
    s = np.sort(noise.astype(np.float64), axis=1)
    return bool(np.diff(s, axis=1).min() >= 1e-3) and keep < noise.shape[1]


def indices(noise: torch.Tensor, keep: int):
    shuffle = torch.argsort(noise, dim=1)
    restore = torch.argsort(shuffle, dim=1)
    return shuffle[:, :keep], restore


def trainable(name: str) -> bool:
    return not name.endswith("attention.attention.key.bias")


def patchify(images: torch.Tensor, patch: int) -> torch.Tensor:
    """HF's patchify: nchpwq -> n (hw) (pqc)."""
    n, c, S, _ = images.shape
    w = S // patch
    return images.reshape(n, c, w, patch, w, patch).permute(0, 2, 4, 3, 5, 1).reshape(n, w * w, patch * patch * c)


def forward(images: torch.Tensor, noise, P, geom: str, mask_ratio=None, bf16: bool = False):
    """{'z', 'latent', 'logits', 'recon_loss', 'ids_restore', 'mask'} in the dtype of `images` / P.  At mask_ratio 0
    the encoder runs on every patch in natural order and only 'z' and 'latent' are returned.  bf16: the blocks', the
    patch, the decoder_embed and the decoder_pred products through contrast_ref.bf16_matmul (rounding emulation)."""
    c, d = vit_cfg(geom), dec_cfg(geom)
    mm = cr.bf16_matmul if bf16 else (lambda a, w: a @ w.T)
    G, D, Dd, Pn = images.shape[0], c.hidden_size, d.hidden_size, num_patches(geom)
    grid = c.image_size // c.patch_size
    dt = images.dtype
    table = torch.from_numpy(_table64(D, grid)).to(dt)
    tabd = torch.from_numpy(_table64(Dd, grid)).to(dt)
    cols = cpu_ref.im2col(images[:, None], c)
    w = P[ENC + "embeddings.patch_embeddings.projection.weight"].reshape(D, -1)
    prod = cr._RoundBf16.apply(cols) @ cr._RoundBf16.apply(w).T if bf16 else cols @ w.T
    patches = (prod + P[ENC + "embeddings.patch_embeddings.projection.bias"]).reshape(G, Pn, D) + table[1:]
    keep_n = len_keep(geom, mask_ratio)
    cls = (P[ENC + "embeddings.cls_token"].reshape(1, 1, D) + table[:1]).expand(G, 1, D)
    if keep_n == Pn:
        kept, restore = patches, None
    else:
        keep, restore = indices(noise, keep_n)
        kept = torch.gather(patches, 1, keep[:, :, None].expand(G, keep_n, D))
    x = torch.cat([cls, kept], dim=1)
    for i in range(c.num_hidden_layers):
        x = cpu_ref.vit_layer(x, P, f"{ENC}encoder.layer.{i}.", c, mm=mm)
    latent = cpu_ref.layer_norm(x, P[ENC + "layernorm.weight"], P[ENC + "layernorm.bias"], c.layer_norm_eps)
    out = {"latent": latent, "z": latent[:, 0] / latent[:, 0].norm(dim=-1, keepdim=True)}
    if restore is None:
        return out
    e = mm(latent, P[DEC + "decoder_embed.weight"]) + P[DEC + "decoder_embed.bias"]
    tok = P[DEC + "mask_token"].reshape(1, 1, Dd).expand(G, Pn - keep_n, Dd)
    full = torch.gather(torch.cat([e[:, 1:], tok], dim=1), 1, restore[:, :, None].expand(G, Pn, Dd))
    xd = torch.cat([e[:, :1], full], dim=1) + tabd
    for i in range(d.num_hidden_layers):
        xd = cpu_ref.vit_layer(xd, P, f"{DEC}decoder_layers.{i}.", d, mm=mm)
    hd = cpu_ref.layer_norm(xd, P[DEC + "decoder_norm.weight"], P[DEC + "decoder_norm.bias"], d.layer_norm_eps)
    logits = (mm(hd, P[DEC + "decoder_pred.weight"]) + P[DEC + "decoder_pred.bias"])[:, 1:]
    mask = (restore >= keep_n).to(dt)
    loss = (((logits - patchify(images, c.patch_size)) ** 2).mean(-1) * mask).sum() / mask.sum()
    out.update({"logits": logits, "recon_loss": loss, "ids_restore": restore, "mask": mask})
    return out


def _table64(dim: int, grid: int) -> np.ndarray:
    """contrast_ref.sincos_2d_table before its cast to float32."""
    q = dim // 4
    omega = 1.0 / 10000.0 ** (np.arange(q, dtype=np.float64) / q)
    h = np.repeat(np.arange(grid, dtype=np.float64), grid)
    w = np.tile(np.arange(grid, dtype=np.float64), grid)
    eh, ew = h[:, None] * omega[None, :], w[:, None] * omega[None, :]
    t = np.concatenate([np.sin(ew), np.cos(ew), np.sin(eh), np.cos(eh)], axis=1)
    return np.concatenate([np.zeros((1, dim)), t], axis=0).astype(np.float32).astype(np.float64)


def to_torch(params, dtype=torch.float64, requires_grad: bool = True):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(requires_grad) for k, v in params.items()}
