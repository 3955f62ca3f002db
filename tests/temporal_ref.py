"""CPU restatement of the VideoMAETemporal plugin for the tests.

TEST INFRASTRUCTURE ONLY.  The reference has no temporal stage, so — like R3D-18 in oracle/cpu_ref.py —
this restates the model's DEFINITION with plain torch CPU ops, composed from the pinned pieces of
oracle/cpu_ref.py (the encoder, the sinusoid table, the pre-LN block) and two head products.  The HIP
path is checked against it; parity is UNPINNED by any reference output.

    P[b, t] = mean_s X[b, t*S + s] + sinusoid_table(T', D)[t]
    for j in range(L_t): P = vit_layer(P, "temporal.layer.{j}.")     # MLP width F_t
    z = P.flatten(1) @ encoder.weight.T + encoder.bias;  r = z @ decoder.weight.T + decoder.bias
"""
import dataclasses
import math

import torch

from oracle import cpu_ref, prng


def temporal_param_shapes(cfg, L_t, F_t, enc_out, n_out):
    """Reference-style names: the encoder's (cpu_ref.vit_param_shapes), `temporal.layer.{j}.` + an
    encoder layer's sub-names, and the head over T' * D features."""
    D = cfg.hidden_size
    T = cfg.num_frames // cfg.tubelet_size
    s = {k: v for k, v in cpu_ref.vit_param_shapes(cfg, enc_out, n_out).items() if k.startswith("video_mae.")}
    for j in range(L_t):
        p = f"temporal.layer.{j}."
        s.update({
            p + "attention.attention.query.weight": (D, D), p + "attention.attention.query.bias": (D,),
            p + "attention.attention.key.weight": (D, D),
            p + "attention.attention.value.weight": (D, D), p + "attention.attention.value.bias": (D,),
            p + "attention.output.dense.weight": (D, D), p + "attention.output.dense.bias": (D,),
            p + "intermediate.dense.weight": (F_t, D), p + "intermediate.dense.bias": (F_t,),
            p + "output.dense.weight": (D, F_t), p + "output.dense.bias": (D,),
            p + "layernorm_before.weight": (D,), p + "layernorm_before.bias": (D,),
            p + "layernorm_after.weight": (D,), p + "layernorm_after.bias": (D,),
        })
    s["encoder.weight"] = (enc_out, T * D)
    s["encoder.bias"] = (enc_out,)
    s["decoder.weight"] = (n_out * 100, enc_out)
    s["decoder.bias"] = (n_out * 100,)
    return s


def make_temporal_params(cfg, L_t, F_t, enc_out, n_out, seed=2):
    """cpu_ref.make_vit_params' recipe over temporal_param_shapes (the encoder's tensors are the very
    ones make_vit_params yields: same seed, same names)."""
    out = {}
    for name, shape in temporal_param_shapes(cfg, L_t, F_t, enc_out, n_out).items():
        if name.endswith("layernorm_before.weight") or name.endswith("layernorm_after.weight"):
            out[name] = prng.normal(seed, shape, name, std=0.1, mean=1.0)
        elif name == "encoder.weight":
            out[name] = prng.normal(seed, shape, name, std=1.0 / math.sqrt(shape[1]))
        elif name == "decoder.weight":
            out[name] = prng.normal(seed, shape, name, std=0.5 / math.sqrt(shape[1]))
        else:
            out[name] = prng.normal(seed, shape, name, std=0.02)
    return out


def temporal_forward(pixels, P, cfg, L_t, F_t, freeze_encoder, mm=None):
    """log-rates (B, 100, n).  `mm` (e.g. cpu_ref.mx_matmul) applies to the encoder's products only:
    the temporal blocks never run on MX-FP8."""
    B = pixels.shape[0]
    D = cfg.hidden_size
    T = cfg.num_frames // cfg.tubelet_size
    if freeze_encoder:
        with torch.no_grad():
            X = cpu_ref.videomae_encoder(pixels, P, cfg, mm)
    else:
        X = cpu_ref.videomae_encoder(pixels, P, cfg, mm)
    Pt = X.reshape(B, T, cfg.num_tokens // T, D).mean(dim=2) + cpu_ref.sinusoid_table(T, D)
    tcfg = dataclasses.replace(cfg, intermediate_size=F_t)
    for j in range(L_t):
        Pt = cpu_ref.vit_layer(Pt, P, f"temporal.layer.{j}.", tcfg)
    z = Pt.flatten(1) @ P["encoder.weight"].T + P["encoder.bias"]
    r = z @ P["decoder.weight"].T + P["decoder.bias"]
    return r.reshape(B, 100, -1)
