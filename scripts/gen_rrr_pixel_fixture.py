#!/usr/bin/env python
"""Generate tests/golden/rrr_pixel.npz: the pinned outputs of the RRR baseline on raw pixels
(src/train_rrr.py, input_mod 'whisker-video').

Run once, where the reference checkout, scipy and scikit-learn are importable:

    python scripts/gen_rrr_pixel_fixture.py --reference /path/to/video-spike

The method is scripts/gen_rrr_baseline_fixture.py's, whose `reference_functions` is used: the reference's
src/model/rrr.py is loaded by path, `_std` and `bits_per_spike` are taken out of their modules with `ast`, scipy's
gaussian_filter1d and sklearn's r2_score are used themselves, and `train_model_main` is called unmodified.  The
glue of main() (the flatten of lines 98-102, lines 108-171 and 193-224) is the call sequence below.  The inputs are
those of tests/rrr_pixel_ref.py, re-derived from (seed, name) by oracle/prng.py, so the fixture holds OUTPUTS only:
`X/...` the 20 closure losses, n_iter, func_evals, U, V, b, per-neuron bps and r2, co_bps and pred of the one
session; `X/perm/...` the same from a second run whose fit saw the standardised training trials in another order
(the reference's own spread, the yardstick of the tests).

Nothing is written unless the fit took its 20 closures and the restatement (tests/rrr_pixel_ref.py) is within
100 x that spread on every key.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True          # never write into the reference checkout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rrr_baseline_ref as rb            # noqa: E402
import rrr_pixel_ref as rp               # noqa: E402
import rrr_ref as rr                     # noqa: E402
from gen_rrr_baseline_fixture import reference_functions   # noqa: E402
from gen_rrr_fixture import Recorder     # noqa: E402

FACTOR = 100.0


def run(ref_rrr, ns, perm=False):
    """The flatten, the preparation with the reference's _std and scipy's filter, train_model_main, and
    train_rrr.py:193-224's scoring; with `perm` the fit sees the standardised training trials in another order."""
    from scipy.ndimage import gaussian_filter1d
    from sklearn.metrics import r2_score

    def stats(a):
        _, mean, std = ns["_std"](a)
        return mean, std
    prepared, gt = rb.prepare(rp.flatten(rp.make_raw()), rp.INPUT_MOD, rp.frame_idx(),
                              smooth_fn=lambda y, s: gaussian_filter1d(y, s, axis=1), stats=stats)
    assert prepared[rp.EID]["X"][0].dtype == np.float64 and prepared[rp.EID]["X"][0].shape == (rp.K_TRAIN, rp.T, rp.C + 1)
    train = prepared
    if perm:
        d = prepared[rp.EID]
        p = np.argsort(rr.prng.uniform(rp.SEED, len(d["X"][0]), "rrrp.X.perm"))
        train = {rp.EID: {**d, "X": [d["X"][0][p], d["X"][1]], "y": [d["y"][0][p], d["y"][1]]}}
    model, _ = ref_rrr.train_model_main(train_data=train, l2=rr.L2, n_comp=rb.N_COMP, model_fname="unused", save=False)
    opt = Recorder.last
    st = opt.state[opt._params[0]]
    _, _, pred = model.predict_y_fr(prepared, rp.EID, 1)                        # train_rrr.py:193
    pred = np.clip(pred.cpu().detach().numpy(), 1e-3, None)
    held = gt[rp.EID]
    bps_list, r2_list = [], []
    for n in range(pred.shape[2]):                                              # train_rrr.py:207-223
        bps = ns["bits_per_spike"](pred[:, :, [n]], held[:, :, [n]])
        r2_list.append(np.nanmean([r2_score(held[k, :, n], pred[k, :, n]) for k in range(pred.shape[0])]))
        bps_list.append(np.nan if np.isinf(bps) else bps)
    bps = np.array(bps_list, dtype=np.float64)
    return {"losses": np.array(opt.closure_losses), "n_iter": np.int64(st["n_iter"]),
            "func_evals": np.int64(st["func_evals"]), "V": model.model["V"].detach().numpy().copy(),
            "U": model.model[f"{rp.EID}_U"].detach().numpy().copy(),
            "b": model.model[f"{rp.EID}_b"].detach().numpy().astype(np.float64),
            "bps": bps, "r2": np.array(r2_list, dtype=np.float64), "co_bps": np.float64(np.nanmean(bps)),
            "pred": np.asarray(pred, dtype=np.float64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VIDEO_SPIKE_REFERENCE"),
                    help="checkout of PPWangyc/video-spike (or set VIDEO_SPIKE_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rrr_pixel.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or VIDEO_SPIKE_REFERENCE) is required: RRRGD and the helpers are taken from it")
    ref_rrr, ns = reference_functions(a.reference)
    ref_rrr.optim.LBFGS = Recorder(torch.optim.LBFGS)
    ref_rrr.get_device = lambda: torch.device("cpu")
    torch.set_num_threads(1)
    # the restated uint8 statistics are numpy's, bit for bit
    x0 = rp.flatten(rp.make_raw())[rp.EID]["X"][0]
    _, mean, std = ns["_std"](x0)
    m2, s2 = rp.stats_u8(x0)
    assert mean.dtype == np.float64 and np.array_equal(mean, m2) and np.array_equal(std, s2)
    assert std[:, rp.CONSTANT_PIXEL].max() == 1e-8 and (x0[:, :, rp.SATURATED_PIXEL] == 255).mean() > 0.5
    one, two = run(ref_rrr, ns), run(ref_rrr, ns, perm=True)
    for o in (one, two):
        assert o["n_iter"] == 20 and o["func_evals"] == 20 and len(o["losses"]) == 20, o["n_iter"]
    assert one["losses"][-1] < 0.97 * one["losses"][0], one["losses"]
    nan = np.isnan(one["bps"])
    assert nan[rp.SILENT] and nan.sum() == 1 and np.array_equal(nan, np.isnan(two["bps"])), np.flatnonzero(nan)
    assert not np.isnan(one["r2"]).any()
    fx = {}
    for k, v in one.items():
        fx[f"{rp.GEOM}/{k}"] = v
    for k, v in two.items():
        if k != "pred":
            fx[f"{rp.GEOM}/perm/{k}"] = v
    fx[f"{rp.GEOM}/perm/pred_maxdiff"] = np.float64(np.abs(one["pred"] - two["pred"]).max())
    got = rp.run()
    assert got["n_iter"] == 20 and got["func_evals"] == 20
    d, s = rp.distances(got, fx, label="restatement (generator)")
    bad = {k: (v, s[k]) for k, v in d.items() if not v <= FACTOR * s[k]}
    assert not bad, f"the geometry is a bad choice: distance > {FACTOR} x spread for {bad}"
    print(f"loss {one['losses'][0]:.6g} -> {one['losses'][-1]:.6g}, co_bps {float(one['co_bps']):.5f}, spreads {s}")
    np.savez_compressed(a.out, **fx)
    size = os.path.getsize(a.out)
    assert size < 1 << 20, size
    print(f"wrote {a.out}: {size} bytes, {len(fx)} arrays")


if __name__ == "__main__":
    main()
