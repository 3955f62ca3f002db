#!/usr/bin/env python
"""Generate tests/golden/rrr.npz: the reduced-rank regression validation's pinned outputs.

Run once, where the reference checkout, scipy, scikit-learn and tqdm are importable:

    python scripts/gen_rrr_fixture.py --reference /path/to/video-spike

At run time it loads the reference's src/model/rrr.py by path (it needs numpy and torch only) and takes
`train_rrr` and `_std` out of src/utils/utils.py and `bits_per_spike` / `neg_log_likelihood` out of
src/utils/metric_utils.py with `ast` (the modules import cebra, wandb and torcheval at the top and cannot be
imported whole; oracle/gen_fixtures.py takes the metrics the same way).  The reference's `train_rrr` then runs
unmodified on the inputs of tests/rrr_ref.py, which are re-derived from (seed, name) by oracle/prng.py, so the
fixture holds OUTPUTS only.  Stored per geometry: the 20 closure losses, L-BFGS's n_iter and func_evals, the
final U, V, b, per-neuron bps and r2, co_bps, and pred for the smallest geometry.

The reference's own spread is stored too (`<geom>/perm/...`): the same quantities from a second run in which
the standardised training trials reach the fit in another order (a wrapper around `train_model_main` permutes
them; nothing else changes).  That is one sample of what float64 summation order does to this fit, the
yardstick of the tests' tolerances.
"""
import argparse
import ast
import importlib.util
import logging
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True          # never write into the reference checkout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rrr_ref as rr                     # noqa: E402

PRED_GEOM = "A"                          # the smallest geometry: its pred is stored in full


def reference_functions(reference):
    """The reference's rrr module (by path) and a namespace holding its train_rrr, _std and bits_per_spike."""
    from scipy.special import gammaln
    from sklearn.metrics import r2_score as r2_score_sklearn
    from tqdm import tqdm
    src = os.path.join(reference, "src")
    spec = importlib.util.spec_from_file_location("reference_rrr", os.path.join(src, "model", "rrr.py"))
    ref_rrr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_rrr)
    ns = {"np": np, "torch": torch, "gammaln": gammaln, "r2_score_sklearn": r2_score_sklearn, "tqdm": tqdm,
          "logger": logging.getLogger("reference"), "train_model_main": ref_rrr.train_model_main}
    for path, names in ((os.path.join(src, "utils", "metric_utils.py"), ("neg_log_likelihood", "bits_per_spike")),
                        (os.path.join(src, "utils", "utils.py"), ("_std", "train_rrr"))):
        tree = ast.parse(open(path).read(), filename=path)
        defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert len(defs) == len(names), (path, names)
        exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ref_rrr, ns


class Recorder:
    """Stands in for `optim.LBFGS` inside the reference's rrr module: the same optimiser, with every closure
    value and the final state kept."""
    last = None

    def __init__(self, real):
        self.real = real

    def __call__(self, params, *args, **kwargs):
        opt = self.real(params, *args, **kwargs)
        opt.closure_losses = []
        step = opt.step

        def recording_step(closure):
            def wrapped():
                v = closure()
                opt.closure_losses.append(float(v))
                return v
            return step(wrapped)
        opt.step = recording_step
        Recorder.last = opt
        return opt


def run(geom, ref_rrr, ns, perm=None):
    """The reference's train_rrr on a geometry; with `perm` the fit sees the standardised training trials in
    that order."""
    data = rr.make_data(geom)
    gt = data["y"][1].copy()
    real_main = ref_rrr.train_model_main

    def main_permuted(train_data, **kw):
        shuffled = {eid: {**d, "X": [d["X"][0][perm], d["X"][1]], "y": [d["y"][0][perm], d["y"][1]]}
                    for eid, d in train_data.items()}
        return real_main(train_data=shuffled, **kw)

    ns["train_model_main"] = main_permuted if perm is not None else real_main
    res = ns["train_rrr"]({geom: data})[geom]
    opt = Recorder.last
    st = opt.state[opt._params[0]]
    model = {k: v.detach().cpu().numpy() for k, v in zip(("U", "b", "V"), opt._params)}
    assert np.array_equal(res["gt"], gt)
    bps, r2 = np.array(res["bps"], dtype=np.float64), np.array(res["r2"], dtype=np.float64)
    return {"losses": np.array(opt.closure_losses), "n_iter": np.int64(st["n_iter"]),
            "func_evals": np.int64(st["func_evals"]), "U": model["U"], "V": model["V"],
            "b": model["b"].astype(np.float64), "bps": bps, "r2": r2, "co_bps": np.float64(np.nanmean(bps)),
            "pred": np.asarray(res["pred"], dtype=np.float64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VIDEO_SPIKE_REFERENCE"),
                    help="checkout of PPWangyc/video-spike (or set VIDEO_SPIKE_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rrr.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or VIDEO_SPIKE_REFERENCE) is required: train_rrr and RRRGD are taken from it")
    ref_rrr, ns = reference_functions(a.reference)
    ref_rrr.optim.LBFGS = Recorder(torch.optim.LBFGS)
    ref_rrr.get_device = lambda: torch.device("cpu")
    torch.set_num_threads(1)
    fx = {}
    for geom, g in rr.GEOMETRIES.items():
        one = run(geom, ref_rrr, ns)
        kt = g["k_train"]
        perm = np.argsort(rr.prng.uniform(rr.SEED, kt, f"rrr.{geom}.perm"))
        two = run(geom, ref_rrr, ns, perm=perm)
        # the reference runs all 20 iterations (no tolerance exit), in both orders
        for o in (one, two):
            assert o["n_iter"] == 20 and o["func_evals"] == 20 and len(o["losses"]) == 20, (geom, o["n_iter"])
        nan = np.isnan(one["bps"])
        assert nan[rr.SILENT] and nan.sum() <= 3, (geom, np.flatnonzero(nan))
        assert np.array_equal(nan, np.isnan(two["bps"])) and not np.isnan(one["r2"]).any()
        assert np.isfinite(one["bps"][rr.SILENT_IN_TRAIN])
        # something was fitted: the loss fell, and the fit beats the null model for most neurons (co_bps itself is
        # dominated by the neuron that is silent in training: its clipped rate of 1e-3 costs bits per spike)
        assert one["losses"][-1] < 0.97 * one["losses"][0] and np.nanmedian(one["bps"]) > 0, \
            (one["losses"], np.nanmedian(one["bps"]))
        for k, v in one.items():
            if k != "pred" or geom == PRED_GEOM:
                fx[f"{geom}/{k}"] = v
        for k, v in two.items():
            if k != "pred":
                fx[f"{geom}/perm/{k}"] = v
        fx[f"{geom}/perm/pred_maxdiff"] = np.float64(np.abs(one["pred"] - two["pred"]).max())
        spread = {k: float(np.nanmax(np.abs(one[k] - two[k])) / np.nanmax(np.abs(one[k])))
                  for k in ("losses", "U", "V", "bps", "r2")}
        print(f"{geom}: loss {one['losses'][0]:.6g} -> {one['losses'][-1]:.6g}, co_bps {one['co_bps']:.5f}, "
              f"median bps {np.nanmedian(one['bps']):.4f}, mean r2 {np.nanmean(one['r2']):.5f}, NaN bps at {np.flatnonzero(nan).tolist()}, "
              f"max|b| {np.abs(one['b']).max():.2e}, spread {spread}, pred {fx[f'{geom}/perm/pred_maxdiff']:.2e}")
    np.savez_compressed(a.out, **fx)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {len(fx)} arrays")


if __name__ == "__main__":
    main()
