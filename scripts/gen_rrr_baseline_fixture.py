#!/usr/bin/env python
"""Generate tests/golden/rrr_baseline.npz: the RRR baseline's pinned outputs.

Run once, where the reference checkout, scipy and scikit-learn are importable:

    python scripts/gen_rrr_baseline_fixture.py --reference /path/to/video-spike

The method is scripts/gen_rrr_fixture.py's.  At run time the reference's src/model/rrr.py is loaded by path, and
`_std` / `_one_hot` (src/utils/utils.py) and `bits_per_spike` / `neg_log_likelihood` (src/utils/metric_utils.py)
are taken out of their modules with `ast`; scipy's gaussian_filter1d and sklearn's r2_score are used themselves;
`train_model_main` is called unmodified, with the multi-session dict for geometry M.  What joins these inside
src/train_rrr.py's main() (lines 108-236) is not a function and cannot be taken that way: it is the call sequence
below (`prepare`, `score`), the same one tests/rrr_baseline_ref.py restates.  The inputs are those of
tests/rrr_baseline_ref.py, re-derived from (seed, name) by oracle/prng.py, so the fixture holds OUTPUTS only:
per geometry the 20 closure losses, L-BFGS's n_iter and func_evals, V, and per session U, b, per-neuron bps and
r2, co_bps (pred for W only); `<geom>/perm/...` the same from a second run whose fit saw the standardised
training trials of every session in another order (the reference's own spread, the yardstick of the tests);
`smooth/<name>` scipy's gaussian_filter1d(y, 2, axis=1) of the two smoothing inputs.

Before anything is written the restatement is held to the fixture: for every key its distance to the reference's
first run must be at most 100 x the reference's spread, else the geometry is a bad choice.
"""
import argparse
import ast
import importlib.util
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
import rrr_ref as rr                     # noqa: E402
from gen_rrr_fixture import Recorder     # noqa: E402

PRED_GEOM = "W"                          # its pred is stored in full
FACTOR = 100.0


def reference_functions(reference):
    """The reference's rrr module (by path) and a namespace holding its _std, _one_hot and bits_per_spike."""
    from scipy.special import gammaln
    src = os.path.join(reference, "src")
    spec = importlib.util.spec_from_file_location("reference_rrr", os.path.join(src, "model", "rrr.py"))
    ref_rrr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_rrr)
    ns = {"np": np, "torch": torch, "gammaln": gammaln}
    for path, names in ((os.path.join(src, "utils", "metric_utils.py"), ("neg_log_likelihood", "bits_per_spike")),
                        (os.path.join(src, "utils", "utils.py"), ("_std", "_one_hot"))):
        tree = ast.parse(open(path).read(), filename=path)
        defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert len(defs) == len(names), (path, names)
        exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ref_rrr, ns


def prepared_sessions(geom, ns):
    """The train_data dict train_model_main takes, and the ground truth.  P: the preparation with the reference's
    functions and scipy's filter; W / M: the reference's _std per split pair, as utils.py's train_rrr does."""
    from scipy.ndimage import gaussian_filter1d
    g = rb.GEOMETRIES[geom]
    data = rb.make_raw(geom)

    def stats(a):
        _, mean, std = ns["_std"](a)
        return mean, std
    if "input_mod" in g:
        prepared, gt = rb.prepare(data, g["input_mod"], rb.frame_idx(geom),
                                  smooth_fn=lambda y, s: gaussian_filter1d(y, s, axis=1), one_hot=ns["_one_hot"],
                                  stats=stats)
        return prepared, gt
    prepared, gt = {}, {}
    for eid, d in data.items():
        mean_X, std_X = stats(d["X"][0])
        mean_y, std_y = stats(d["y"][0])
        X = [np.concatenate([(x - mean_X) / std_X, np.ones(x.shape[:2] + (1,))], axis=2) for x in d["X"]]
        y = [(v - mean_y) / std_y for v in d["y"]]
        prepared[eid] = {"X": X, "y": y, "setup": {"mean_X_Tv": mean_X, "std_X_Tv": std_X, "mean_y_TN": mean_y,
                                                   "std_y_TN": std_y}}
        gt[eid] = d["y"][1]
    return prepared, gt


def run(geom, ref_rrr, ns, perm=False):
    """train_model_main on a geometry's sessions (one fit), then train_rrr.py:193-224's scoring per session; with
    `perm` the fit sees the standardised training trials of every session in another order."""
    from sklearn.metrics import r2_score
    prepared, gt = prepared_sessions(geom, ns)
    train = prepared
    if perm:
        train = {}
        for eid, d in prepared.items():
            p = np.argsort(rr.prng.uniform(rb.SEED, len(d["X"][0]), f"rrrb.{geom}.{eid}.perm"))
            train[eid] = {**d, "X": [d["X"][0][p], d["X"][1]], "y": [d["y"][0][p], d["y"][1]]}
    model, _ = ref_rrr.train_model_main(train_data=train, l2=rr.L2, n_comp=rb.N_COMP, model_fname="unused", save=False)
    opt = Recorder.last
    st = opt.state[opt._params[0]]
    out = {"losses": np.array(opt.closure_losses), "n_iter": np.int64(st["n_iter"]),
           "func_evals": np.int64(st["func_evals"]), "V": model.model["V"].detach().numpy().copy()}
    for eid in prepared:
        _, _, pred = model.predict_y_fr(prepared, eid, 1)                       # train_rrr.py:193
        pred = np.clip(pred.cpu().detach().numpy(), 1e-3, None)
        held = gt[eid]
        bps_list, r2_list = [], []
        for n in range(pred.shape[2]):                                          # train_rrr.py:207-223
            bps = ns["bits_per_spike"](pred[:, :, [n]], held[:, :, [n]])
            r2_list.append(np.nanmean([r2_score(held[k, :, n], pred[k, :, n]) for k in range(pred.shape[0])]))
            bps_list.append(np.nan if np.isinf(bps) else bps)
        bps = np.array(bps_list, dtype=np.float64)
        out[eid] = {"U": model.model[f"{eid}_U"].detach().numpy().copy(),
                    "b": model.model[f"{eid}_b"].detach().numpy().astype(np.float64),
                    "bps": bps, "r2": np.array(r2_list, dtype=np.float64), "co_bps": np.float64(np.nanmean(bps)),
                    "pred": np.asarray(pred, dtype=np.float64)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VIDEO_SPIKE_REFERENCE"),
                    help="checkout of PPWangyc/video-spike (or set VIDEO_SPIKE_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rrr_baseline.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or VIDEO_SPIKE_REFERENCE) is required: RRRGD and the helpers are taken from it")
    from scipy.ndimage import gaussian_filter1d
    ref_rrr, ns = reference_functions(a.reference)
    ref_rrr.optim.LBFGS = Recorder(torch.optim.LBFGS)
    ref_rrr.get_device = lambda: torch.device("cpu")
    torch.set_num_threads(1)
    fx = {}
    for name in rb.SMOOTH_INPUTS:
        y = rb.smooth_input(name)
        fx[f"smooth/{name}"] = gaussian_filter1d(y, rb.SMOOTH_W, axis=1)
        assert fx[f"smooth/{name}"].dtype == y.dtype
        assert np.array_equal(rb.smooth(y), fx[f"smooth/{name}"]), f"the scipy-order restatement differs on {name}"
    for geom, g in rb.GEOMETRIES.items():
        one, two = run(geom, ref_rrr, ns), run(geom, ref_rrr, ns, perm=True)
        for o in (one, two):
            assert o["n_iter"] == 20 and o["func_evals"] == 20 and len(o["losses"]) == 20, (geom, o["n_iter"])
        assert one["losses"][-1] < 0.97 * one["losses"][0], one["losses"]
        for k in ("losses", "n_iter", "func_evals", "V"):
            fx[f"{geom}/{k}"], fx[f"{geom}/perm/{k}"] = one[k], two[k]
        for eid in g["sessions"]:
            nan = np.isnan(one[eid]["bps"])
            assert nan[rb.SILENT] and nan.sum() <= 3, (geom, eid, np.flatnonzero(nan))
            assert np.array_equal(nan, np.isnan(two[eid]["bps"])) and not np.isnan(one[eid]["r2"]).any()
            assert np.isfinite(one[eid]["bps"][rb.SILENT_IN_TRAIN])
            for k, v in one[eid].items():
                if k != "pred" or geom == PRED_GEOM:
                    fx[f"{geom}/{eid}/{k}"] = v
            for k, v in two[eid].items():
                if k != "pred":
                    fx[f"{geom}/perm/{eid}/{k}"] = v
            fx[f"{geom}/perm/{eid}/pred_maxdiff"] = np.float64(np.abs(one[eid]["pred"] - two[eid]["pred"]).max())
        # the spread check: the restatement against the first run, every key within FACTOR x the reference's spread
        got = rb.run(geom)
        assert got["n_iter"] == 20 and got["func_evals"] == 20
        d, s = rb.distances(got, fx, geom, label="restatement (generator)")
        bad = {k: (v, s[k]) for k, v in d.items() if not v <= FACTOR * s[k]}
        assert not bad, f"geometry {geom} is a bad choice: distance > {FACTOR} x spread for {bad}"
        print(f"{geom}: loss {one['losses'][0]:.6g} -> {one['losses'][-1]:.6g}, co_bps "
              f"{[round(float(one[e]['co_bps']), 5) for e in g['sessions']]}, spreads {s}")
    np.savez_compressed(a.out, **fx)
    size = os.path.getsize(a.out)
    assert size < 1 << 20, size
    print(f"wrote {a.out}: {size} bytes, {len(fx)} arrays")


if __name__ == "__main__":
    main()
