#!/usr/bin/env python
"""Generate tests/golden/pca.npz: the PCA video embedding's pinned inputs and outputs.

Run once, where the reference checkout and scikit-learn are importable:

    python scripts/gen_pca_fixture.py --reference /path/to/video-spike

The method is scripts/gen_rrr_baseline_fixture.py's.  The reference's `get_pca_embedding` (src/utils/utils.py) is
taken out of its module by name with `ast` at run time, into a namespace that holds numpy and sklearn's PCA (the
module imports cebra at its top and cannot be imported whole); no reference text is stored.  Per geometry of
tests/pca_ref.py the fixture holds
  <g>/video                       the synthetic uint8 video (n, t, 1, h, w)
  <g>/mean, components, singular_values, scores
                                  the exact answer: sklearn PCA(5, svd_solver='full') on the float64 pixel matrix
  <g>/ref_scores                  get_pca_embedding(video) under np.random.seed(0 .. 7): (8, n, t, 5)
  <g>/spread                      the reference's spread: its worst distance to the exact scores over the 8 seeds,
                                  max |z - Z| / max |Z|
  <g>/restatement                 the same distance for tests/pca_ref.py's subspace iteration with f32 products
and for geometry C the end-to-end RRR run on the reference's scores (tests/rrr_baseline_ref.py's restated main()
with input_mod 'pca'): C/spikes, C/idx, C/e2e/{bps, r2, co_bps} from seed 0 and C/e2e/spread/{...}, the largest
distance of the other seeds' runs to it.

Before anything is written a geometry is refused where the restatement lies further from the exact scores than the
reference does, or where the two largest |entries| of a kept component differ by less than 1e-3 relative (the sign
rule would be a coin toss).
"""
import argparse
import ast
import contextlib
import io
import os
import sys

import numpy as np

sys.dont_write_bytecode = True          # never write into the reference checkout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pca_ref as pr                     # noqa: E402
import rrr_baseline_ref as rb            # noqa: E402
import rrr_ref as rr                     # noqa: E402

SEEDS = range(8)
SIGN_MARGIN = 1e-3


def reference_function(reference):
    """The reference's get_pca_embedding, compiled from its own file into a namespace with np and sklearn's PCA."""
    from sklearn.decomposition import PCA
    path = os.path.join(reference, "src", "utils", "utils.py")
    tree = ast.parse(open(path).read(), filename=path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_pca_embedding"]
    assert len(defs) == 1, path
    ns = {"np": np, "PCA": PCA}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns["get_pca_embedding"]


def e2e(scores, spikes, idx):
    """tests/rrr_baseline_ref.py's restated main() on one session whose X are PCA scores (n, t, k)."""
    kt = pr.C_TRAIN
    data = {"C": {"X": [scores[:kt], scores[kt:]], "y": [spikes[:kt], spikes[kt:]], "setup": {}}}
    prepared, gt = rb.prepare(data, "pca", idx)
    p = prepared["C"]
    out = rb.fit({"C": (p["X"][0], p["y"][0])})
    s = rr.score(p["X"][1], out["C"]["U"], out["V"], out["C"]["b"], p["setup"]["mean_y_TN"], p["setup"]["std_y_TN"],
                 gt["C"])
    return {"bps": s["bps"], "r2": s["r2"], "co_bps": np.float64(s["co_bps"])}


def e2e_distance(a, b):
    return {"bps": rr.dist(a["bps"], b["bps"]), "r2": rr.dist(a["r2"], b["r2"]),
            "co_bps": abs(float(a["co_bps"]) - float(b["co_bps"])) / abs(float(b["co_bps"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VIDEO_SPIKE_REFERENCE"),
                    help="checkout of PPWangyc/video-spike (or set VIDEO_SPIKE_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pca.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or VIDEO_SPIKE_REFERENCE) is required: get_pca_embedding is taken from it")
    from sklearn.decomposition import PCA
    get_pca_embedding = reference_function(a.reference)
    k = pr.K_COMP
    fx = {}
    for g, (n, t, h, w) in pr.GEOMETRIES.items():
        video = pr.make_video(g)
        X = video.reshape(n * t, h * w).astype(np.float64)
        assert max(X.shape) > 500 and k < 0.8 * min(X.shape), "sklearn's 'auto' must take the randomized solver"
        full = PCA(n_components=k, svd_solver="full")
        Z = full.fit_transform(X)
        mine = pr.exact_pca(X, k)
        assert pr.score_distance(mine["scores"], Z) < 1e-11 and np.allclose(mine["components"], full.components_,
                                                                           rtol=0, atol=1e-11)
        margin = pr.sign_margin(full.components_)
        assert (margin >= SIGN_MARGIN).all(), f"geometry {g}: the sign of a component is a coin toss ({margin})"
        ref = []
        for seed in SEEDS:
            np.random.seed(seed)
            with contextlib.redirect_stdout(io.StringIO()):          # it prints the shape
                ref.append(get_pca_embedding(video, out_dim=k))
        ref = np.stack(ref)
        spread = max(pr.score_distance(z.reshape(n * t, k), Z) for z in ref)
        res = pr.subspace_pca(video.reshape(n * t, h * w), k)
        dist = pr.score_distance(res["scores"], Z)
        assert res["converged"], f"geometry {g}: the restatement did not converge ({res['history']})"
        assert dist <= spread, f"geometry {g} is a bad choice: restatement {dist:.3e} > reference spread {spread:.3e}"
        sv = full.singular_values_
        print(f"{g}: {n * t} x {h * w}, singular values {np.round(sv, 1)}, sign margins {np.round(margin, 4)}, "
              f"reference spread {spread:.3e}, restatement {dist:.3e} in {res['n_iter']} steps "
              f"(residual {res['history'][-1]:.2e})")
        fx.update({f"{g}/video": video, f"{g}/mean": full.mean_, f"{g}/components": full.components_,
                   f"{g}/singular_values": sv, f"{g}/scores": Z.reshape(n, t, k), f"{g}/ref_scores": ref,
                   f"{g}/spread": np.float64(spread), f"{g}/restatement": np.float64(dist)})
    sv = fx["B/singular_values"]
    assert abs(sv[1] - sv[2]) / sv[1] < 0.04, f"geometry B: singular values 2 and 3 must lie within 4 % ({sv})"
    # the end-to-end run on geometry C
    spikes, idx = pr.c_spikes(), pr.c_frame_idx()
    runs = [e2e(z, spikes, idx) for z in fx["C/ref_scores"]]
    assert not np.isnan(runs[0]["bps"]).any() and not np.isnan(runs[0]["r2"]).any()
    sp = {key: max(e2e_distance(r, runs[0])[key] for r in runs[1:]) for key in ("bps", "r2", "co_bps")}
    assert all(v > 0 for v in sp.values()), sp
    fx.update({"C/spikes": spikes, "C/idx": idx.astype(np.int64)})
    for key in ("bps", "r2", "co_bps"):
        fx[f"C/e2e/{key}"] = runs[0][key]
        fx[f"C/e2e/spread/{key}"] = np.float64(sp[key])
    print(f"C end to end: co_bps {float(runs[0]['co_bps']):.5f}, seed spreads {sp}")
    np.savez_compressed(a.out, **fx)
    size = os.path.getsize(a.out)
    assert size < 1 << 20, size
    print(f"wrote {a.out}: {size} bytes, {len(fx)} arrays")


if __name__ == "__main__":
    main()
