#!/usr/bin/env python
"""Generate tests/golden/flow_features.npz: what the reference's get_optic_flow and get_rrr_data give for seeded tiny
trials.

Run once, where the reference checkout is readable (numpy and torch on the CPU are all it needs):

    python scripts/gen_flow_features_fixture.py --reference /path/to/video-spike

`get_optic_flow` (src/utils/ibl_data_utils.py) and `get_rrr_data` (src/utils/utils.py) are taken out of their
modules by name with `ast` at run time (the modules import ONE, cv2, matplotlib and more at their tops and cannot be
imported whole); no reference text is stored.  get_optic_flow runs in a namespace whose `cv2` is a stand-in:
`calcOpticalFlowFarneback` returns the next of this script's seeded synthetic fields (tests/flow_features_ref.py) and
`arrowedLine` does nothing; the dense field is an input of this project as it is of the reference's shards.  The
function computes the motion energy but does not return it: it is read off the function's own local `me` when it
returns (a profile hook; the function is not changed).  get_rrr_data runs on torch CPU tensors with tqdm as the
identity.

Per geometry g of flow_features_ref.GEOMETRIES (A: 7 flow frames of 6 x 5; B: 5 of 7 x 9; C: 11 of 1 x 1; 3 trials):
  <g>/video, <g>/flow             the inputs (uint8, float32)
  <g>/me, <g>/of, <g>/of-2d       (K, F), (K, F), (K, F, 2): the reference's outputs per trial, stacked
  <g>/med, <g>/bounds             (K, F - 1, 2), (K, 2, 2): np.median / np.percentile(., 10 | 90) of |flow| called as the
                                  reference calls them (the values it normalises / clips to)
  <g>/d_ref_me, <g>/d_ref_of      the largest distance of the reference's float32 series to the float64 restatement
rrr/batch<i>/<key>                geometry A as two loader batches
rrr/<branch>/X, rrr/y, rrr/timestamp   get_rrr_data's results for every branch of flow_features_ref.RRR_BRANCHES
"""
import argparse
import ast
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True          # never write into the reference checkout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import flow_features_ref as fr          # noqa: E402


def reference_function(reference, rel, name, ns):
    path = os.path.join(reference, *rel)
    tree = ast.parse(open(path).read(), filename=path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(defs) == 1, (path, name)
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns[name]


class FakeCv2:
    """cv2 for get_optic_flow: the flow of frame pair i is the i-th field handed in."""

    def __init__(self):
        self.fields, self.at = None, 0

    def load(self, fields):
        self.fields, self.at = fields, 0

    def calcOpticalFlowFarneback(self, prev, nxt, flow, *params):
        assert flow is None and len(params) == 7
        f = self.fields[self.at]
        self.at += 1
        return f.copy()

    def arrowedLine(self, *a, **k):
        return None


def run_optic_flow(fn, cv2, video, flow):
    """The reference's dict for one trial plus its local `me` at the return."""
    seen = {}

    def hook(frame, event, arg):
        if event == "return" and frame.f_code is fn.__code__:
            seen["me"] = np.array(frame.f_locals["me"])
    cv2.load(flow)
    sys.setprofile(hook)
    try:
        out = fn(video)
    finally:
        sys.setprofile(None)
    assert cv2.at == len(flow) and np.array_equal(out["of-video"], flow)
    return out, seen["me"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "flow_features.npz"))
    args = ap.parse_args()
    cv2 = FakeCv2()
    get_optic_flow = reference_function(args.reference, ("src", "utils", "ibl_data_utils.py"), "get_optic_flow",
                                        {"np": np, "cv2": cv2})
    get_rrr_data = reference_function(args.reference, ("src", "utils", "utils.py"), "get_rrr_data",
                                      {"np": np, "torch": torch, "tqdm": lambda it: it})
    out = {}
    for g, (K, Fp, H, W) in fr.GEOMETRIES.items():
        video, flow = fr.make_inputs(g)
        assert (flow > 0).any() and (flow < 0).any()
        res = {k: [] for k in ("me", "of", "of-2d", "med", "bounds")}
        d_me = d_of = 0.0
        for k in range(K):
            ref, me = run_optic_flow(get_optic_flow, cv2, video[k], flow[k])
            assert me.dtype == np.float32 and ref["of"].dtype == np.float32 and ref["of-2d"].dtype == np.float32
            den = fr.denominators(video[k], flow[k])
            assert min(den) > 0.05, (g, k, den)           # every min-max denominator is far from zero
            a = np.abs(flow[k])
            med = np.stack([np.median(a[..., c], axis=(1, 2)) for c in range(2)], axis=1)
            bounds = np.array([[np.percentile(a[..., c], 10), np.percentile(a[..., c], 90)] for c in range(2)])
            assert med.dtype == np.float32 and bounds.dtype == np.float32
            want = fr.flow_features(video[k], flow[k])
            # the restatement's order statistics are numpy's, bit for bit
            assert np.array_equal(want["med"], med) and np.array_equal(want["bounds"], bounds)
            assert np.array_equal(want["of-2d"], ref["of-2d"])
            d_me = max(d_me, float(np.abs(me.astype(np.float64) - want["me"]).max()))
            d_of = max(d_of, float(np.abs(ref["of"].astype(np.float64) - want["of"]).max()))
            for name, v in (("me", me), ("of", ref["of"]), ("of-2d", ref["of-2d"]), ("med", med), ("bounds", bounds)):
                res[name].append(v)
        out[f"{g}/video"], out[f"{g}/flow"] = video, flow
        for name, v in res.items():
            out[f"{g}/{name}"] = np.stack(v)
        out[f"{g}/d_ref_me"], out[f"{g}/d_ref_of"] = np.float64(d_me), np.float64(d_of)
        # ties straddle the ranks: the median's neighbours and the percentiles' are repeated values somewhere
        a = np.abs(flow)
        ties = sum(len(np.unique(a[k, f, :, :, c])) < H * W for k in range(K) for f in range(Fp) for c in range(2))
        print(f"{g}: d_ref me {d_me:.3e}, of {d_of:.3e}; frames with tied values {ties} of {K * Fp * 2}; "
              f"weights {fr.percentile_ranks(Fp * H * W, 10)[2]:.4f} / {fr.percentile_ranks(Fp * H * W, 90)[2]:.4f}")
    assert fr.percentile_ranks(11, 10)[2] == 0 and fr.percentile_ranks(11, 90)[2] == 0
    assert fr.percentile_ranks(210, 10)[2] != 0

    batches = fr.make_batches("A")
    for i, b in enumerate(batches):
        for k, v in b.items():
            out[f"rrr/batch{i}/{k}"] = v
    tb = [{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in b.items()} for b in batches]
    for mod in fr.RRR_BRANCHES:
        X, y, stamps = get_rrr_data(tb, mod)
        assert np.array_equal(np.asarray(X), fr.rrr_data(batches, mod)) and np.asarray(X).dtype == fr.rrr_data(batches, mod).dtype
        out[f"rrr/{mod}/X"] = np.asarray(X)
        out["rrr/y"], out["rrr/timestamp"] = np.asarray(y), np.asarray(stamps)
        print(f"get_rrr_data {mod}: X {np.asarray(X).shape} {np.asarray(X).dtype}")
    try:
        get_rrr_data([{k: v for k, v in tb[0].items() if k != "timestamp"}], "wheel-speed")
        raise SystemExit("the reference did not assert on a batch without a timestamp")
    except AssertionError:
        pass
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")
    assert os.path.getsize(args.out) < (1 << 20)


if __name__ == "__main__":
    main()
