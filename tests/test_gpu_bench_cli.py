"""bench.py's command line: a plain run does the timed steps only (`--full` holds the rest),
`--steps` sets the number of timed steps, `ms_per_step` and `value` agree, and `--dump-outputs`
writes the last timed step's outputs from inputs that are the same in every run."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, BATCH = 3, 1, 2


def _bench(dump_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--batch", str(BATCH), "--neurons", "16", "--dump-outputs", str(dump_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return lines[0], {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(str(dump_dir), "*.npy")))}


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _bench(tmp_path_factory.mktemp("dump_a"))


def test_plain_run_times_the_steps_and_nothing_else(plain_run):
    line, _ = plain_run
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "clips/sec" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["ms_per_step"] > 0
    # value = clips / elapsed and ms_per_step = elapsed / steps describe the same timed region (both
    # rounded to 3 decimals: ms_per_step of a ~10 ms step carries 1e-4 of rounding)
    assert line["value"] == pytest.approx(1e3 * BATCH / line["ms_per_step"], rel=1e-3)
    for k in ("roofline", "cpu_baseline", "parity", "c3", "c4"):
        assert line[k] is None, k


def test_dump_outputs_holds_the_last_steps_loss_and_parameters(plain_run):
    line, arrs = plain_run
    assert {"loss", "losses", "param_enc_flat", "param_head_flat"} <= set(arrs)
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert arrs["losses"].shape == (STEPS,) and arrs["loss"].shape == (1,)
    assert arrs["loss"][0] == arrs["losses"][-1]
    assert float(arrs["loss"][0]) == pytest.approx(line["final_loss"], abs=1e-6)    # the line rounds to 6 decimals
    assert all(np.isfinite(a).all() and a.size > 0 for a in arrs.values())
    assert float(np.abs(arrs["param_enc_flat"]).max()) > 0 and float(np.abs(arrs["param_head_flat"]).max()) > 0


def test_same_arguments_give_the_same_inputs_and_outputs(plain_run, tmp_path):
    """A second process with the same arguments starts from the same weights, clips and targets: the
    losses agree to f32 rounding of a bf16 step (1e-4; run-to-run differences come only from the
    arrival order of the bias gradients' f32 atomics, ~1e-7), and no parameter differs by more than
    AdamW can move it in the steps taken (|update| <= lr per step, lr <= 5e-5: 4 steps, 2e-4) —
    other seeds would differ by the initialisation's spread (1e-2) and by whole losses."""
    (_, a), (_, b) = plain_run, _bench(tmp_path)
    assert set(a) == set(b)
    np.testing.assert_allclose(b["losses"], a["losses"], rtol=1e-4)
    for k in a:
        if k.startswith("param_"):
            assert a[k].shape == b[k].shape
            assert float(np.abs(a[k].astype(np.float64) - b[k]).max()) <= 2e-4, k
