"""bench.py without --full: the headline line only, and --dump-outputs writes what the timed path computed in its last step.
The benchmark runs as a child process; the dumped rows are then checked against a forward of the same seeded inputs here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_last_steps_embeddings(tmp_path):
    from gpu_util import la, model, rel_l2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--clip-seconds", "10", "--batch", "8", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 2 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"].startswith("f16x3")
    T = la.synth.conv_out_length(160000)
    assert abs(d["value"] - 8 * T / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]  # ms_per_step is one timed step
    assert not {"roofline", "kernels", "alt_precision", "two_streams", "cpu_baseline", "embed_rel_l2"} & set(d)
    assert d["config"]["cpu_baseline_sample"] == "skipped"
    rows, idx = np.load(out / "last_hidden_state.npy"), np.load(out / "last_hidden_state_index.npy")
    assert rows.dtype == np.float32 and rows.shape == (8 * T, 768)  # 3 992 rows: under DUMP_MAX_ROWS, all of them
    np.testing.assert_array_equal(idx, np.arange(8 * T, dtype=np.float64))
    m, _ = model()
    x, mask = la.synth.batch([160000] * 8)
    with torch.no_grad():
        y = m.speecht5.encoder(input_values=torch.from_numpy(x).cuda(), attention_mask=torch.from_numpy(mask).cuda()).last_hidden_state
    assert rel_l2(rows, y.reshape(-1, 768)) < 1e-6
