"""bench.py's command line: a plain run times exactly --steps decode tokens (also past the end of the context, where
the decode goes on from the first timed position), prints one JSON line without the --full legs, and --dump-outputs
writes the last timed step's logits and the greedy tokens.  One short run of a 2-layer model, shared by the tests."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, PROMPT, N_CTX, N_VOCAB = 20, 4, 4080, 4096, 128256   # 12 positions left: the timed steps wrap once


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bench") / "dump")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "bench.py"), "--gpus", "1", "--layers", "2", "--prompt", str(PROMPT),
        "--steps", str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", out]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), out


def test_plain_line(run):
    line, _ = run
    assert line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["ms_per_step"] > 0 and line["unit"] == "tok/s" and line["higher_is_better"] is True
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - 1) < 1e-2      # both are rounded
    assert line["config"]["gen_positions"] == [PROMPT + WARMUP, N_CTX]
    for k in ("roofline", "generate_path", "cpu_baseline"):
        assert k not in line


def test_dumped_outputs(run):
    _, out = run
    assert sorted(os.listdir(out)) == ["logits.npy", "tokens.npy"]
    logits, tokens = np.load(os.path.join(out, "logits.npy")), np.load(os.path.join(out, "tokens.npy"))
    assert logits.dtype == np.float32 and logits.shape == (N_VOCAB,) and np.isfinite(logits).all()
    assert tokens.dtype == np.float64 and tokens.shape == (STEPS,)
    assert ((tokens >= 0) & (tokens < N_VOCAB) & (tokens == np.floor(tokens))).all()
    # the last step's token is the greedy choice over the last step's logits (first index wins ties)
    assert int(tokens[-1]) == int(np.argmax(logits))
