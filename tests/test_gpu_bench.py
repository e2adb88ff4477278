"""bench.py's plain run on one GPU (MI355X): the headline line alone (no reference decodes, no extra legs), --steps timed
steps, and --dump-outputs DIR with the last timed step's hypotheses, in utterance order -- the same hypotheses as a --full
run of the same arguments, whose every utterance is compared with the unmodified reference decoder's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
SMALL = ["--gpus", "1", "--lanes", "6", "--frames", "150", "--utts", "10"]
NAMES = ("utt_index", "utt_n_words", "utt_n_frames", "utt_score", "utt_total_scale", "utt_n_entry", "utt_status", "utt_exit_id", "words")


def bench(tmp_path, extra):
    env = dict(os.environ, TMPDIR=str(tmp_path))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True, text=True,
                       errors="ignore", timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out, full = tmp_path / "out", tmp_path / "full"
    d = bench(tmp_path, ["--steps", "3", "--warmup", "1", "--dump-outputs", str(out)])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(d)
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["full"] is False
    assert not {"identical_to_reference", "cpu_baseline", "roofline", "kernels", "scoring", "wide_beam", "ps_fwdtree"} & set(d)
    # 10 utterances over 6 lanes: one queue (one decode call) per timed step, counted where the calls are made
    assert d["decode_calls_timed"] == 3
    a = {k: np.load(out / f"{k}.npy") for k in NAMES}
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["utt_index"], np.arange(10)) and not a["utt_status"].any()
    assert a["utt_n_frames"].sum() == d["config"]["frames_per_step"] and a["words"].shape == (a["utt_n_words"].sum(), 6)
    # the same arguments with --full: every utterance's -hyp / -hypseg line is the reference decoder's, and the dumped
    # hypotheses are the plain run's
    f = bench(tmp_path, ["--steps", "2", "--warmup", "1", "--full", "--no-scoring", "--no-ps", "--no-wide-beam", "--cpu-procs", "3",
                         "--dump-outputs", str(full)])
    assert f["identical_to_reference"] == {"hyp": True, "hypseg": True} and f["utterances_checked_against_reference"] == 10
    for k in NAMES:
        assert np.array_equal(np.load(full / f"{k}.npy"), a[k]), k
