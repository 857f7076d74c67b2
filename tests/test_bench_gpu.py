"""bench.py is self-launching: `python bench.py --gpus N` starts its own torch.distributed.run child
(the command the driver uses for the scaling runs). Rehearsed here with two ranks on the one GPU
(DCTS_BENCH_REHEARSE=1: every rank on cuda:0, the collective over gloo); a real multi-GPU box runs
the same code with one GPU per rank over RCCL."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*argv, rehearse=False):
    env = dict(os.environ, PYTHONPATH=ROOT)
    if rehearse:
        env["DCTS_BENCH_REHEARSE"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_self_launches_two_ranks():
    common = ["--batch", "16", "--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-headline"]
    one = run_bench("--gpus", "1", *common)
    two = run_bench("--gpus", "2", *common, rehearse=True)
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert two["scaling"] == "strong" and "all_gather_ms" in two and "all_gather_ms" not in one
    assert two["config"]["sharding"].startswith("layer-sharded")
    for r in (one, two):
        assert r["unit"] == "Mmaps/s" and r["roofline"]["bound"] == "hbm" and r["parity_check_rel_err"] <= 1e-4
        assert r["dead_channels_not_plus_zero"] == 0
    # two ranks share ONE GPU here, so there is no speed-up to expect; the rehearsal must stay in the
    # same ballpark as the single-rank run (it pays the gloo round trip through host memory)
    assert two["value"] >= 0.2 * one["value"]


def test_bench_u2netp_at_320():
    """BASELINE.json config 5 names a 320x320 input (the reference crops to 288)."""
    r = run_bench("--net", "u2netp", "--input-size", "320", "--batch", "2", "--steps", "3", "--warmup", "1",
                  "--full", "--no-cpu-baseline", "--no-headline")
    assert "320x320" in r["config"]["workload"] and r["roofline"]["kernel"].startswith("k_split_fused2")


def test_bench_rehearsal_with_four_ranks_and_channel_range_units():
    """`bench.py --gpus N` beyond two ranks. A one-GPU box admits at most six processes on its
    card, so the eight-rank case is rehearsed over gloo on the CPU (tests/test_distributed_cpu.py) and the
    bench itself with FOUR ranks here: VGG-16-bn has 12 hook points (< 4 per rank), so the units are channel
    ranges (bench.py cuts wide layers exactly then) and the sharded result must still pass the device-side
    Parseval check on every rank's share."""
    r = run_bench("--gpus", "4", "--net", "vgg_16_bn", "--batch", "32", "--steps", "5", "--warmup", "2",
                  "--full", "--no-cpu-baseline", "--no-headline", rehearse=True)
    assert r["n_gpus"] == 4 and r["scaling"] == "strong" and "all_gather_ms" in r
    assert r["parity_check_rel_err"] <= 1e-4 and r["dead_channels_not_plus_zero"] == 0
    assert r["config"]["load_imbalance"] <= 1.10


def test_plain_run_times_only_the_steps_and_dumps_its_outputs(tmp_path):
    """A plain run: `--steps` timed steps, a line without the --full figures, and `--dump-outputs` writes the scores and
    the last step's energies, identical from run to run; every step sees the same batch, so each score is the mean of
    its channel's energies."""
    import numpy as np
    argv = ["--gpus", "1", "--batch", "16", "--steps", "4", "--warmup", "1"]
    r = run_bench(*argv, "--dump-outputs", str(tmp_path / "a"))
    run_bench(*argv, "--dump-outputs", str(tmp_path / "b"))
    assert r["steps"] == 4 and r["ms_per_step"] > 0 and r["value"] > 0
    assert r["unit"] == "Mmaps/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
    assert not {"roofline", "headline", "cpu_baseline", "parity_check_rel_err"} & set(r)
    out = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("scores", "energy")}
    assert out["scores"].shape == (22720,) and out["energy"].shape == (16, 22720)
    for n, v in out.items():
        assert v.dtype == np.float32
        np.testing.assert_array_equal(v, np.load(tmp_path / "b" / (n + ".npy")))
    np.testing.assert_allclose(out["energy"].mean(0, dtype=np.float64), out["scores"], rtol=1e-5)
