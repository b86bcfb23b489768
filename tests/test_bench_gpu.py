"""bench.py's own launch paths on the GPU box (the driver's contract): the multi-rank self-spawn (`--gpus N` re-executes the
script under torch.distributed.run, one process per rank) exercised with two ranks sharing the one GPU of the box over gloo
-- inference (batch sharding, no data-path collective, MAX over ranks) and training (DDP gradient all-reduce,
train_lm.py:559-563,625-628) -- and with eight ranks (inference): BASELINE configuration 3's launch shape rehearsed on one GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*flags, timeout=420):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):           # a clean single-process start: bench.py spawns the ranks itself
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "rank 0 prints exactly one JSON line:\n" + out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_spawns_two_ranks_and_reports_the_whole_job():
    line = _bench("--gpus", "2", "--dist-backend", "gloo", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--cudnn-benchmark", "0",
                  "--full")
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 16 and line["scaling"] == "weak"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "frames/s"
    # whole-job aggregate: 16 frames per step over the slowest rank's time
    assert abs(line["value"] - 16 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert "roofline" in line and "gloo" in line["config"]["parallelism"]


def test_plain_run_times_the_steps_and_dumps_the_last_outputs(tmp_path):
    """a plain run's line holds the headline fields only; --dump-outputs writes the three end points of the last timed step"""
    line = _bench("--steps", "3", "--warmup", "1", "--batch", "1", "--cudnn-benchmark", "0", "--dump-outputs", str(tmp_path))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert abs(line["value"] - 1 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert not {"roofline", "hot_path_ops", "cpu_baseline", "breakdown_ms"} & set(line)
    shapes = {"pred_rgbd_segs": (1, 22, 12288), "pred_kp_ofs": (1, 8, 12288, 3), "pred_ctr_ofs": (1, 1, 12288, 3)}
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in shapes)
    for k, shape in shapes.items():
        a = np.load(tmp_path / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), k


def test_bench_spawns_eight_ranks_on_the_one_gpu():
    """the 8-GPU launch of BASELINE configuration 3's inference half, rehearsed on one GPU: eight processes (per-rank MIOpen caches, eight
    contexts in 288 GB, batch 2 per rank to keep it short) over gloo -- spawn, sharding, barrier and MAX-over-ranks timing as the driver's
    `--gpus 8` run will exercise them"""
    line = _bench("--gpus", "8", "--dist-backend", "gloo", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--cudnn-benchmark", "0",
                  "--batch", "2", timeout=900)
    assert line["n_gpus"] == 8 and line["config"]["global_batch"] == 16 and line["scaling"] == "weak"
    assert abs(line["value"] - 16 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]


def test_bench_train_mode_wraps_ddp_on_two_ranks():
    """... and the training half: DistributedDataParallel over two ranks sharing the GPU (one frame each), gradient all-reduce every step.
    (Eight training ranks on one GPU were 173 s of MIOpen cold starts in the GPU suite; the eight-rank launch shape is covered by the
    inference test above, the gradient averaging by tests/test_multigpu_gpu.py and the gloo tests of tests/test_distributed_cpu.py.)"""
    line = _bench("--gpus", "2", "--dist-backend", "gloo", "--mode", "train", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                  "--batch", "1", "--cudnn-benchmark", "0", "--full", timeout=600)
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 2
    assert "train" in line["metric"] and line["value"] > 0
    # the per-step collective census every >1-rank training line carries (over gloo BatchNorm statistics stay per rank: no Python-side
    # collective, no second variant to time; on RCCL the same fields price SyncBatchNorm, tests/test_multigpu_gpu.py)
    extra = line["train_extra"]
    assert extra["sync_batchnorm_layers"] == 0 and extra["python_side_collectives_per_step"] == {} and "bn_variants" not in extra


def test_training_step_record_in_bf16(capsys):
    """the single-GPU training step of BASELINE configuration 3's shape (forward + backward + Adam, bs = 8, N = 12288, bf16 autocast, the
    reference's objective): the record the driver's GPU-test log carries for SURVEY 8f-3.  Measured 148 frames/s
    (profiles/r04_start_bench_train_bf16_optin.json); the floor asserted here is what round 3 had measured (110) -- a regression guard,
    not a target."""
    line = _bench("--mode", "train", "--precision", "bf16", "--steps", "4", "--warmup", "2", "--no-cpu-baseline", "--cudnn-benchmark", "0",
                  timeout=900)
    with capsys.disabled():
        print("\n[train bf16 bs=8] %.1f frames/s, %.1f ms/step" % (line["value"], line["ms_per_step"]))
    assert "train" in line["metric"] and line["config"]["global_batch"] == 8
    assert line["value"] >= 110.0, line["value"]
