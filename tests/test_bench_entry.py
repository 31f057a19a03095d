"""bench.py's own entry point at N = 2, exactly as a user or the driver types it
(`python bench.py --gpus 2 ...`, no launcher): bench.py must start the two ranks
itself and the printed line must describe a 2-rank job.  Runs on CPU with gloo
through the test-only --selftest hook (tiny oracle-quantised Llama, oracle
shard-local product); the greedy tokens must equal the unsharded model's."""
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO


def _run(*extra, env_extra=None, timeout=300):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([REPO, os.path.join(REPO, "tests"), env.get("PYTHONPATH", "")])
    env.pop("WORLD_SIZE", None)
    env["OMP_NUM_THREADS"] = "1"
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--selftest", "bench_selftest_hook",
                           "--steps", "4", "--warmup", "1", "--prompt", "5", *extra],
                          capture_output=True, text=True, timeout=timeout, env=env, cwd=REPO)


def _line(p):
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (p.stdout, p.stderr[-3000:])
    return json.loads(lines[0])


@pytest.mark.parametrize("extra,parallelism,gbatch", [((), "tp2-rowsplit-allgather", 1),
                                                      (("--weak",), "tp2-megatron-pair-allreduce", 2)])
def test_bench_gpus2_starts_two_ranks(extra, parallelism, gbatch):
    p = _run("--gpus", "2", *extra)
    assert p.returncode == 0, p.stderr[-4000:]
    line = _line(p)
    assert line["n_gpus"] == 2
    assert line["config"]["parallelism"] == parallelism
    assert line["config"]["global_batch"] == gbatch
    assert line["config"]["projection_groups"] == 4
    assert line["selftest"]["tokens_equal_unsharded"] is True


def test_bench_world_size_mismatch_exits_nonzero():
    """A launcher that started fewer ranks than --gpus asks for must not yield a line."""
    p = _run("--gpus", "2", env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert "WORLD_SIZE=1" in p.stderr


@pytest.mark.gpu
def test_plain_run_times_the_decode_only_and_dumps_its_outputs(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W` (one decoder layer here): N timed steps, ms_per_step
    consistent with value, none of the --full measurements, and --dump-outputs' two arrays with the
    last step's logits picking the last token of the history."""
    import numpy as np

    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--layers", "1", "--prompt", "8", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-4000:]
    line = _line(p)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "tokens/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) < 1e-3      # bs = 1: tokens/s x s/token
    for key in ("roofline", "parity", "cpu_baseline", "prefill_config4"):
        assert line[key] is None
    for key in ("decode_other_codes", "chain_roofline", "rowsplit_layer", "weak_scaling_extra"):
        assert key not in line
    logits, tokens = np.load(tmp_path / "out" / "logits.npy"), np.load(tmp_path / "out" / "tokens.npy")
    assert logits.dtype == np.float32 and logits.shape == (1, 128256) and np.isfinite(logits).all()
    assert tokens.dtype == np.float64 and tokens.shape[0] == 1
    n = 8 + 2 + 1 + 3            # prompt, the two steps before the capture, warm-up, timed
    assert tokens[0, n - 1] == logits[0].argmax() and not tokens[0, n:].any()


def test_dump_outputs_of_the_decode_loop(tmp_path, monkeypatch):
    """--dump-outputs: the decode loop hands back its last step's logits and the token history,
    dump_outputs writes them as float32 / float64 .npy, a second run writes the same arrays, and an
    array over its share of the byte budget is written as the same fixed sample each time."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    from test_distributed import _tiny_llama_4bit

    cfg, _, ref = _tiny_llama_4bit()
    steps, warmup, prompt = 4, 1, 5
    runs = []
    for d in ("a", "b"):
        outputs = {}
        _, hist = bench.decode_bench_graph(ref, cfg, steps, warmup, prompt, 1, 2, graph=False, device="cpu",
                                           outputs=outputs)
        assert set(outputs) == {"logits", "tokens"}
        assert outputs["logits"].shape == (2, cfg.vocab_size) and outputs["logits"].dtype == torch.float32
        last = prompt + warmup + steps - 1       # where the last timed step wrote its token
        assert torch.equal(outputs["logits"].argmax(-1), hist[:, last])
        assert torch.equal(outputs["tokens"], hist)
        bench.dump_outputs(str(tmp_path / d), outputs)
        runs.append({n: np.load(tmp_path / d / f"{n}.npy") for n in ("logits", "tokens")})
    assert runs[0]["logits"].dtype == np.float32 and runs[0]["tokens"].dtype == np.float64
    assert np.array_equal(runs[0]["tokens"], hist.numpy())
    for n in ("logits", "tokens"):
        assert np.array_equal(runs[0][n], runs[1][n])

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 256)   # 128 bytes per array: 32 logits, 16 tokens
    for d in ("c", "d"):
        bench.dump_outputs(str(tmp_path / d), outputs)
    small = np.load(tmp_path / "c" / "logits.npy")
    assert small.shape == (32,) and np.isin(small, runs[0]["logits"]).all()
    assert np.array_equal(small, np.load(tmp_path / "d" / "logits.npy"))
    assert sum(os.path.getsize(tmp_path / "c" / f) - 128 for f in os.listdir(tmp_path / "c")) <= 256


def test_greedy_token_is_torch_argmax():
    """The bench's two-stage greedy pick returns torch.argmax's index (the first maximal one),
    ties included, at the Llama-3 vocabulary and at a width it hands straight to argmax."""
    import torch
    sys.path.insert(0, REPO)
    from bench import greedy_token
    for seed in range(24):
        g = torch.Generator().manual_seed(seed)
        for V in (128256, 1000):
            x = torch.randn(2, 1, V, generator=g).half()
            if seed % 2:
                x = (x * 2).round().clamp(-3, 3)   # thousands of tied maxima
            assert torch.equal(greedy_token(x), x.argmax(-1))
