"""bench.py's command line: a plain run times its steps and prints its line and nothing more,
`--full` adds the sustained run, the self check and the CPU baseline, and `--dump-outputs DIR`
writes the last timed step's outputs, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench(args, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                         timeout=timeout, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout  # stdout holds the JSON line only
    return json.loads(lines[0])


def test_plain_run_switches_the_extra_legs_off():
    import bench

    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, "")
    assert a.cpu_seconds == 0 and a.sustained_steps == 0 and a.no_verify
    # the legs' own options shape them under --full and never start them without it
    a = bench.parse(["--cpu-seconds", "5", "--sustained-steps", "20"])
    assert a.cpu_seconds == 0 and a.sustained_steps == 0 and a.no_verify
    a = bench.parse(["--full"])
    assert a.cpu_seconds == 10.0 and a.sustained_steps == 200 and not a.no_verify
    a = bench.parse(["--full", "--cpu-seconds", "0", "--sustained-steps", "0", "--no-verify"])
    assert a.cpu_seconds == 0 and a.sustained_steps == 0 and a.no_verify


def test_dump_blocks_is_a_fixed_sample_within_the_budget():
    import bench

    S = 26215
    per_block = 5 * S  # RS(10,4): four parity rows and one rebuilt row
    idx = bench.dump_blocks(4096, per_block)
    assert idx == bench.dump_blocks(4096, per_block)  # seeded: the same blocks every time
    assert idx == sorted(set(idx)) and idx[0] == 0 and idx[-1] == 4095
    assert len(idx) > 2 and len(idx) * per_block * 4 <= 64 * 10**6
    assert bench.dump_blocks(16, per_block) == list(range(16))  # a small output is written whole
    big = 6 * 262144  # RS(16,4) 4 MiB: four parity rows and two rebuilt rows
    idx = bench.dump_blocks(256, big)
    assert 2 < len(idx) < 256 and len(idx) * big * 4 <= 64 * 10**6


def test_mock_dump_outputs_repeats(tmp_path):
    """Two runs of the same arguments write the same arrays (--mock: the CPU stand-in's parity),
    --steps sets the steps in the line, and the line carries ms_per_step."""
    import oracle_lib as orc

    import bench

    got = []
    for d in ("a", "b"):
        j = _bench(["--gpus", "1", "--mock", "--steps", "2", "--warmup", "0", "--dump-outputs", str(tmp_path / d)])
        assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["cpu_baseline"] is None
        assert sorted(os.listdir(tmp_path / d)) == ["parity.npy"]
        got.append(np.load(tmp_path / d / "parity.npy"))
    assert got[0].dtype == np.float32 and np.array_equal(got[0], got[1])
    k, m, S, nb = 4, 2, 4096, 8
    data = np.stack([orc.splitmix64_bytes(bench.SEED ^ b, k * S) for b in range(nb)]).reshape(nb, k, S)
    assert np.array_equal(got[0], orc.encode_fast(k, m, data).astype(np.float32))


def test_mock_full_carries_the_cpu_baseline():
    j = _bench(["--gpus", "1", "--mock", "--steps", "2", "--full", "--cpu-seconds", "0.1"])
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline"]["single_core_value"] > 0


BLOCKS = 128  # more blocks than the dump's budget holds (95 at this shape), so the sample is drawn


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """A plain run: no sustained run, no self check, no CPU baseline; value and ms_per_step
    describe the same steps; parity.npy and rebuilt.npy hold the sampled blocks' parity rows and
    rebuilt row 0, byte for byte what the CPU oracle encodes from the generator's blocks."""
    import oracle_lib as orc

    import bench

    k, m, B = 10, 4, 256 * 1024
    S = (B + k - 1) // k
    j = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--blocks", str(BLOCKS), "--settle-ms", "0",
                "--dump-outputs", str(tmp_path)])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "GiB/s" and j["dtype"] == "u8" and j["higher_is_better"]
    assert j["cpu_baseline"] is None and "sustained" not in j
    assert j["verify"] == {"verified": False, "skipped": True, "ranks_verified": 0}
    assert abs(j["value"] - BLOCKS * B / (j["ms_per_step"] * 1e-3) / 2**30) / j["value"] < 0.01
    idx = bench.dump_blocks(BLOCKS, (m + 1) * S)
    assert len(idx) < BLOCKS and j["dumped"]["blocks"] == len(idx)
    par, reb = np.load(tmp_path / "parity.npy"), np.load(tmp_path / "rebuilt.npy")
    assert par.dtype == np.float32 and par.shape == (len(idx), m, S)
    assert reb.dtype == np.float32 and reb.shape == (len(idx), 1, S)
    assert par.nbytes + reb.nbytes <= 64 * 10**6
    data = np.zeros((len(idx), k * S), dtype=np.uint8)
    for r, b in enumerate(idx):
        data[r, :B] = orc.splitmix64_bytes(bench.SEED ^ b, B)
    data = data.reshape(len(idx), k, S)
    assert np.array_equal(par, orc.encode_fast(k, m, data).astype(np.float32))
    assert np.array_equal(reb[:, 0], data[:, 0].astype(np.float32))


@pytest.mark.gpu
def test_full_run_keeps_every_leg(tmp_path):
    """--full: the sustained run, the self check and the CPU baseline as before, and the dump of
    the fused CRC words beside the rows."""
    j = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--blocks", str(BLOCKS), "--settle-ms", "0", "--full",
                "--sustained-steps", "4", "--cpu-seconds", "0.2", "--fused-crc", "--dump-outputs", str(tmp_path)])
    assert j["verify"]["verified"] and j["verify"]["ranks_verified"] == 1 and j["verify"]["crc_blocks_checked"] > 0
    assert j["sustained"]["steps"] == 4 and j["sustained"]["value"] > 0
    assert j["cpu_baseline"]["value"] > 0
    assert sorted(os.listdir(tmp_path)) == ["crc.npy", "parity.npy", "rebuilt.npy"]
    crc = np.load(tmp_path / "crc.npy")
    assert crc.dtype == np.float64 and crc.shape == (BLOCKS, 14)
