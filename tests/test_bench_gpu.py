"""bench.py on the GPU.  A plain one-GPU run with --dump-outputs (C2), and
bench.py --full in the N > 1 shape rehearsed on one GPU: two self-spawned ranks under torch.distributed.run with gloo, both
driving cuda:0, run the C4 workload strong-scaled (two 2^25-word shards), the
host_memory phase (a 1 Mi-word share per rank here) and the root-held
scatter/gather phase.  The HIP kernels run under a real process group and
every check the line carries must hold: per-step verdicts all-reduced to the
global index, outputs checked against the generated secrets and a Python
recomputation, the gathered masked words equal to one K_MASK launch over the
root's whole arrays."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps, carries everything
    beside the headline figure as skipped, and --dump-outputs writes the last
    step's outputs: the canonical secrets of the sampled words equal the
    secrets the seeded share ODOs were generated from (regenerated here), the
    masked words are canonical field elements, no MAC failure."""
    import numpy as np
    import amphora_amd as A
    from amphora_amd.spdz import TEST_PRIME, TEST_R, TEST_RINV

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    argv = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c2", "--steps", "3",
            "--warmup", "1", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    W, n = 1 << 20, 2
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False and line["verified"] is True
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 / W - 1) < 1e-9
    for k in ("pattern_probe", "host_memory", "scatter_gather", "cpu_baseline"):
        assert line[k] == {"skipped": "needs --full"}, (k, line[k])
    got = {p.name[:-4]: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert sorted(got) == ["first_fail", "masked", "sample_index", "secrets"]
    assert all(v.dtype == np.float64 for v in got.values()) and sum(v.nbytes for v in got.values()) <= 64 << 20
    idx = got["sample_index"].astype(np.int64)
    assert len(idx) > 1 << 17 and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < W
    assert got["masked"].shape == got["secrets"].shape == (len(idx), 4)
    assert got["first_fail"].tolist() == [-1.0, -1.0]
    ctx = A.Context(TEST_PRIME, TEST_R, TEST_RINV, device=0)
    _, _, plain = ctx.synth_odos(seed=2000, n=n, words=W, with_plain=True)
    want = plain.cpu().numpy()[idx].view("<u4").astype(np.float64)
    assert np.array_equal(got["secrets"], want)
    top = got["masked"][:, ::-1].astype(np.uint64)  # most significant limb first
    p_limbs = [(TEST_PRIME >> (32 * k)) & 0xFFFFFFFF for k in (3, 2, 1, 0)]
    below = np.zeros(len(idx), bool)
    tie = np.ones(len(idx), bool)
    for k in range(4):
        below |= tie & (top[:, k] < p_limbs[k])
        tie &= top[:, k] == p_limbs[k]
    assert below.all()


def test_two_rank_line_under_a_process_group():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    argv = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--same-device",
            "--full", "--steps", "5", "--warmup", "2", "--sg-steps", "1", "--sg-warmup", "0", "--host-words",
            str(1 << 20), "--host-steps", "2", "--no-cpu-baseline"]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=280, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["verified"] is True, line["verify_checks"]
    assert line["n_gpus"] == 2 and line["config"]["words_total"] == 1 << 26
    assert all(line["verify_checks"].values()) and line["verify_checks"]["all_ranks"]
    assert [p["rank"] for p in line["per_rank"]] == [0, 1]
    assert line["ranks_summary"]["pg_world_size"] == 2
    hm = line["host_memory"]
    assert hm["verified"] is True and hm["words_per_rank"] == 1 << 20
    assert hm["words_per_s"] > 0 and hm["frac_of_link"] > 0
    sg = line["scatter_gather"]
    assert sg["verified"] is True and all(sg["verify_checks"].values()), sg
