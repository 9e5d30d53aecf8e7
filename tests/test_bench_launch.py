"""bench.py --gpus N is its own launcher: N fresh ranks started before any GPU call, one sequence each, the job's one
JSON line from rank 0 (BASELINE.json configs[4]; the split follows src/Pipeline.cpp:133-138: the keyframe is fixed at
frame 0, so sequences are independent).  The CPU tests drive bench.py's real entry with --selftest-launch (stops before the
first GPU call); the GPU test runs the whole bench with two ranks sharing the one GPU of the box."""
import json
import os
import subprocess
import sys
import time

import pytest

from edge_based_visual_odometry_amd import sharding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _clean_env():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def _json_lines(text):
    return [json.loads(l) for l in text.splitlines() if l.startswith("{")]


def test_bench_gpus_2_starts_two_ranks_by_itself():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--selftest-launch", "--dist-backend", "gloo", "--steps", "10"],
                         env=_clean_env(), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = _json_lines(out.stdout)
    assert len(lines) == 1                                   # rank 0 prints the job's ONE line
    r = lines[0]
    assert r["n_gpus"] == 2 and r["backend"] == "gloo"
    assert r["per_rank_seconds"] == [0.25, 0.5] and r["max_seconds"] == 0.5     # MAX over ranks
    assert r["value"] == 2 * 10 / 0.5                        # whole-job throughput: every rank's steps over the max
    assert r["sequences"][0] != r["sequences"][1]            # one sequence per rank


def test_four_ranks_are_pinned_to_disjoint_cores():
    """configs[4] readiness: every rank of `bench.py --gpus N` runs on its own cores (sharding.pin_rank), thread pools capped"""
    avail = sorted(os.sched_getaffinity(0))
    if len(avail) < 4:
        pytest.skip("fewer than four cores")
    out = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--selftest-launch", "--dist-backend", "gloo", "--steps", "4"],
                         env=_clean_env(), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = _json_lines(out.stdout)[0]
    assert r["n_gpus"] == 4 and r["pinned"] is True
    sets = [set(c) for c in r["rank_cpus"]]
    assert len(sets) == 4 and all(sets)
    for a in range(4):
        assert sets[a] <= set(avail)
        for b in range(a + 1, 4):
            assert not (sets[a] & sets[b]), (a, b, sets)
    assert len({len(x) for x in sets}) == 1                  # equal shares
    assert int(r["omp_num_threads"]) == len(sets[0])         # the rank's thread pools are capped to its share


def test_rank_cpu_sets_follow_the_gpus_numa_nodes(tmp_path):
    """a node with two NUMA domains, four GPUs each: ranks 0-3 share node 0's cores, ranks 4-7 node 1's, all disjoint"""
    sysfs = tmp_path
    for d in range(8):
        p = sysfs / "class" / "drm" / f"renderD{128 + d}" / "device"
        p.mkdir(parents=True)
        (p / "numa_node").write_text(f"{d // 4}\n")
    for n, cpulist in ((0, "0-15,32-47"), (1, "16-31,48-63")):
        p = sysfs / "devices" / "system" / "node" / f"node{n}"
        p.mkdir(parents=True)
        (p / "cpulist").write_text(cpulist + "\n")
    sets = sharding.rank_cpu_sets(8, 8, available=range(64), sysfs=str(sysfs))
    node0 = set(range(0, 16)) | set(range(32, 48))
    assert all(len(s) == 8 for s in sets)
    assert all(set(sets[r]) <= node0 for r in range(4)) and all(not (set(sets[r]) & node0) for r in range(4, 8))
    assert len(set().union(*map(set, sets))) == 64           # disjoint and complete
    # a cgroup that leaves 16 cores: shares shrink, still disjoint, still on the right node
    sets = sharding.rank_cpu_sets(8, 8, available=list(range(0, 8)) + list(range(16, 24)), sysfs=str(sysfs))
    assert [len(s) for s in sets] == [2] * 8 and set(sets[5]) <= set(range(16, 24))
    # no NUMA information (this container): equal contiguous shares of what is available; more ranks than cores: not pinned
    assert sharding.rank_cpu_sets(2, 1, available=range(8), sysfs=str(tmp_path / "none")) == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert sharding.rank_cpu_sets(4, 4, available=range(2), sysfs=str(tmp_path / "none")) == [None] * 4


def test_bench_under_an_external_launcher_uses_its_ranks():
    """what the driver does: torch.distributed.run sets RANK / WORLD_SIZE; bench.py must not launch again"""
    env = _clean_env()
    port = sharding.free_port()
    procs = []
    for r in range(2):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, BENCH, "--gpus", "2", "--selftest-launch", "--dist-backend", "gloo"],
                                      env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert [p.returncode for p in procs] == [0, 0], outs
    assert _json_lines(outs[0][0])[0]["n_gpus"] == 2 and _json_lines(outs[1][0]) == []


def test_bench_under_torch_distributed_run():
    """the driver's own command line for N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N"""
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(sharding.free_port()), BENCH, "--gpus", "2", "--steps", "7", "--warmup", "1",
                          "--selftest-launch", "--dist-backend", "gloo"], env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = _json_lines(out.stdout)
    assert len(lines) == 1 and lines[0]["n_gpus"] == 2 and lines[0]["value"] == 2 * 7 / 0.5


def test_gpus_must_match_world_size():
    env = dict(_clean_env(), RANK="0", LOCAL_RANK="0", WORLD_SIZE="3", MASTER_ADDR="127.0.0.1", MASTER_PORT="1")
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--selftest-launch"], env=env, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2 and "WORLD_SIZE=3" in out.stderr


def test_a_failing_rank_fails_the_job_and_ends_the_others(tmp_path):
    prog = tmp_path / "rank.py"
    prog.write_text("import os, sys, time\n"
                    "assert os.environ['WORLD_SIZE'] == '3' and os.environ['MASTER_ADDR'] == '127.0.0.1'\n"
                    "assert os.environ['LOCAL_RANK'] == os.environ['RANK']\n"
                    "if os.environ['RANK'] == '1':\n    sys.exit(7)\n"
                    "time.sleep(120)\n")
    t0 = time.monotonic()
    rc = sharding.launch_ranks(3, [sys.executable, str(prog)], env=_clean_env())
    assert rc == 7 and time.monotonic() - t0 < 60            # the sleeping ranks were ended, not waited for


def test_all_ranks_ok_returns_zero(tmp_path):
    prog = tmp_path / "ok.py"
    prog.write_text("import os\nopen(os.environ['OUT'] + os.environ['RANK'], 'w').write(os.environ['MASTER_PORT'])\n")
    assert sharding.launch_ranks(4, [sys.executable, str(prog)], env=dict(_clean_env(), OUT=str(tmp_path / "r"))) == 0
    ports = {(tmp_path / f"r{r}").read_text() for r in range(4)}
    assert len(ports) == 1                                   # one rendezvous for the job


@pytest.mark.gpu
def test_bench_gpus_2_on_one_gpu_runs_the_hot_path_on_both_ranks():
    """Two ranks share the box's one GPU (gloo for the barrier: RCCL wants a device per rank); each owns its own sequence,
    rank 0 checks its pair's known answers and prints the job's line."""
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "5", "--warmup", "1", "--streams", "2", "--full",
                          "--no-cpu-baseline", "--no-transfer-legs"], env=_clean_env(), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = _json_lines(out.stdout)
    assert len(lines) == 1
    r = lines[0]
    assert r["n_gpus"] == 2 and r["steps"] == 5 and r["scaling"] == "weak"
    assert len(r["per_rank_pairs_per_s"]) == 2 and all(v > 0 for v in r["per_rank_pairs_per_s"])
    assert r["verified"] is True
    assert abs(r["value"] - 2 * 5 / (r["ms_per_step"] * 5e-3)) < 1e-6 * r["value"]
    assert r["value"] <= sum(r["per_rank_pairs_per_s"]) * (1 + 1e-9)


@pytest.mark.gpu
def test_rccl_reductions_of_the_bench_on_the_gpu(tmp_path):
    """The collectives bench.py issues on a full node -- barrier, MAX all-reduce and all-gather of one double on the rank's own
    device through RCCL (backend "nccl") -- with the one rank this box can give them: the device-tensor path of
    sharding.max_over_ranks / gather_over_ranks, in a process of its own."""
    prog = tmp_path / "rccl.py"
    prog.write_text(
        "import os, sys\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "import torch, torch.distributed as dist\n"
        "from edge_based_visual_odometry_amd import sharding\n"
        "os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(sharding.free_port()), RANK='0', WORLD_SIZE='1')\n"
        "torch.cuda.set_device(0)\n"
        "dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))\n"
        "dist.barrier()\n"
        "t = torch.tensor([1.5], dtype=torch.float64, device='cuda:0')\n"
        "dist.all_reduce(t, op=dist.ReduceOp.MAX)\n"
        "out = [torch.zeros_like(t)]\n"
        "dist.all_gather(out, t)\n"
        "assert float(t.item()) == 1.5 and float(out[0].item()) == 1.5\n"
        "assert sharding.max_over_ranks(2.5, dist, 'cuda:0') == 2.5\n"
        "assert sharding.gather_over_ranks(3.5, dist, 'cuda:0') == [3.5]\n"
        "dist.destroy_process_group()\n"
        "print('rccl ok')\n")
    out = subprocess.run([sys.executable, str(prog)], env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "rccl ok" in out.stdout, out.stderr[-3000:]


def test_dump_outputs_and_steps_argument(tmp_path):
    """--dump-outputs writes float64 .npy files (integer lists exactly) under the 64 MB cap; --steps 0 is refused"""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_module_for_dump", BENCH)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.write_outputs(str(tmp_path / "d"), {"col_idx": np.array([0, 7, 2**31 - 1], dtype=np.int32), "keep": np.array([1, 0], np.uint8)})
    got = np.load(tmp_path / "d" / "col_idx.npy")
    assert got.dtype == np.float64 and got.tolist() == [0, 7, 2**31 - 1]
    assert np.load(tmp_path / "d" / "keep.npy").tolist() == [1.0, 0.0]
    with pytest.raises(SystemExit):
        b.write_outputs(str(tmp_path / "big"), {"x": np.zeros(b.DUMP_MAX_BYTES // 8 + 1)})
    assert not (tmp_path / "big").exists()
    out = subprocess.run([sys.executable, BENCH, "--steps", "0"], env=_clean_env(), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--steps" in out.stderr
