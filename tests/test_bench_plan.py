"""bench.py's multi-GPU plumbing that needs no GPU: the strong-scaling partition (both assignment rules) and the refusal to
start N ranks on fewer devices."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))


def test_plan_only_reports_both_assignments():
    r = _bench("--plan-only", "--gpus", "8", "--genomes", "1", "--records", "20000")
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["ranks"] == 8 and len(d["ops_per_rank_hash"]) == 8 and len(d["ops_per_rank_lpt"]) == 8
    assert abs(sum(d["ops_per_rank_hash"]) - sum(d["ops_per_rank_lpt"])) < 1
    # 24 contigs of very different sizes over 8 ranks: the hash rule is visibly uneven, the size-aware one is not
    assert d["imbalance_max_over_mean_hash"] > 1.15 and d["imbalance_max_over_mean_lpt"] < 1.1


def test_lpt_keeps_a_target_on_one_rank():
    sys.path.insert(0, ROOT)
    from wgatools_amd import multigpu
    rng = np.random.default_rng(1)
    names, mb = multigpu.human_like_targets(3)
    tid = rng.choice(len(names), size=5000, p=mb / mb.sum())
    rec = [names[k] for k in tid]
    w = rng.integers(1, 10000, 5000)
    for rule in (multigpu.owners(rec, 5), multigpu.owners_lpt(rec, w, 5)):
        seen = {}
        for t, o in zip(rec, rule):
            assert seen.setdefault(t, int(o)) == int(o)
        assert set(int(x) for x in rule) <= set(range(5))
    per = np.bincount(multigpu.owners_lpt(rec, w, 5), weights=w, minlength=5)
    assert per.max() / per.mean() < 1.1


def test_gpus_n_without_a_launcher_refuses_missing_devices():
    r = _bench("--gpus", "2")
    assert r.returncode == 2 and "device(s) visible" in r.stderr


def test_traffic_comes_from_the_newest_rounds_counter_passes():
    """roofline.traffic is read from the committed PMC summary of the newest round whose workload and row-kernel source both
    match what bench.py is about to time; anything else must give null, never an older round's figure."""
    import glob

    sys.path.insert(0, ROOT)
    import bench

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_traffic.json")))
    assert files, "no committed counter passes"
    newest = json.load(open(files[-1]))

    class Args:
        records = newest["workload"]["records"]
        mean_ops = newest["workload"]["mean_ops"]

    class Job:
        n_ops = newest["workload"]["ops"]

    got = bench.pmc_traffic(Args, Job)
    if newest["kernel_source_sha"] == bench.kernel_source_sha():
        assert got == newest["hbm_bytes_per_launch"]
        assert 1.0 <= got / (4 * Job.n_ops) < 20.0
    else:
        assert got is None or got != newest["hbm_bytes_per_launch"]
    Job.n_ops += 1
    assert bench.pmc_traffic(Args, Job) is None


def _cpu_job(n, row_bytes):
    """the attributes of pipeline.Paf2MafStatJob that bench.dump_outputs reads, as CPU tensors"""
    import torch

    class Job:
        pass

    j = Job()
    j.torch, j.n, j.out_bytes = torch, n, row_bytes
    g = torch.Generator().manual_seed(7)
    j.out = torch.randint(0, 256, (row_bytes + 64,), dtype=torch.uint8, generator=g)
    j.counts = torch.randint(0, 1 << 40, (n, 11), dtype=torch.int64, generator=g)
    j.diag = torch.full((n, 3), -1, dtype=torch.int64)
    j.t_row_off = torch.arange(n, dtype=torch.int64) * 1000
    j.q_row_off = j.t_row_off + 500
    j.rec_off = torch.arange(n + 1, dtype=torch.int64) * 1000
    return j, j.counts.sum(0)


def test_dump_outputs_writes_the_last_steps_arrays(tmp_path):
    """--dump-outputs: every array a caller of the timed path receives, as float64 (rows as float32), within the budget; a
    batch whose per-record arrays do not fit is a seeded sample of its records; the same job gives the same files"""
    sys.path.insert(0, ROOT)
    import bench

    j, totals = _cpu_job(3000, 200_000)
    total = bench.dump_outputs(j, totals, str(tmp_path / "a"))
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(a) == {"totals", "rows_sample", "counts", "diag", "t_row_off", "q_row_off", "rec_off"}
    assert total == sum(x.nbytes for x in a.values()) <= 64 << 20
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert np.array_equal(a["counts"], j.counts.numpy().astype(np.float64))
    assert np.array_equal(a["totals"], a["counts"].sum(0)) and (a["diag"] == -1).all()
    assert np.array_equal(a["rec_off"], j.rec_off.numpy().astype(np.float64))
    rows = a["rows_sample"]
    assert rows.shape == (1024, 4096) and rows.max() <= 255
    src = j.out.numpy()
    for r in rows[:16]:      # every window is a run of consecutive row bytes
        hit = np.flatnonzero(src[: j.out_bytes - 4095] == r[0])
        assert any(np.array_equal(src[s:s + 4096], r) for s in hit)

    budget = (2 << 20) + (200 << 10)   # 3000 records do not fit beside a 1 MB rows sample (and 1 MB of slack): a sample
    bench.dump_outputs(j, totals, str(tmp_path / "b"), budget=budget, row_windows=64)
    bench.dump_outputs(j, totals, str(tmp_path / "c"), budget=budget, row_windows=64)
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sum(x.nbytes for x in b.values()) <= budget
    pick = b["record_index"].astype(np.int64)
    assert 0 < len(pick) < 3000 and np.all(np.diff(pick) > 0)
    assert np.array_equal(b["counts"], j.counts.numpy()[pick].astype(np.float64))
    assert np.array_equal(b["rec_off"], j.rec_off.numpy()[pick].astype(np.float64))
    for f in os.listdir(tmp_path / "b"):
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f))


def test_dump_outputs_is_refused_where_there_are_no_timed_steps(tmp_path):
    for mode in ("--north-star", "--plan-only"):
        r = _bench(mode, "--dump-outputs", str(tmp_path / "d"))
        assert r.returncode == 2 and "--dump-outputs" in r.stderr, (mode, r.stderr)
        assert not (tmp_path / "d").exists()
