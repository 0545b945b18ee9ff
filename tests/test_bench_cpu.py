"""CPU checks of bench.py's plumbing: the N-rank launcher (`--gpus N` re-executes under torch.distributed.run) and the
lookup of the committed PMC traffic summaries (profiles/).  No GPU, no oracle."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_gpus_n_without_launcher_needs_n_gpus():
    """`python bench.py --gpus 2` on a box with fewer GPUs: clear message, exit code 2 (not a silent 1-rank run)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MMG_BENCH_BACKEND")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2, (p.returncode, p.stderr[-400:])
    assert "needs 2 GPUs" in p.stderr


def test_gpus_n_reexecs_under_torch_distributed_run(monkeypatch):
    """With enough devices (here: the gloo smoke-test backend, which shares GPUs) the script starts N ranks of itself."""
    calls = []
    monkeypatch.setenv("MMG_BENCH_BACKEND", "gloo")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: calls.append((cmd, env)) or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1", "--scaling", "strong", "--workload", "c3"])
    with pytest.raises(SystemExit) as ei:
        bench.main()
    assert ei.value.code == 0 and len(calls) == 1
    cmd, env = calls[0]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    tail = cmd[cmd.index(os.path.join(REPO, "bench.py")) + 1:]
    assert tail == ["--gpus", "4", "--steps", "3", "--warmup", "1", "--scaling", "strong", "--workload", "c3"]
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_traffic_lookup_picks_the_workloads_own_file(tmp_path):
    def put(name, kernels):
        json.dump({"kernels": {k: {"traffic_bytes_corrected": v} for k, v in kernels.items()}}, open(tmp_path / name, "w"))
    put("r02_config3_pmc_hbm_traffic.json", {"k_conversation_fast2": 6100000})
    put("r02_strong_config3_pmc_hbm_traffic.json", {"k_conversation_fast2": 29900000})
    put("r02_config5_pmc_hbm_traffic.json", {"k_conversation": 17301504})
    put("r02_strong_config5_pmc_hbm_traffic.json", {"k_conv_tile": 247000000})
    d = str(tmp_path)
    assert bench.traffic_lookup("c3", "k_conversation", False, d)[0] == 6100000
    assert bench.traffic_lookup("c3", "k_conversation", True, d)[0] == 29900000
    assert bench.traffic_lookup("c5", "k_conversation", False, d)[0] == 17301504
    assert bench.traffic_lookup("c5", "k_conv_tile", True, d)[0] == 247000000
    assert bench.traffic_lookup("c5", "k_conv_tile", False, d) == (None, None)
    # a newer round's file wins; a file without the kernel falls through to the older one
    put("r03_config3_pmc_hbm_traffic.json", {"k_wgrad": 1})
    assert bench.traffic_lookup("c3", "k_conversation", False, d)[0] == 6100000
    put("r04_config3_pmc_hbm_traffic.json", {"k_conversation_fast2": 5000000})
    assert bench.traffic_lookup("c3", "k_conversation", False, d)[0] == 5000000


def test_traffic_lookup_on_the_committed_profiles():
    """The committed summaries: config 3's per-GPU shard is the ~6 MB file, not the 30 MB whole-batch one; config 5 resolves."""
    v3, src3 = bench.traffic_lookup("c3", "k_conversation", False)
    assert v3 is not None and "strong" not in src3 and v3 < 12e6
    v3s, src3s = bench.traffic_lookup("c3", "k_conversation", True)
    assert v3s is not None and "strong" in src3s and v3s > v3
    v5, _ = bench.traffic_lookup("c5", "k_conversation", False)
    assert v5 is not None


def test_rocprof_lookup_parses_the_newest_summary(tmp_path):
    def put(name, rows):
        with open(tmp_path / name, "w") as f:
            f.write('"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n')
            for n, c, tot in rows:
                f.write('"%s",%d,%d,%f,1.0,1,1,0\n' % (n, c, tot, tot / c))
    put("r04_config2_kernel_stats.csv", [("void mmg::k_conversation_fast3<256, 32, 64, 100, true>(mmg::Dims)", 100, 2600000),
                                         ("mmg::k_opt(mmg::JobTable const*)", 100, 500000)])
    put("r05_config2_kernel_stats.csv", [("void mmg::k_conversation_fast3<256, 32, 64, 100, true>(mmg::Dims)", 10, 200000),
                                         ("void mmg::k_bwd_conv_fast<256, 32, 64, 100, 30, true, true>(mmg::Dims)", 10, 150000),
                                         ("mmg::k_wgrad(mmg::JobTable const*)", 10, 100000), ("mmg::k_wreduce(mmg::JobTable const*)", 10, 30000),
                                         ("mmg::k_opt(mmg::JobTable const*)", 10, 50000), ("__amd_rocclr_copyBuffer", 7, 999999)])
    put("r05_strong_config3_kernel_stats.csv", [("mmg::k_wgrad(mmg::JobTable const*)", 10, 1000000), ("mmg::k_opt(mmg::JobTable const*)", 10, 50000)])
    r = bench.rocprof_lookup("c2", False, str(tmp_path))
    assert r["source"].endswith("r05_config2_kernel_stats.csv") and r["dominant"] == "k_conversation_fast3" and r["minibatches"] == 10
    assert abs(r["per_group"]["k_conversation"] - 20.0) < 1e-9 and abs(r["per_group"]["k_wgrad"] - 13.0) < 1e-9     # k_wgrad + k_wreduce: one launch group
    assert bench.rocprof_lookup("c3", True, str(tmp_path))["dominant"] == "k_wgrad"
    assert bench.rocprof_lookup("c3", False, str(tmp_path)) is None


def _committed_bench_lines():
    import glob
    import re
    out = []
    for f in glob.glob(os.path.join(REPO, "profiles", "r*_bench_line*.json")):
        m = re.match(r"r(\d+)_", os.path.basename(f))
        try:
            d = json.loads(open(f).read().strip().splitlines()[-1])
        except Exception:
            continue
        if m and isinstance(d.get("roofline"), dict) and d["roofline"].get("rocprof_source"):
            out.append((int(m.group(1)), f, d))
    return sorted(out)


def test_roofline_of_the_committed_bench_line_follows_from_the_committed_rocprof_summary():
    """The newest committed bench line names its dominant kernel from a committed rocprofv3 summary, and `frac_rocprof` is that
    kernel's operand bytes (the line's own `algorithmic_amount`) / the summary's per-minibatch average / peak: recomputed here
    from the CSV the line cites.  sec8d_bytes_per_minibatch is SURVEY.md 8(d)'s 4 (B F + D V + B) + 24 P."""
    lines = _committed_bench_lines()
    if not lines:
        pytest.skip("no committed bench line carries roofline.rocprof_source yet")
    _, path, d = lines[-1]
    rf = d["roofline"]
    src = os.path.join(REPO, rf["rocprof_source"])
    assert os.path.exists(src), "the line cites %s, which is not committed" % rf["rocprof_source"]
    w = "c2"
    import re
    num = re.search(r"config(\w+?)_kernel_stats", os.path.basename(src)).group(1)
    assert num == "2", "the default line is configs[1]"
    rp = bench.rocprof_lookup(w, False, os.path.dirname(src))
    assert bench.GROUP_OF[rp["dominant"]] == rf["kernel"] and rp["dominant"] == rf["rocprof_kernel"]
    us = rp["per_group"][rf["kernel"]]
    assert abs(us - rf["rocprof_avg_us"]) < 1e-6 * max(1.0, us)
    scale, peak = (1e9, bench.HBM_PEAK_GBS) if rf["bound"] == "hbm" else (1e12, bench.MFMA_F32_PEAK_TFLOPS)
    want = rf["algorithmic_amount"] / (us * 1e-6) / scale / peak
    assert abs(want - rf["frac_rocprof"]) <= 1e-9 + 1e-6 * want
    assert rf["peak"] == peak and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert rf["sec8d_bytes_per_minibatch"] == 4 * (64 * 512 + 30 * 100 + 64) + 24 * 384180
    assert abs(rf["step_frac"] - rf["sec8d_bytes_per_minibatch"] / (d["ms_per_step"] * 1e-3) / 1e9 / bench.HBM_PEAK_GBS) < 1e-9
    if rf.get("traffic") and rf["bound"] == "hbm":
        assert abs(rf["traffic_ratio"] - rf["traffic"] / rf["algorithmic_amount"]) < 1e-9
    assert "value_first_pass" in d and d["value_first_pass"] > 0


def test_sec8d_bytes_and_algorithmic_work_conventions():
    assert bench.sec8d_bytes_per_minibatch(bench.C2, 64, 384180) == 4 * (64 * 512 + 3000 + 64) + 24 * 384180      # 9.36 MB: SURVEY.md 8(d)
    # the baselines' hidden tiles (2 K floats per live row) are the implementation's tape, not algorithmic bytes
    b1 = bench.algorithmic_work("k_bwd_conv", bench.C2, 64, 3.0)[1]
    b2 = bench.algorithmic_work("k_bwd_conv", bench.C2, 64, 4.0)[1]
    per_row = (b2 - b1) / 64 / 4
    assert per_row == 2 * 256 + 6 * 32 + 13 * 64 + 30 + 100 + 16


def _gloo_line(*extra):
    """The one JSON line of `bench.py --gpus 2 --steps 4 --warmup 1 <extra>` as the driver launches it (torch.distributed.run,
    two gloo ranks of tests/bench_stub_driver.py)."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, MMG_BENCH_BACKEND="gloo", OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(REPO, "tests", "bench_stub_driver.py"), "--gpus", "2", "--steps", "4",
                        "--warmup", "1"] + list(extra),
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_n_gt_1_line_shape_under_gloo(tmp_path):
    """`bench.py --gpus 2 --full`: the weak configs[1] figure AND the strong-scaling figures of configs[2] (512) / configs[4] (2048)
    with rccl_world and per-collective us in the SAME line."""
    d = _gloo_line("--full")
    assert d["full"] is True
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["rccl_world"] == 2 and d["config"]["global_batch"] == 128
    # value = the exact --steps pass (2 ranks x 4 x 7.0 exchange steps in 4 x 70 us); the long window is reported beside it
    assert abs(d["value"] - 2 * (4 * 7.0) / (4 * 7e-5)) < 1e-6 * d["value"] and d["value_first_pass"] == d["value"]
    assert d["value_window"] == 2 * 400 * 8.0 / 2.0 and d["config"]["window"]["value"] == d["value_window"]
    assert abs(d["ms_per_step"] - 0.07) < 1e-9
    assert d["config"]["collective_us"]["grads_f32_allreduce_us"] == 22.0
    sc = d["strong_configs"]
    assert set(sc) == {"c3s", "c5s"}
    assert sc["c3s"]["global_batch"] == 512 and sc["c3s"]["per_gpu_batch"] == 256 and sc["c3s"]["scaling"] == "strong" and sc["c3s"]["rccl_world"] == 2
    assert sc["c5s"]["global_batch"] == 2048 and sc["c5s"]["per_gpu_batch"] == 1024
    assert sc["c5s"]["value_window"] == 30 * 100 * 8.0 / 2.0 and abs(sc["c5s"]["value"] - 1e5) < 1e-3 and "collective_us" in sc["c5s"]
    assert "other_configs" not in d and "cpu_baseline" not in d


def test_n_gt_1_plain_line_under_gloo():
    """A plain `bench.py --gpus 2`: the same headline from the timed steps of ONE workload run per rank (the stub leaves out
    what only --full measures, so using it would fail), and nothing of the window or the strong-scaling configs."""
    d = _gloo_line()
    assert d["full"] is False and d["n_gpus"] == 2 and d["config"]["rccl_world"] == 2 and d["config"]["global_batch"] == 128
    assert abs(d["value"] - 2 * (4 * 7.0) / (4 * 7e-5)) < 1e-6 * d["value"] and d["value_first_pass"] == d["value"]
    assert abs(d["ms_per_step"] - 0.07) < 1e-9 and d["config"]["timed_minibatches"] == 4
    assert d["config"]["collective"] == "torch.distributed.all_reduce, backend gloo"
    for k in ("value_window", "roofline", "strong_configs", "other_configs", "cpu_baseline"):
        assert k not in d, k
    assert "window" not in d["config"] and "collective_us" not in d["config"]


def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    """--dump-outputs: float64 stays float64, everything else becomes float32; past the byte limit every array keeps the same
    seeded sample of its entries, identical from run to run."""
    import numpy as np
    outs = {"a": np.arange(1000, dtype=np.float32), "b": np.linspace(0, 1, 3000), "c": np.arange(6, dtype=np.int32).reshape(2, 3)}
    n = bench.dump_outputs(outs, str(tmp_path / "full"))
    assert n == {"a": 1000, "b": 3000, "c": 6}
    a, b, c = (np.load(tmp_path / "full" / (k + ".npy")) for k in "abc")
    assert a.dtype == np.float32 and b.dtype == np.float64 and c.dtype == np.float32
    assert np.array_equal(a, outs["a"]) and np.array_equal(b, outs["b"]) and np.array_equal(c, np.arange(6))
    limit = 3 * 4096 + 8000                  # (the helper keeps 4096 bytes per array for the .npy header)
    n1 = bench.dump_outputs(outs, str(tmp_path / "s1"), limit=limit)
    n2 = bench.dump_outputs(outs, str(tmp_path / "s2"), limit=limit)
    assert n1 == n2 and 0 < n1["a"] < 1000 and 0 < n1["b"] < 3000
    assert sum(os.path.getsize(p) for p in (tmp_path / "s1").iterdir()) <= limit
    for k in "abc":
        x, y = np.load(tmp_path / "s1" / (k + ".npy")), np.load(tmp_path / "s2" / (k + ".npy"))
        assert np.array_equal(x, y)
    sa = np.load(tmp_path / "s1" / "a.npy")
    assert np.all(np.diff(sa) > 0) and set(sa.tolist()) <= set(outs["a"].tolist())     # a sorted subset of the entries


def test_dump_outputs_flag_writes_what_the_timed_steps_returned(tmp_path, monkeypatch, capsys):
    """`bench.py --steps K --dump-outputs DIR`: run_workload is asked for the outputs of exactly K timed steps, they land in DIR,
    and the line keeps ms_per_step = the timed seconds / K."""
    import numpy as np
    seen = []

    def stub(workload, steps, warmup, seed, rank, world, local_rank, strong=False, want_roofline=True, outputs=False, full=True):
        seen.append((workload, steps, warmup, outputs, full))
        CFG, B, label = bench.WORKLOADS[workload]
        return dict(workload=workload, label=label, B=B, Bg=B, cfg=CFG, collective="none (single rank)",
                    first_pass_ms_per_minibatch=0.05, first_pass_steps_per_minibatch=7.0, first_pass_ex_steps=steps * 7.0,
                    first_pass_seconds=steps * 5e-5, dist_world=1,
                    outputs={"params": np.ones(5, np.float32), "losses": np.arange(8, dtype=np.float32)} if outputs else None)

    monkeypatch.setattr(bench, "run_workload", stub)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    out = tmp_path / "dump"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "2", "--no-other-configs", "--no-cli",
                                      "--no-cpu-baseline", "--dump-outputs", str(out)])
    bench.main()
    assert seen == [("c2", 7, 2, True, False)]
    d = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert d["steps"] == 7 and abs(d["ms_per_step"] - 0.05) < 1e-9
    assert d["dump_outputs"]["entries"] == {"losses": 8, "params": 5}
    assert np.array_equal(np.load(out / "losses.npy"), np.arange(8, dtype=np.float32))
    assert np.array_equal(np.load(out / "params.npy"), np.ones(5, np.float32))


def _stubbed_main(monkeypatch, capsys, argv):
    """bench.main() with the GPU legs replaced by stubs that record their calls; returns (calls, the printed line)."""
    calls = []

    def run_workload(workload, steps, warmup, seed, rank, world, local_rank, strong=False, want_roofline=True, outputs=False, full=True):
        calls.append(("run_workload", workload, strong, full))
        CFG, B, label = bench.WORKLOADS[workload]
        Bg = bench.STRONG_GLOBAL_BATCH[workload] if strong else B
        res = dict(workload=workload, label=label, B=Bg, Bg=Bg, cfg=CFG, collective="none (single rank)",
                   first_pass_ms_per_minibatch=0.05, first_pass_steps_per_minibatch=7.0, first_pass_ex_steps=steps * 7.0,
                   first_pass_seconds=steps * 5e-5, dist_world=1, outputs=None)
        if full:
            res.update(elapsed=2.0, minibatches=steps * 10, ex_steps=steps * 80.0, sample_steps=1.0, collective_us=None,
                       window_live_rows_per_sample=8.0, roofline={"kernel": "k_game", "kernels_us": {"k_game": 40.0}} if want_roofline else None)
        return res

    def run_cli(seconds=2.0, epochs=None, dist_backend=None, log_dev=10 ** 9):
        calls.append(("run_cli", log_dev))
        return dict(cli_steps_per_s=1.0, cli_ms_per_minibatch=1.0) if log_dev >= 10 ** 9 else dict(cli_default_flags_steps_per_s=1.0)

    def cpu_baseline(seconds_budget=24.0):
        calls.append(("cpu_baseline",))
        return dict(value=100.0)

    for name, f in (("run_workload", run_workload), ("run_cli", run_cli), ("cpu_baseline", cpu_baseline)):
        monkeypatch.setattr(bench, name, f)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    bench.main()
    return calls, json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_plain_run_times_the_steps_and_nothing_else(monkeypatch, capsys):
    """`bench.py --steps N --warmup W` runs ONE workload without the post-timing passes, and no other config, CLI loop or CPU
    baseline; the headline keys keep their meaning."""
    calls, d = _stubbed_main(monkeypatch, capsys, ["--steps", "20", "--warmup", "3"])
    assert calls == [("run_workload", "c2", False, False)]
    assert d["metric"].startswith("exchange-steps/sec (whole node), 30-class Adaptive") and d["unit"] == "exchange-steps/s"
    assert abs(d["value"] - 20 * 7.0 / (20 * 5e-5)) < 1e-6 * d["value"] and abs(d["ms_per_step"] - 0.05) < 1e-12
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 20 and d["warmup"] == 3 and d["full"] is False
    for k in ("value_window", "roofline", "other_configs", "cpu_baseline", "strong_configs"):
        assert k not in d, k
    assert "window" not in d["config"] and "cli" not in d["config"]


def test_full_run_keeps_every_other_measurement(monkeypatch, capsys):
    """`--full`: the same headline, then the window and roofline of the metric's workload, the six other configs, the shipped loop
    (twice: plain and with the reference's -log_dev 1000) and the CPU baseline -- in that order, as before the option existed."""
    calls, d = _stubbed_main(monkeypatch, capsys, ["--steps", "20", "--warmup", "3", "--full"])
    assert calls == ([("run_workload", "c2", False, True)]
                     + [("run_workload", w, s, True) for w, s in (("c3", False), ("c4", False), ("c4r256", False), ("c5", False),
                                                                 ("c3", True), ("c5", True))]
                     + [("run_cli", 10 ** 9), ("run_cli", 1000), ("cpu_baseline",)])
    assert abs(d["value"] - 20 * 7.0 / (20 * 5e-5)) < 1e-6 * d["value"] and abs(d["ms_per_step"] - 0.05) < 1e-12 and d["full"] is True
    assert d["value_window"] == 20 * 80.0 / 2.0 == d["config"]["window"]["value"]
    assert d["roofline"]["kernel"] == "k_game"
    assert set(d["other_configs"]) == {"c3", "c4", "c4r256", "c5", "c3s", "c5s"}
    assert d["config"]["cli"]["cli_over_resident_window"] == 1.0 / d["value_window"]
    assert d["cpu_baseline"]["gpu_first_pass_over_cpu"] == d["value"] / 100.0
    # the --no-* switches still narrow a --full run
    calls, d = _stubbed_main(monkeypatch, capsys, ["--steps", "20", "--warmup", "3", "--full", "--no-other-configs", "--no-cli", "--no-cpu-baseline"])
    assert calls == [("run_workload", "c2", False, True)] and "value_window" in d and "other_configs" not in d
