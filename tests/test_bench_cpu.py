"""bench.py host logic that needs no GPU: the committed PMC figures it reports and the algorithmic-byte bookkeeping
(10 B forward + 18 B backward per token-channel; config 2 = 1.879 GB per step)."""
import json
import os

import bench


def test_algorithmic_bytes():
    assert (bench.FWD_BYTES, bench.BWD_BYTES) == (10, 18)
    units = 8 * 4096 * 2048
    assert units * (bench.FWD_BYTES + bench.BWD_BYTES) == 1_879_048_192
    assert bench.HBM_PEAK_GBPS == 8000.0


def test_committed_pmc_figures_are_consistent():
    pmc = bench.pmc_from_file()
    bwd, fwd = pmc["chunk_bwd12k_kernel"]["hbm_bytes"], pmc["chunk_fwd_kernel"]["hbm_bytes"]
    units = 8 * 4096 * 2048
    ckpt = units * 4                                   # one fp32 64x64 state per 64 tokens and head = 4 B per token-channel
    # measured traffic = algorithmic bytes + checkpoints, within 2 % (no re-reads from HBM: the second stage of a 64-token pair
    # takes its checkpoint from the L2)
    assert abs(bwd - (units * 18 + ckpt)) <= 0.02 * bwd
    assert abs(fwd - (units * 10 + ckpt)) <= 0.02 * fwd
    for k in ("chunk_bwd12k_kernel", "chunk_fwd_kernel"):
        assert 0.2 < bench.valu_issue_share_of(pmc[k]["counters"]) < 1.0
    assert bench.valu_issue_share_of({}) is None


def test_committed_bench_lines_carry_the_contract_fields():
    root = os.path.dirname(os.path.abspath(bench.__file__))
    for name in ("r06_bench_final.json", "r06_bench_driver_style.json", "r06_bench_bi.json", "r06_bench_infctx.json", "r05_bench_final.json", "r04_bench_final.json"):
        with open(os.path.join(root, "profiles", name)) as f:
            d = json.loads(f.read())
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                    "vs_baseline", "dtype", "data", "config", "roofline"):
            assert key in d, (name, key)
        r = d["roofline"]
        assert r["bound"] == "hbm" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
        assert "workload" in d["config"] and "model" not in d["config"]


def test_live_counter_rows_reduce_to_per_launch_hbm_bytes():
    """bench.pmc_live's parsing: several rows per (dispatch, counter) are summed, launches averaged, FETCH_SIZE doubled (gfx950);
    whole-pass totals are attributed by the phase markers the profiled child launches (marker, forwards, marker, backwards, marker),
    not by kernel names: a backward's own state pass carries a forward kernel's name."""
    rows = []
    kn = "void wkv6::(anonymous namespace)::chunk_bwd12k_kernel<true, 0, false>(wkv6::ScanArgs)"
    fw = "void wkv6::(anonymous namespace)::chunk_fwd_kernel<true, true, false, false>(wkv6::ScanArgs)"     # a state pass
    mk = "wkv6::(anonymous namespace)::pass_marker_kernel()"

    def add(name, disp, fetch, write, n=8):
        for _ in range(n):                                       # one row per XCD
            rows.append({"Kernel_Name": name, "Counter_Name": "FETCH_SIZE", "Dispatch_Id": str(disp), "Counter_Value": str(fetch)})
            rows.append({"Kernel_Name": name, "Counter_Name": "WRITE_SIZE", "Dispatch_Id": str(disp), "Counter_Value": str(write)})
    add(fw, 1, 7.0, 7.0)                                          # in front of the first marker: belongs to no pass
    add(mk, 2, 0.0, 0.0, n=1)
    add(fw, 3, 10.0, 20.0)                                        # forward pass
    add(mk, 4, 0.0, 0.0, n=1)
    add(fw, 5, 1.0, 2.0)                                          # the backward's state pass: backward traffic
    add(kn, 6, 100.0, 50.0)
    add(kn, 7, 100.0, 50.0)
    add(mk, 8, 0.0, 0.0, n=1)
    rows.append({"Kernel_Name": "some_torch_kernel", "Counter_Name": "FETCH_SIZE", "Dispatch_Id": "9", "Counter_Value": "9e9"})
    acc = {}
    bench.add_counter_rows(iter(rows), acc)          # a one-shot iterator, as csv.DictReader is
    out = bench.reduce_counters(acc)
    assert sorted(out) == ["_pass_bwd", "_pass_fwd", "chunk_bwd12k_kernel", "chunk_fwd_kernel"]
    assert out["chunk_bwd12k_kernel"]["counters"] == {"FETCH_SIZE": 800.0, "WRITE_SIZE": 400.0}
    assert out["chunk_bwd12k_kernel"]["hbm_bytes"] == (2 * 800 + 400) * 1024
    n = bench.PMC_CHILD_STEPS
    assert out["_pass_fwd"]["counters"] == {"FETCH_SIZE": 80.0 / n, "WRITE_SIZE": 160.0 / n}
    assert out["_pass_bwd"]["counters"] == {"FETCH_SIZE": (8.0 + 1600.0) / n, "WRITE_SIZE": (16.0 + 800.0) / n}


def test_round6_bench_line_proves_its_steady_state():
    """the committed driver-structured line (python bench.py --steps 20 --warmup 5) carries every timed step, the in-run
    clocks of the first and last timed launch and the pre-warm record; its timed window does not drift (last quarter / first quarter of the steps
    within 3 %, kernels alone), and
    its per-kernel means agree with the committed kernel statistics over the timed launches (profiles/r06_final_kernel_stats.csv) within 3 %."""
    import csv
    root = os.path.dirname(os.path.abspath(bench.__file__))
    d = json.loads(open(os.path.join(root, "profiles", "r06_bench_driver_style.json")).read())
    c = d["config"]
    assert d["steps"] == 20 and d["warmup"] == 5 and d["prewarm_converged"] and 300 <= d["prewarm_ms"] <= 2100
    assert len(c["fwd_ms_steps"]) == 20 and len(c["bwd_ms_steps"]) == 20 and len(c["fwd_kernel_ms_steps"]) == 20
    # drift over the timed window: last quarter / first quarter of the steps within 3 %; the single-step first / last ratio is reported too, but a
    # single launch jitters +-3 % in the steadiest state (profiles/r06_dvfs_transient.txt, table A), so it is held to 5 %
    assert abs(c["tail_head_ratio"] - 1.0) < 0.03 and abs(c["first_last_step_ratio"] - 1.0) < 0.05
    assert abs(sum(c["fwd_ms_steps"]) / 20 - c["fwd_ms"]) < 1e-3 and abs(sum(c["bwd_ms_steps"]) / 20 - c["bwd_ms"]) < 1e-3
    assert len(c["fwd_clock_ghz_first_last"]) == 2 and len(c["bwd_clock_ghz_first_last"]) == 2
    assert abs(c["cycles_per_group"] - c["fwd_ms"] * 1e-3 * c["fwd_clock_ghz"] * 1e9 / 64) < 2.0
    assert abs(c["cycles_per_stage"] - c["bwd_ms"] * 1e-3 * c["bwd_clock_ghz"] * 1e9 / 128) < 2.0
    with open(os.path.join(root, "profiles", "r06_final_kernel_stats.csv")) as fh:
        timed = {("fwd" if "chunk_fwd_kernel" in r["Name"] else "bwd"): float(r["AverageNs"]) * 1e-6
                 for r in csv.DictReader(fh) if r["Scope"].startswith("timed") and ("chunk_fwd_kernel" in r["Name"] or "chunk_bwd12k_kernel" in r["Name"])}
    assert abs(timed["fwd"] / c["fwd_ms"] - 1.0) < 0.03 and abs(timed["bwd"] / c["bwd_ms"] - 1.0) < 0.03, (timed, c["fwd_ms"], c["bwd_ms"])


def test_dump_outputs_stays_in_budget_and_repeats(tmp_path, monkeypatch):
    """--dump-outputs: small arrays whole and in their shape, large ones as the same seeded sample on every run, float32, within the
    byte budget in all; a None output (no gs at the headline workload) is not written."""
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 6000)
    monkeypatch.setattr(bench, "DUMP_WHOLE_ELEMS", 1000)
    g = torch.Generator().manual_seed(1)
    arrays = {"y": torch.randn(4, 256, 16, generator=g).to(torch.bfloat16), "gr": torch.randn(4, 256, 16, generator=g),
              "gu": torch.randn(4, 16, generator=g), "gs": None}
    written = [bench.dump_outputs(str(tmp_path / d), arrays) for d in ("a", "b")]
    assert written[0] == written[1] == {"y": [[4, 256, 16], 2968], "gr": [[4, 256, 16], 2968], "gu": [[4, 16], 64]}
    assert sorted(os.listdir(tmp_path / "a")) == ["gr.npy", "gu.npy", "y.npy"]
    total = 0
    for n in ("y", "gr", "gu"):
        a, b = (np.load(tmp_path / d / (n + ".npy")) for d in ("a", "b"))
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += a.nbytes
    assert total <= 4 * 6000
    assert np.array_equal(np.load(tmp_path / "a" / "gu.npy"), arrays["gu"].numpy())
    assert set(np.load(tmp_path / "a" / "y.npy").tolist()) <= set(arrays["y"].float().reshape(-1).tolist())
