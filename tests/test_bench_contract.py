"""bench.py's roofline bookkeeping (CPU): every kernel the encoder launches is priced against the MFMA
ceiling of the arithmetic it runs (h3: dense FP16 / 3, x6: dense BF16 / 6, bf16: dense BF16)."""
import bench


def test_kernel_peak_by_operand_planes():
    bf16, h3, x6 = bench.BF16_MFMA_PEAK_TFLOPS, bench.BF16_MFMA_PEAK_TFLOPS / 3, bench.BF16_MFMA_PEAK_TFLOPS / 6
    cases = {
        "conv1d_x6_kernel<6, 2, 2, 8, 2, false, 2, false, true>": h3,
        "conv1d_x6_kernel<6, 2, 2, 8, 1, false, 4, true, true>": bf16,
        "conv1d_x6_kernel<6, 1, 1, 8, 3, false, 1, false, false>": x6,
        "resunit_x6_kernel<6, 1, 1, 8, 2, 2>": h3,
        "resunit_x6_kernel<6, 1, 1, 8, 1, 2>": bf16,
        "resunit_rr_kernel<96, 2, 1>": h3,
        "resunit_strip_kernel<3>": h3,
        "resunit_x6_kernel<3, 1, 1, 8, 3, 2>": x6,
        "resunit_w16_kernel<3, 2, true>": x6,
        "resunit_w16_kernel<1, 2, true>": bf16,
        "lstm_seq2_x6_kernel<12, 3, 2>": x6,
        "lstm_seq2_x6_kernel<12, 2, 1>": h3,
        "pw_presplit_x6_kernel": x6,
        "pw_presplit_kernel": h3,
        "conv1d_mfma_kernel<3, 1, 4, 4, 4>": bench.FP32_MFMA_PEAK_TFLOPS,
    }
    for name, peak in cases.items():
        got = bench.kernel_peak(name)[0]
        assert abs(got - peak) < 1e-9, (name, got, peak)


def test_plain_run_is_the_headline_alone_and_full_adds_the_rest(monkeypatch):
    """Without --full every extra leg is off (kernel timer / roofline, CPU baseline, h3); --full turns them on and
    the --no-* switches still trim it."""
    import sys

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (5, 2, False, None)
    assert a.no_cpu_baseline and a.no_kernel_timer and a.no_h3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-h3", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.no_h3 and not a.no_cpu_baseline and not a.no_kernel_timer


def test_dump_outputs_float32_within_budget_and_repeatable(tmp_path, monkeypatch):
    """--dump-outputs: float32 .npy files, small arrays whole (indices exact), an array over its share as the same
    seeded sample every time, everything within the byte budget."""
    import os

    import numpy as np
    import torch

    monkeypatch.setattr(bench, "DUMP_BUDGET", 3 * bench.NPY_HEADER + 4 * (30 + 2 * 500))
    g = torch.Generator().manual_seed(0)
    outs = {"wav": torch.randn(7, 1, 301, generator=g), "codes": torch.randint(0, 8192, (1, 6, 5), generator=g),
            "vq_post": torch.randn(6, 40, 5, generator=g, dtype=torch.float64)}
    info = bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), {k: outs[k] for k in ("vq_post", "codes", "wav")})
    assert sorted(os.listdir(tmp_path / "a")) == ["codes.npy", "vq_post.npy", "wav.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BUDGET
    for name, t in outs.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)
        if info[name]["stored"] == "all":
            assert np.array_equal(a, t.float().numpy())
        else:
            assert a.shape == (500,) and info[name] == {"shape": list(t.shape), "stored": "sample of 500"}
            pos = torch.from_numpy(bench.sample_positions(t.numel(), 500))
            assert np.array_equal(a, t.reshape(-1)[pos].float().numpy())
    assert info["codes"]["stored"] == "all" and info["wav"]["stored"] == info["vq_post"]["stored"] == "sample of 500"


def test_committed_pmc_summaries_are_readable(tmp_path):
    """bench.py reads the newest profiles/*pmc_traffic.json for the roofline's `traffic`: every committed summary has
    the tools/pmc_summary.py layout ({"kernels": {name: {"traffic_bytes_corrected", ...}}}); a summary is used only
    when its `lib_digest` is the running library's (bc_build_digest), never for other kernel code."""
    import glob
    import json
    import os

    files = sorted(glob.glob(os.path.join(os.path.dirname(bench.__file__), "profiles", "*pmc_traffic.json")))
    assert files
    for f in files:
        d = json.load(open(f))
        assert isinstance(d.get("kernels"), dict), f
        for name, v in d["kernels"].items():
            assert "traffic_bytes_corrected" in v, (f, name)
    k = "conv1d_x6_kernel<6, 2, 2, 8, 3, false, 1, false, true>"
    for i, dig in enumerate(("a" * 64, "b" * 64)):
        (tmp_path / f"r0{i}_pmc_traffic.json").write_text(json.dumps(
            {"lib_digest": dig, "kernels": {k: {"traffic_bytes_corrected": 100.0 + i, "mfma_util": 0.5}}}))
    assert bench.pmc_traffic(k, running="a" * 64, profiles=str(tmp_path)) == (100.0, 0.5, "r00_pmc_traffic.json")
    assert bench.pmc_traffic(k, running="b" * 64, profiles=str(tmp_path))[0] == 101.0
    assert bench.pmc_traffic(k, running="c" * 64, profiles=str(tmp_path)) == (None, None, None)


def test_pmc_summary_takes_the_profiled_benchs_digest(tmp_path):
    """tools/pmc_summary.py stamps a summary with the digest the profiled bench printed in its pass logs,
    and with null when the passes disagree or a log has none -- never with the package's current library."""
    import importlib.util
    import json
    import os

    spec = importlib.util.spec_from_file_location("pmc_summary", os.path.join(bench.REPO, "tools", "pmc_summary.py"))
    ps = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ps)
    d1, d2 = "a" * 64, "b" * 64
    for p in ("FETCH_SIZE", "WRITE_SIZE", "MFMA"):
        (tmp_path / f"{p}.log").write_text("rocprof noise\n" + json.dumps({"metric": "m", "lib_digest": d1}) + "\n")
    assert ps.profiled_digest(str(tmp_path)) == d1
    (tmp_path / "MFMA.log").write_text(json.dumps({"metric": "m", "lib_digest": d2}) + "\n")
    assert ps.profiled_digest(str(tmp_path)) is None
    (tmp_path / "MFMA.log").write_text("crashed before the line\n")
    assert ps.profiled_digest(str(tmp_path)) is None
