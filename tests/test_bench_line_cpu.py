"""The one JSON line bench.py prints must stay something the driver can capture: round 4's line grew to 21.5 KB and its head
(metric, value, roofline, cpu_baseline) fell off the front of the driver's record.  compact_line() is held here to <= 6 KB with
the contract's keys, on the largest result this repository has on file (round 4's full result) plus an 8-rank dp object."""
import importlib.util
import json
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("rr_bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _canned():
    with open(os.path.join(REPO, "profiles", "r04_bench_default.json")) as f:
        full = json.loads(f.read().strip().splitlines()[-1])
    full["f16x2_path"] = dict(full.pop("bf16x3_path"), dtype="f32 io, 2xf16 22-bit operands")
    full["n_gpus"] = 8
    full["dp"] = dict(backend="nccl", bucket_bytes=3164404, note="x" * 300,
                      allreduce_us=dict(median=61.2, min=55.0, max=140.3, calls=30),
                      rccl_ranks=[dict(rank=r, local_rank=r, device=r, name="AMD Instinct MI355X", uuid="GPU-%032x" % (r * 977),
                                       host="box-with-a-long-hostname.example") for r in range(8)])
    return full


def test_compact_line_fits_the_drivers_capture_and_keeps_the_contract_keys():
    B = _bench()
    full = _canned()
    assert len(json.dumps(full)) > 15000                   # the input really is the oversized result
    line = B.compact_line(full)
    out = json.dumps(line, separators=(",", ":"))
    assert len(out.encode()) < B.LINE_LIMIT == 6144, len(out)
    for k in B.REQUIRED_KEYS:
        assert k in line and (line[k] is not None or k == "vs_baseline"), k
    r = line["roofline"]
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "launches",
              "algorithmic_flops_per_launch", "algorithmic_bytes_per_launch"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert set(line["cpu_baseline"]) == {"value", "unit", "cores", "kind", "sample"} and line["cpu_baseline"]["kind"] in ("port", "reference")
    assert set(line["roofline_gather"]) <= set(B.ROOF_KEYS) and line["roofline_gather"]["bound"] == "hbm"
    assert line["f16x2_path"]["dtype"] != line["dtype"] and "queries_per_s" in line["f16x2_path"]
    assert set(line["presets"]) == {"listnet32", "ranknet64", "evidential600"}
    assert all(set(v) == {"value", "ms_per_step"} for v in line["presets"].values())
    assert len(line["dp"]["rccl_ranks"]) == 8 and line["config"]["workload"]
    assert "kernels" not in line and "kernels_isolated" not in line and "roofline_isolated" not in line


def test_emit_writes_the_detail_file_and_returns_the_same_short_line(tmp_path, monkeypatch, capsys):
    B = _bench()
    monkeypatch.setattr(B, "REPO", str(tmp_path))
    full = _canned()
    out = B.emit(full)
    assert len(out.encode()) < B.LINE_LIMIT and "\n" not in out
    line = json.loads(out)
    assert line["detail"] == "bench_detail.json" and line["value"] == full["value"]
    with open(tmp_path / "bench_detail.json") as f:
        detail = json.load(f)
    assert "kernels_isolated" in detail and "roofline_isolated" in detail     # nothing measured is lost: it moved
    assert "detail kernels" in capsys.readouterr().err


def test_self_launch_is_decided_before_any_gpu_call():
    """`--gpus N` without a launcher must hand over to a child torch.distributed.run BEFORE the parent touches torch.cuda."""
    src = open(os.path.join(REPO, "bench.py")).read()
    body = src[src.index("def main():"):]
    assert body.index("self_launch(args.gpus") < body.index("torch.cuda.")
    assert "os.exec" not in src and "execv" not in src


def test_write_outputs_keeps_floats_and_a_fixed_sample_above_the_limit(tmp_path):
    """--dump-outputs: every array as <name>.npy in float32 / float64; above the byte limit an array larger than its share
    keeps the same seeded, ordered sample of its elements on every run."""
    B = _bench()
    arrays = {"small": np.arange(10, dtype=np.float32), "big": np.arange(5000, dtype=np.float64).reshape(50, 100),
              "ints": np.arange(4, dtype=np.int64)}
    n = B.write_outputs(str(tmp_path / "all"), arrays)
    assert n == sum(os.path.getsize(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all"))
    assert sorted(os.listdir(tmp_path / "all")) == ["big.npy", "ints.npy", "small.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "all" / "big.npy"), arrays["big"])
    ints = np.load(tmp_path / "all" / "ints.npy")
    assert ints.dtype == np.float32 and ints.tolist() == [0, 1, 2, 3]
    samples = []
    for d in ("s1", "s2"):
        assert B.write_outputs(str(tmp_path / d), arrays, limit=3072) <= 3072
        big = np.load(tmp_path / d / "big.npy")
        assert big.dtype == np.float64 and 0 < big.size < 5000 and (np.diff(big) > 0).all()
        np.testing.assert_array_equal(np.load(tmp_path / d / "small.npy"), arrays["small"])
        samples.append(big)
    np.testing.assert_array_equal(samples[0], samples[1])
