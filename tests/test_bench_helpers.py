"""CPU: the pure-host helpers bench.py builds its line from (no device work here)."""
import json
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_attention_summary_counts_the_eleven_full_layers():
    """4·L²·64 FLOP per (sequence, head) for S = QKᵀ and PV, 12 heads, 11 full layers, over the
    time of every attention launch of the step (the CLS-only layer's time included)."""
    B, L, steps, peak = 64, 512, 10, 838.9
    per_layer = 4.0 * L * L * 64 * 12 * B
    ms_total = 18.73  # 1.873 ms per step
    a = bench.attention_summary(ms_total, 12 * steps, steps, B, L, peak, "here")
    assert a["launches_per_step"] == 12
    assert a["full_layer_algorithmic_gflop"] == round(per_layer / 1e9, 2) == 51.54
    tf = 11 * per_layer / (ms_total / steps) / 1e9
    assert a["algorithmic_tflops"] == round(tf, 2)
    assert a["frac_of_peak"] == round(tf / peak, 4)
    assert a["timing"].endswith("here")
    assert bench.attention_summary(0.0, 0, steps, B, L, peak, "here") is None


def test_single_stream_engine_is_a_config_not_the_environment(monkeypatch):
    """The roofline / attention passes build their engine with ae_config.streams = one stream
    (the product library reads no AE_* environment) and leave the environment untouched."""
    import apmc_amd.engine as eng_mod
    seen = []

    class FakeEngine:
        def __init__(self, *a, **kw):
            seen.append(kw)

    monkeypatch.setattr(eng_mod, "Engine", FakeEngine)

    class Dev:
        index = 0

    before = dict(os.environ)
    bench.single_stream_engine({}, "f32x3", Dev())
    assert seen[-1]["streams"] == "one" and not seen[-1].get("tools")
    assert dict(os.environ) == before


def test_headline_is_the_timed_steps_alone(monkeypatch):
    """The plain run's line: value and ms_per_step come from --steps timed steps of B queries
    (value · ms_per_step = 1000 · B · ranks), and no other measurement's key is in it."""
    import numpy as np

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse_args()
    assert not args.full and args.dump_outputs is None
    probs = np.linspace(0.1, 0.9, args.batch, dtype=np.float32)
    h = bench.headline(args, 1, 0.105, probs, 838.9)
    assert h["metric"] == bench.METRIC and h["unit"] == "victim queries/s"
    assert h["higher_is_better"] is True and h["dtype"].startswith("f32x3")
    assert h["steps"] == 7 and h["ms_per_step"] == 15.0
    assert h["value"] == round(7 * 64 / 0.105, 3)
    assert h["probs_checksum"] == float(np.round(probs.astype(np.float64).sum(), 6))
    assert not {"roofline", "attention", "fp32_mode", "cpu_baseline", "microbench",
                "attack"} & set(h)


def test_dump_outputs_writes_float32_arrays(tmp_path):
    """--dump-outputs: the step's [B, C] probabilities as DIR/probs.npy (one file per rank when
    there are several), float32, DIR created on demand."""
    import numpy as np

    p = np.random.default_rng(0).random((64, 1)).astype(np.float32)
    bench.dump_outputs(tmp_path / "a" / "b", p, 0, 1)
    got = np.load(tmp_path / "a" / "b" / "probs.npy")
    assert got.dtype == np.float32 and np.array_equal(got, p)
    bench.dump_outputs(tmp_path / "a" / "b", p.astype(np.float64), 1, 2)
    got = np.load(tmp_path / "a" / "b" / "probs_rank1.npy")
    assert got.dtype == np.float32 and np.array_equal(got, p)


def test_pmc_traffic_comes_from_the_newest_round():
    """roofline.traffic: the committed FETCH / WRITE summary of the newest round for the
    precision (r<round><letters>_ ordering: r4z after r4k after r3ap after r3z)."""
    import re

    def order(f):
        m = re.match(r"r(\d+)([a-z]*)_", f.name)
        return (int(m.group(1)), len(m.group(2)), m.group(2))
    split = [f for f in (ROOT / "profiles").glob("r*pmc*ffn1*.json")
             if json.loads(f.read_text()).get("precision") == "f32x3"]
    if not split:
        pytest.skip("no f32x3 PMC summary committed")
    newest = max(split, key=order)
    want = float(json.loads(newest.read_text())["hbm_bytes_per_launch"])
    assert bench.pmc_traffic_per_launch("f32x3") == want
