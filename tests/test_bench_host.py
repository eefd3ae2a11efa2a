"""bench.py host logic on the CPU: the PMC traffic field's provenance, --dump-outputs."""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _write(root, workload, sha, rows=1_000_000_000, hbm=13.0e9):
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", f"pmc_{workload}.json"), "w") as f:
        json.dump({"rows": rows, "hbm_bytes_per_launch": hbm, "collected": "2026-10-18T00:00Z",
                   "kernel_src_sha16": sha}, f)


def test_traffic_names_its_profile_and_drops_stale_ones(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "kernel_src_sha16", lambda w: "feedfacecafebeef")
    # current profile: scaled bytes + where they came from
    _write(str(tmp_path), "project", "feedfacecafebeef")
    t, src = bench.pmc_traffic("project", 500_000_000)
    assert t == round(13.0e9 / 2)
    assert src["file"] == "profiles/pmc_project.json" and src["current"] and src["collected"]
    # collected against other kernel sources: no bytes, and it says why
    _write(str(tmp_path), "project", "0123456789abcdef")
    t, src = bench.pmc_traffic("project", 1_000_000_000)
    assert t is None and not src["current"] and "stale_reason" in src
    # many-key GROUP BY reads its own profile; a missing one is null
    t, src = bench.pmc_traffic("group", 1_000_000_000, keys=1_000_000)
    assert t is None and src["file"] is None
    r = bench.roofline(13e9, 2.0, 8e9, "k", (None, {"file": None}), "t")
    assert r["traffic"] is None and r["traffic_source"] == {"file": None} and r["frac"] == round(6500 / 8000, 4)


def test_kernel_src_sha_covers_every_family():
    shas = {w: bench.kernel_src_sha16(w) for w in bench.PMC_FAMILIES}
    assert all(len(s) == 16 for s in shas.values())
    assert len(set(shas.values())) == len(shas)  # each family hashes its own source


def test_dump_outputs_formats_and_sample(tmp_path, monkeypatch):
    """--dump-outputs: float32 stays, other types become float64; a long
    array is sampled at positions that depend only on its length; the other
    ranks' files carry their rank."""
    import numpy as np
    import torch

    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    v = torch.arange(5000, dtype=torch.float32) * 0.5
    i = torch.arange(5000, dtype=torch.int64) + (1 << 40)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"values": v, "rows": i, "count": torch.tensor([5000]), "host": (2.5, 7)})
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert list(a) == ["count.npy", "host.npy", "rows.npy", "values.npy"]
    assert a["values.npy"].dtype == np.float32 and all(a[f].dtype == np.float64 for f in a if f != "values.npy")
    assert a["count.npy"].tolist() == [5000.0] and a["host.npy"].tolist() == [2.5, 7.0]
    assert len(a["values.npy"]) == len(a["rows.npy"]) == 1000
    pos = a["rows.npy"] - float(1 << 40)  # int64 row ids are exact in float64
    assert np.array_equal(a["values.npy"], (pos * 0.5).astype(np.float32)) and (np.diff(pos) >= 0).all()
    assert 0 <= pos.min() and pos.max() < 5000 and len(np.unique(pos)) > 500
    assert all(np.array_equal(a[f], np.load(tmp_path / "b" / f)) for f in a)  # the same sample every run
    bench.dump_outputs(str(tmp_path / "c"), {"values": v}, world=4, rank=3)  # 4 ranks share the size limit
    assert os.listdir(tmp_path / "c") == ["values_rank3.npy"]
    assert len(np.load(tmp_path / "c" / "values_rank3.npy")) == 250
