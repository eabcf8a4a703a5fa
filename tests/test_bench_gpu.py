"""bench.py's output contract on the GPU (the driver parses this line): one short run of the
headline workload in a child process, checked field by field.  The numbers themselves are the
bench's business; here the line's shape, its units and the roofline / traffic bookkeeping."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_contract(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
           "--pool", "240", "--prewarm-ms", "0", "--no-cpu-baseline", "--no-e2e",
           "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 1
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["dtype"] == "u8" and d["vs_baseline"] is None and d["cpu_baseline"] is None
    seg = d["config"]["frames_per_step"]
    assert seg == 120 and d["config"]["width"] == 3840 and d["config"]["height"] == 2160
    # value is the whole job's frames over the timed steps' wall time
    assert d["value"] == pytest.approx(4 * seg / (d["ms_per_step"] * 4 / 1e3), rel=1e-3)
    rl = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rl, k
    assert rl["bound"] == "hbm" and rl["unit"] == "GB/s" and rl["peak"] == 8000.0
    # both figures are rounded in the line (frac to 4 places, achieved to 0.1 GB/s): after a slow
    # first step on a cold machine frac is ~0.002, and the rounding alone is then more than 1e-3 of it
    assert rl["frac"] == pytest.approx(rl["achieved"] / rl["peak"], rel=1e-3, abs=0.5e-4 + 0.05 / rl["peak"])
    assert 0 < rl["frac"] < 1
    # a JPEG of 4K testsrc at q5 is ~320 KB (the oracle's CPU sweep agrees)
    assert 250e3 < d["mean_jpeg_bytes"] < 400e3
    # a plain run measures the headline alone: nothing that takes runs of its own
    assert d["full"] is False and d["e2e"] is None and d["segments_per_launch"] is None
    assert not any("isolated" in e["kernel"] for e in d["roofline_kernels"])
    # --dump-outputs: the last timed step's sizes and JPEG bytes as float arrays, 64 MB at most
    import numpy as np
    arrs = {f[:-4]: np.load(tmp_path / "dump" / f) for f in sorted(os.listdir(tmp_path / "dump"))}
    assert sorted(arrs) == ["jpeg_checksums", "jpeg_sample", "jpeg_sample_frames", "jpeg_sizes"]
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64e6
    sizes = arrs["jpeg_sizes"]
    assert sizes.shape == (seg,) and 250e3 < sizes.mean() < 400e3
    picked = arrs["jpeg_sample_frames"].astype(int)
    sample = arrs["jpeg_sample"]
    assert len(picked) >= 1 and sample.size == min(sizes[picked].sum(), 12 << 20)
    assert list(sample[:2]) == [0xFF, 0xD8]  # a JPEG's start-of-image marker
    n0 = int(sizes[picked[0]])  # the first sampled frame's bytes against its checksums
    assert arrs["jpeg_checksums"].shape == (seg, 2)
    assert arrs["jpeg_checksums"][picked[0], 0] == sample[:n0].astype(np.float64).sum()
