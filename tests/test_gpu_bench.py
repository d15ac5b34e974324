"""GPU: a plain bench.py run on a small shape, in process: the headline line without the --full measurements,
and --dump-outputs writing what the timed (graph-replayed) step computed, the same from run to run."""
from __future__ import annotations

import json
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

S, C, L, R, ITERS = 16, 32, 2, 2, 3
ARGV = ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", f"--size={S}", f"--channels={C}",
        f"--levels={L}", f"--radius={R}", f"--iters={ITERS}"]


def _run(monkeypatch, capsys, out):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ARGV + ["--dump-outputs", str(out)])
    bench.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_plain_run_line_and_dump(monkeypatch, capsys, tmp_path):
    import dvccorr
    from dvccorr.sharded import HipRows
    line = _run(monkeypatch, capsys, tmp_path / "a")
    _run(monkeypatch, capsys, tmp_path / "b")
    assert line["steps"] == 2 and line["unit"] == "voxel-queries/s" and line["dtype"] == "bf16"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(ITERS * S ** 3 / (line["ms_per_step"] * 1e-3))
    for key in ("roofline", "build", "lookup_avg_ms", "flow_step", "backward", "backward_amp", "cpu_baseline"):
        assert key not in line                             # those take runs of their own: --full only

    # the step's inputs again (bench.main), through the same rows, eagerly
    g = torch.Generator(device="cpu").manual_seed(1234)
    f1 = torch.randn(1, C, S, S, S, generator=g)
    f2 = torch.randn(1, C, S, S, S, generator=g)
    base = dvccorr.coords_grid_3d(1, S, S, S, torch.device("cpu"))
    coords = [base + bench.synthetic_flow("random", 1, S, 2.0, g) for _ in range(ITERS)]
    with torch.no_grad():
        rows = HipRows(f1.cuda().reshape(1, C, -1), f2.cuda(), L, R, False, "bf16", "materialised")
        want = [rows.lookup(c.cuda().reshape(1, 3, -1).contiguous()).cpu().numpy() for c in coords]
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == [f"lookup_{i:02d}.npy" for i in range(ITERS)]
    for name, w in zip(names, want):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and a.shape == (1, L * (2 * R + 1) ** 3, S ** 3)
        assert np.array_equal(a, b) and np.array_equal(a, w)
