"""bench.py's command line: a plain run prints the result line without the CPU legs, --steps sets the
timed steps, and --dump-outputs writes what the last timed step left its caller -- the int64 lightmap (as
float64) and the finalised float32 texels -- which equal the oracle's bake of the same schedule bit for bit."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fm_oracle as O
from conftest import GOLDEN, REPO

BENCH = os.path.join(REPO, "bench.py")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_writes_float_arrays(tmp_path):
    """dump_outputs on host tensors: lightmap.npy float64 holding the int64 sums exactly, texels.npy float32."""
    import torch

    lm = torch.tensor([[1, 2, 3, 0], [2**52 + 1, -5, 1_000_012_800 << 25, 0]], dtype=torch.int64)
    tex = torch.tensor([[0.5, 0.25, 1.0, 7.0], [1e-8, 3.0, 2.0, 0.0]], dtype=torch.float32)
    d = str(tmp_path / "dump" / "nested")
    _bench().dump_outputs(d, lm, tex)
    assert sorted(os.listdir(d)) == ["lightmap.npy", "texels.npy"]
    a, t = np.load(os.path.join(d, "lightmap.npy")), np.load(os.path.join(d, "texels.npy"))
    assert a.dtype == np.float64 and a.shape == (2, 4) and np.array_equal(a.astype(np.int64), lm.numpy())
    assert t.dtype == np.float32 and np.array_equal(t.view(np.uint32), tex.numpy().view(np.uint32))


@pytest.mark.gpu
def test_plain_run_line_and_dump_match_the_oracle(torch_cuda, example_scene, tmp_path):
    """One plain run of BASELINE config 1's size (example.png, spa 65,000: 11,008 work items) in a fresh
    process: 3 timed steps, no CPU legs in the line, and the dumped arrays equal the oracle's whole bake."""
    spa, steps = 65_000, 3
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--config", "example",
                        "--spa", str(spa), "--dump-outputs", d], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "photons/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(out["config"]["photons_per_step"] / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in out if k.startswith("cpu_baseline")], "the CPU legs belong to --full"

    L = O.schedule_with_offsets(example_scene, spa, np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy")))
    assert out["config"]["photons_per_step"] == 100 * int(L["item_begin"][-1] + L["count"][-1])
    olm, _ = O.bake_port(example_scene, L)
    lm, tex = np.load(os.path.join(d, "lightmap.npy")), np.load(os.path.join(d, "texels.npy"))
    assert lm.dtype == np.float64 and lm.shape == (example_scene.num_texels, 4)
    assert tex.dtype == np.float32 and tex.shape == (example_scene.num_texels, 4)
    assert np.array_equal(lm[:, :3].astype(np.int64), olm) and not lm[:, 3].any()
    exp = O.finalize(olm, np.zeros((example_scene.num_texels, 4), np.float32))
    assert np.array_equal(tex.view(np.uint32), exp.view(np.uint32))
