"""bench.py --dump-outputs: the arrays it writes are the last timed frame
(whole, or a fixed seeded pixel sample of a frame over 48 MB), float32 or
float64, at most 64 MB in all, identical from run to run; a plain run
reports the headline only."""
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
LIMIT = 64 * 10**6


@pytest.fixture(scope="module")
def bench():
    # bench.py sets its HIP queue count when it is loaded: not for this process
    env, path = dict(os.environ), list(sys.path)
    spec = importlib.util.spec_from_file_location("_bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
    finally:
        os.environ.clear()
        os.environ.update(env)
        sys.path[:] = path
    return mod


def _load(d):
    files = sorted(Path(d).iterdir())
    assert all(f.suffix == ".npy" for f in files)
    arrays = {f.stem: np.load(f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(f.stat().st_size for f in files) <= LIMIT
    return arrays


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.uint8])
def test_dump_small_frame_whole(bench, tmp_path, dtype):
    g = torch.Generator().manual_seed(3)
    frame = (torch.rand((45, 77, 4), generator=g) * 255).to(dtype)
    shapes = bench.dump_outputs(tmp_path / "a" / "b", frame)      # the folder is created
    arrays = _load(tmp_path / "a" / "b")
    assert set(arrays) == {"frame"} and shapes == {"frame": [45, 77, 4]}
    assert arrays["frame"].dtype == np.float32
    assert np.array_equal(arrays["frame"], frame.float().numpy())


def test_dump_large_frame_sample(bench, tmp_path):
    H, W = 2160, 3840                                   # 133 MB of RGBA32F
    flat = torch.arange(H * W, dtype=torch.int32)
    frame = torch.stack([(flat % 4093).float(), (flat // 4093).float(),
                         (flat % 7).float(), torch.ones(H * W)], -1).reshape(H, W, 4)
    bench.dump_outputs(tmp_path / "a", frame)
    bench.dump_outputs(tmp_path / "b", frame)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == {"frame_sample", "frame_sample_index"}
    for k in a:                                          # the same sample every time
        assert a[k].tobytes() == b[k].tobytes()
    idx = a["frame_sample_index"]
    assert idx.dtype == np.float64 and np.array_equal(idx, np.floor(idx))
    i = idx.astype(np.int64)
    assert i.min() >= 0 and i.max() < H * W and (np.diff(i) > 0).all()
    assert len(i) == bench.DUMP_SAMPLE_PIXELS
    # spread over the whole frame, not a corner of it
    assert i.min() < H * W // 100 and i.max() > H * W - H * W // 100
    assert a["frame_sample"].dtype == np.float32
    assert np.array_equal(a["frame_sample"], frame.reshape(-1, 4).numpy()[i])


@pytest.mark.gpu
def test_plain_bench_dumps_the_timed_frame(renderer, tmp_path):
    """One plain run of the benchmark (3 timed steps of C3): the line holds the
    headline and ms_per_step for the steps asked for, nothing --full measures,
    and the dumped sample is the frame a one-device render gives, bit for bit."""
    from sdf3d_amd import abi, scenes
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--config", "C3", "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    W, H = d["config"]["width"], d["config"]["height"]
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(W * H / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    for k in ("cpu_baseline", "roofline", "parity", "kernel_ms", "display_rgba8", "fast",
              "frame_verified"):
        assert d[k] is None, k
    arrays = _load(tmp_path / "d")
    f = scenes.config("C3", precision=abi.PRECISION_EXACT, pose=0)
    assert (f.params.width, f.params.height) == (W, H)
    ref, _ = renderer.render(f)
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    if "frame" in arrays:
        got, want = arrays["frame"], ref
    else:
        i = arrays["frame_sample_index"].astype(np.int64)
        got, want = arrays["frame_sample"], ref.reshape(-1, ref.shape[-1])[i]
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
