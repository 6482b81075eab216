#!/usr/bin/env python3
"""Caller-supplied rays against the frame render they can replace (DESIGN.md
"render_rays").

C4 at 3840 x 2160 (default), each precision, one light of the test rig,
scenes.palette, one bounce at strength 1, sky + sun + fog.  Three paths, timed
with device events on one stream, alternated window by window in one process:

  env         one sdf_render_env call
  rays_rows   sdf_render_rays (SDF_RAYS_UNIT) on the rays of sdf_camera_rays in
              their row-major order: a wave is 64 pixels of one row
  rays_tiles  the same rays permuted so that every 64 consecutive rays are one
              8 x 8 tile, the render's own wave shape

Each window runs back to back for at least --window seconds (after a warm-up of
every leg; never fewer than 20 launches per leg in all) and gives one ms per
frame; --repeats windows per leg; the spread is that of the env leg's repeats,
(max - min) / median.  On the timed frame both ray orders must give the env
frame bit for bit in exact precision (asserted); in fast precision the number
of differing words is recorded (the frame render contracts layer 0 around a
uniform eye).  Recorded too -- at the tests' 37 x 23 shape -- the largest
deviation of the fast rays composite from the reference replayed at the
kernel's step counts (tests/test_gpu_rays.py asserts fast_paths.ENV_BOUND).

    python tools/rays_probe.py --out profiles/rays_C4.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

from lights_probe import window  # noqa: E402  (the same windows)


def measure(torch, legs, stream, seconds, repeats):
    """Warm every leg up, then `repeats` windows per leg, alternated:
    ({leg: [ms per frame]}, {leg: launches timed})."""
    import time
    est = {}
    for k, fn in legs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        est[k] = (time.perf_counter() - t0) * 1e3 / 3
    ms, launches = {k: [] for k in legs}, {k: 0 for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            t, n = window(torch, fn, stream, seconds, est[k])
            ms[k].append(t)
            launches[k] += n
    return ms, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--precisions", nargs="+", default=["exact", "fast"])
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per leg, alternated")
    ap.add_argument("--no-deviation", action="store_true", help="skip the fast deviation")
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    a = ap.parse_args()
    if a.width % 8 or a.height % 8:
        raise SystemExit("rays_probe: width and height must be multiples of 8 (whole tiles)")

    import numpy as np
    import torch
    import env_ref as ER
    import lights_ref as LR
    import materials_ref as MR
    from sdf3d_amd import Renderer, abi, scenes
    if not torch.cuda.is_available():
        raise SystemExit("rays_probe: no HIP device (there is nothing to measure without one)")
    rd = Renderer("cuda:0")
    s = torch.cuda.current_stream()
    env = ER.environment(abi.ENV_SKY | abi.ENV_SUN | abi.ENV_FOG)
    W, H = a.width, a.height
    n = W * H
    # ray i of the tiled order is pixel perm[i]: tiles row-major, 8 x 8 inside
    perm = torch.arange(n, device=rd.device).reshape(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3) \
        .reshape(-1)
    rec = {"config": a.config, "width": W, "height": H, "rays": n, "window_s": a.window,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "bounces": 1,
           "flags": "SKY|SUN|FOG", "fog": list(ER.FOG_RANGE), "results": []}

    for prec in a.precisions:
        p = abi.PRECISION_EXACT if prec == "exact" else abi.PRECISION_FAST
        f = scenes.config(a.config, W, H, precision=p)
        kw = dict(lights=LR.rig(1), materials=MR.palette_for(f), reflect=(1, 1.0), env=env,
                  stream=s)
        frame = rd.alloc(f)[0]
        o, d = (t.reshape(n, 3) for t in rd.camera_rays(f))
        ot, dt = o[perm].contiguous(), d[perm].contiguous()
        rows, tiles = (torch.empty((n, 4), dtype=torch.float32, device=rd.device)
                       for _ in range(2))
        legs = {"env": lambda: rd.render(f, out=frame, **kw),
                "rays_rows": lambda: rd.render_rays(f, o, d, unit=True, out=rows, **kw),
                "rays_tiles": lambda: rd.render_rays(f, ot, dt, unit=True, out=tiles, **kw)}
        ms, launches = measure(torch, legs, s, a.window, a.repeats)
        assert min(launches.values()) >= 20, launches
        torch.cuda.synchronize()
        # the timed frame: both orders against the env render, word for word
        want = frame.reshape(n, 4).view(torch.int32)
        back = torch.empty_like(tiles)
        back[perm] = tiles
        differ = {"rays_rows": int((rows.view(torch.int32) != want).sum()),
                  "rays_tiles": int((back.view(torch.int32) != want).sum())}
        if p == abi.PRECISION_EXACT:
            assert differ == {"rays_rows": 0, "rays_tiles": 0}, differ
        med = {k: statistics.median(v) for k, v in ms.items()}
        r = {"precision": prec, "kernel_id": rd.lib.sdf_kernel_id(p).decode(),
             "ms": {k: round(v, 4) for k, v in med.items()},
             "windows_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
             "launches": launches,
             "mrays_per_s": {k: round(n / v / 1e3, 1) for k, v in med.items()},
             "env_spread": round((max(ms["env"]) - min(ms["env"])) / med["env"], 5),
             "rays_rows_over_env": round(med["rays_rows"] / med["env"], 5),
             "rays_tiles_over_env": round(med["rays_tiles"] / med["env"], 5),
             "rays_rows_over_tiles": round(med["rays_rows"] / med["rays_tiles"], 5),
             "words_differing_from_env": differ, "words": 4 * n}
        rec["results"].append(r)
        print(json.dumps(r), flush=True)
        del frame, o, d, ot, dt, rows, tiles, back
        torch.cuda.empty_cache()

    if not a.no_deviation:
        # fast precision's composite of the camera's rays against the reference,
        # at the tests' shape and by the tests' own comparison
        from gpu_support import rays_fast_deviation
        dev = {}
        for name in ("C4", "C3", "REF"):
            for b in (1, 2):
                dmax, left_out, pixels = rays_fast_deviation(rd, name, b)
                dev[f"{name}_bounces{b}"] = {"max_abs_deviation": dmax, "rays_left_out": left_out,
                                             "rays": pixels}
        rec["fast_deviation"] = {"shape": list(ER.SHAPE), "flags": "SKY|SUN|FOG",
                                 "boundary": ER.BOUNDARY, "frames": dev,
                                 "largest": max(v["max_abs_deviation"] for v in dev.values())}
        print(json.dumps(rec["fast_deviation"]), flush=True)

    text = json.dumps(rec, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({"rays_probe": "done"}), flush=True)


if __name__ == "__main__":
    main()
