#!/usr/bin/env python3
"""Shading at points against the frame render whose hit points they are
(DESIGN.md "shade_points").

C4 at 3840 x 2160 (default), each precision, scenes.palette, with one light of
the test rig and with eight.  The points are the frame's 8,294,400 hit points,
P_0 = O_0 + D_0 d, formed on the device from sdf_trace_camera's t and
sdf_camera_rays in unfused fp32; the eye is the camera.  Three legs, timed with
device events on one stream, alternated window by window in one process:

  materials     one sdf_render_materials call (its kernels are the parent
                commit's, instruction for instruction: tools/asm_compare.py)
  points_rows   sdf_shade_points (rgba) on the points in row-major order: a
                wave is 64 pixels of one row
  points_tiles  the same points regrouped so that every 64 consecutive points
                are one 8 x 8 tile, the render's own wave shape

Each window runs back to back for at least --window seconds (after a warm-up of
every leg; never fewer than 20 launches per leg in all) and gives one ms per
call; --repeats windows per leg; the spread is that of the materials leg's
repeats, (max - min) / median.  In exact precision both orders must give the
frame bit for bit (asserted); in fast precision the number of differing words
is recorded.  Recorded too -- at the tests' 37 x 23 shape and by the tests' own
comparison -- the largest deviation of the fast kernel from the reference
replayed at its own shadow counts (tests/test_gpu_points.py asserts 4 x that).

    python tools/points_probe.py --out profiles/points_C4.json
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

from rays_probe import measure  # noqa: E402  (the same windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--precisions", nargs="+", default=["exact", "fast"])
    ap.add_argument("--lights", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per leg, alternated")
    ap.add_argument("--no-deviation", action="store_true", help="skip the fast deviation")
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    a = ap.parse_args()
    if a.width % 8 or a.height % 8:
        raise SystemExit("points_probe: width and height must be multiples of 8 (whole tiles)")

    import torch
    import lights_ref as LR
    import materials_ref as MR
    from sdf3d_amd import Renderer, abi, scenes
    if not torch.cuda.is_available():
        raise SystemExit("points_probe: no HIP device (there is nothing to measure without one)")
    rd = Renderer("cuda:0")
    s = torch.cuda.current_stream()
    W, H = a.width, a.height
    n = W * H
    # point i of the tiled order is pixel perm[i]: tiles row-major, 8 x 8 inside
    perm = torch.arange(n, device=rd.device).reshape(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3) \
        .reshape(-1)
    rec = {"config": a.config, "width": W, "height": H, "points": n, "window_s": a.window,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "results": []}

    for prec in a.precisions:
        p = abi.PRECISION_EXACT if prec == "exact" else abi.PRECISION_FAST
        f = scenes.config(a.config, W, H, precision=p)
        mats = MR.palette_for(f)
        o, d = (t.reshape(n, 3) for t in rd.camera_rays(f))
        t = rd.trace_camera(f, normal=False, prim=False, steps=False).t.reshape(n, 1)
        P = (o + d * t).contiguous()       # a product and a sum, each rounded once
        Pt = P[perm].contiguous()
        eye = [float(x) for x in o[0].cpu()]
        del d, t
        for nl in a.lights:
            lights = LR.rig(nl)
            frame = rd.alloc(f)[0]
            legs = {"materials": lambda: rd.render(f, out=frame, lights=lights, materials=mats,
                                                   stream=s)}
            out = {}

            def points(which, pts):
                out[which] = rd.shade_points(f, pts, eye=eye, lights=lights, materials=mats,
                                             stream=s).rgba
            legs["points_rows"] = lambda: points("rows", P)
            legs["points_tiles"] = lambda: points("tiles", Pt)
            ms, launches = measure(torch, legs, s, a.window, a.repeats)
            assert min(launches.values()) >= 20, launches
            torch.cuda.synchronize()
            want = frame.reshape(n, 4).view(torch.int32)
            back = torch.empty_like(out["tiles"])
            back[perm] = out["tiles"]
            differ = {"points_rows": int((out["rows"].view(torch.int32) != want).sum()),
                      "points_tiles": int((back.view(torch.int32) != want).sum())}
            if p == abi.PRECISION_EXACT:
                assert differ == {"points_rows": 0, "points_tiles": 0}, differ
            med = {k: statistics.median(v) for k, v in ms.items()}
            r = {"precision": prec, "lights": nl, "kernel_id": rd.lib.sdf_kernel_id(p).decode(),
                 "ms": {k: round(v, 4) for k, v in med.items()},
                 "windows_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                 "launches": launches,
                 "mpoints_per_s": {k: round(n / v / 1e3, 1) for k, v in med.items()},
                 "materials_spread": round((max(ms["materials"]) - min(ms["materials"])) /
                                           med["materials"], 5),
                 "points_rows_over_materials": round(med["points_rows"] / med["materials"], 5),
                 "points_tiles_over_materials": round(med["points_tiles"] / med["materials"], 5),
                 "points_rows_over_tiles": round(med["points_rows"] / med["points_tiles"], 5),
                 "words_differing_from_frame": differ, "words": 4 * n}
            rec["results"].append(r)
            print(json.dumps(r), flush=True)
            del frame, back, out
        del o, P, Pt
        torch.cuda.empty_cache()

    if not a.no_deviation:
        from points_ref import FAST_CASES, fast_deviation
        dev = {}
        for name, pose, pal in FAST_CASES:
            d, far = fast_deviation(rd, name, pose, pal)
            dev[name] = dict(d, material_points=far)
        rec["fast_deviation"] = {
            "shape": list(MR.SHAPE), "lights": 3, "frames": dev,
            "largest": max(max(v["rgba"], v["ao"], v["shadow"]) for v in dev.values()),
            "largest_material": max(v["material"] for v in dev.values())}
        print(json.dumps(rec["fast_deviation"]), flush=True)

    text = json.dumps(rec, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({"points_probe": "done"}), flush=True)


if __name__ == "__main__":
    main()
