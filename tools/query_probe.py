#!/usr/bin/env python3
"""The query entry points against the render they share their march with
(DESIGN.md "query").

For each config (default C4 and C5 at 1920 x 1080) and each precision these
paths are timed with device events on one stream, alternated window by window
in one process, every one into buffers allocated once:

  camera_march   sdf_trace_camera writing t and steps only
  camera_all     sdf_trace_camera writing t, steps, normal and prim
  render_flags0  sdf_render of the same frame with flags 0 (no shadow, no AO)
  render         sdf_render with the config's own flags: the unchanged kernels
  trace_ordered  sdf_trace (all four outputs) on the camera's own rays in pixel
                 order: a wave is 64 pixels of one row instead of an 8 x 8 tile
  trace_shuffled the same rays in a random order: every wave incoherent, the
                 price of the wave-uniform culling and of divergent march
                 lengths

Each window runs back to back for at least --window seconds (after a warm-up
of every leg) and gives one ms-per-call figure; --repeats windows per leg; the
spread is that of the render_flags0 leg's repeats, (max - min) / median.
Recorded too, on the tests' 200-ray set over REF, C4 and C5: the largest
deviations of the fast kernels from the reference (the bounds of
tests/test_gpu_query.py).

    python tools/query_probe.py --out profiles/query_C4.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

from lights_probe import measure  # noqa: E402  (the same windows and alternation)

BASE = "render_flags0"


def ratios(ms):
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = (max(ms[BASE]) - min(ms[BASE])) / med[BASE]
    out = {"ms": {k: round(v, 4) for k, v in med.items()},
           "windows_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "render_flags0_spread": round(spread, 5)}
    for k in med:
        if k != BASE:
            out[f"{k}_over_render_flags0"] = round(med[k] / med[BASE], 5)
    out["camera_all_over_camera_march"] = round(med["camera_all"] / med["camera_march"], 5)
    out["trace_ordered_over_camera_all"] = round(med["trace_ordered"] / med["camera_all"], 5)
    out["trace_shuffled_over_trace_ordered"] = round(med["trace_shuffled"] / med["trace_ordered"],
                                                     5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["C4", "C5"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--precisions", nargs="+", default=["exact", "fast"])
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per leg, alternated")
    ap.add_argument("--no-deviation", action="store_true", help="skip the fast deviation")
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    a = ap.parse_args()

    import numpy as np
    import torch
    import materials_ref as MR
    import query_ref as Q
    from sdf3d_amd import Renderer, abi, scenes
    if not torch.cuda.is_available():
        raise SystemExit("query_probe: no HIP device (there is nothing to measure without one)")
    rd = Renderer("cuda:0")
    lib = rd.lib
    s = torch.cuda.current_stream()
    sp = C.c_void_p(s.cuda_stream)
    rec = {"configs": a.configs, "width": a.width, "height": a.height, "window_s": a.window,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "kernel_id": {p: lib.sdf_kernel_id(abi.PRECISION_EXACT if p == "exact"
                                              else abi.PRECISION_FAST).decode()
                         for p in a.precisions}, "results": []}
    n = a.width * a.height
    dev = rd.device
    t = torch.empty(n, dtype=torch.float32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    nr = torch.empty((n, 3), dtype=torch.float32, device=dev)
    pr = torch.empty(n, dtype=torch.int32, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    march = abi.sdf_hits(p(t), p(st), None, None)
    every = abi.sdf_hits(p(t), p(st), p(nr), p(pr))
    perm = torch.from_numpy(np.random.default_rng(7).permutation(n)).to(dev)

    for config in a.configs:
        f0 = scenes.config(config, a.width, a.height)
        O, D = Q.camera_rays(f0)
        O, D = torch.from_numpy(O).to(dev), torch.from_numpy(D).to(dev)
        Os, Ds = O[perm].contiguous(), D[perm].contiguous()
        for prec in a.precisions:
            f = scenes.config(config, a.width, a.height,
                              precision=abi.PRECISION_EXACT if prec == "exact"
                              else abi.PRECISION_FAST)
            g = f.copy()
            g.params.flags = 0
            out = rd.alloc(f)[0]

            def camera(h, f=f):
                abi.check(lib.sdf_trace_camera(C.byref(f.scene), C.byref(f.camera),
                                               C.byref(f.params), C.byref(h), sp), "trace_camera")

            def rays(o, d, f=f):
                abi.check(lib.sdf_trace(C.byref(f.scene), C.byref(f.params), p(o), p(d), n,
                                        C.byref(every), sp), "trace")
            legs = {"camera_march": lambda: camera(march),
                    "camera_all": lambda: camera(every),
                    "render_flags0": lambda g=g, out=out: rd.render(g, out=out, stream=s),
                    "render": lambda f=f, out=out: rd.render(f, out=out, stream=s),
                    "trace_ordered": lambda: rays(O, D),
                    "trace_shuffled": lambda: rays(Os, Ds)}
            r = {"config": config, "precision": prec}
            r.update(ratios(measure(torch, legs, s, a.window, a.repeats)))
            camera(every)
            torch.cuda.synchronize()
            r["pixels_hit"] = round(float((pr >= 0).float().mean()), 5)
            r["mean_steps"] = round(float(st.float().mean()), 3)
            rec["results"].append(r)
            print(json.dumps(r), flush=True)
            del out
            torch.cuda.empty_cache()

    if "fast" in a.precisions and not a.no_deviation:
        o, d = Q.ray_set()
        od, dd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        devs = {}
        for name in ("REF", "C4", "C5"):
            f = scenes.config(name, 64, 36, precision=abi.PRECISION_FAST)
            h = rd.trace(f, od, dd)
            torch.cuda.synchronize()
            got = {k: getattr(h, k).cpu().numpy() for k in ("t", "steps", "normal", "prim")}
            devs[name] = Q.fast_deviation(scenes.config(name, 64, 36), o, d, got, MR.GAP)
        rec["fast_deviation"] = {"rays": len(o), "seed": Q.SEED, "gap": MR.GAP, "scenes": devs,
                                 "largest_t": max(v["t"] for v in devs.values()),
                                 "largest_normal": max(v["normal"] for v in devs.values())}
        print(json.dumps(rec["fast_deviation"]), flush=True)

    text = json.dumps(rec, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({"query_probe": "done", "kernel_id": rec["kernel_id"]}), flush=True)


if __name__ == "__main__":
    main()
