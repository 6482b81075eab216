#!/usr/bin/env python3
"""Mirror reflections against the materials render they extend (DESIGN.md
"Reflections").

For one frame (default C4 at 1920 x 1080, scenes.palette) and L in {1, 4}
lights of the test rig (tests/lights_ref.py RIG[:L]), these paths are timed
with device events on one stream, alternated window by window in one process:

  lights            one sdf_render_lights call (the frame's one material)
  materials         one sdf_render_materials call
  reflect0/1/2      one sdf_render_reflect call with 0, 1, 2 bounces, strength 1
                    (0 bounces is the materials call)
  parent_lights     sdf_render_lights and sdf_render_materials of another build
  parent_materials  of the library (--parent-lib, e.g. the parent commit's):
                    are the existing kernels untouched?
  NAME              sdf_render_reflect, 2 bounces, of a variant build
                    (--variant NAME=PATH, e.g. another SDF_REFLECT_WAVES_PER_EU)

Each window renders back to back for at least --window seconds (after a
warm-up of every leg) and gives one ms-per-frame figure; --repeats windows per
leg; the spread is that of the materials leg's repeats, (max - min) / median.
Beside every reflect ratio stands the simple model 1 + sum_j f_j, f_j the
share of the frame's 8 x 8 tiles with a live lane at layer j, read from the
kernel's own layer planes (layer = j renders with step counts).  Recorded too:
whether the timed 2-bounce frame equals the composition of the kernel's own
layers and weights bit for bit (tests/reflect_ref.py composite), and -- at the
tests' 37 x 23 shape -- the largest deviation of the fast composite from the
reference replayed at the kernel's step counts (the bound of
tests/test_gpu_reflect.py).

    python tools/reflect_probe.py --out profiles/reflect_C4.json
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

import gpu_support as G  # noqa: E402
from lights_probe import measure  # noqa: E402  (the same windows and alternation)


def ratios(ms, base="materials"):
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = (max(ms[base]) - min(ms[base])) / med[base]
    out = {"ms": {k: round(v, 4) for k, v in med.items()},
           "windows_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "materials_spread": round(spread, 5)}
    for k in med:
        if k != base:
            out[f"{k}_over_materials"] = round(med[k] / med[base], 5)
    return out


def kernel_layers(rd, f, bounces, mats, lights):
    """The kernel's own C_j, W_j, steps and alive planes (tests/gpu_support.py)."""
    return G.own_layers(lambda r: G.both(rd, f, lights=lights, materials=mats, reflect=r),
                        bounces, 1.0)


def tile_shares(np, alive):
    """Share of the frame's 8 x 8 tiles with a live lane, per layer."""
    H, W, J = alive.shape
    th, tw = (H + 7) // 8, (W + 7) // 8
    pad = np.zeros((th * 8, tw * 8, J), dtype=bool)
    pad[:H, :W] = alive
    tiles = pad.reshape(th, 8, tw, 8, J).any(axis=(1, 3))
    return [round(float(tiles[..., j].mean()), 5) for j in range(J)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--lights", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--precisions", nargs="+", default=["exact", "fast"])
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per leg, alternated")
    ap.add_argument("--parent-lib", default=None, help="another build's libsdf3d.so")
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=PATH",
                    help="a variant build whose 2-bounce sdf_render_reflect is timed too")
    ap.add_argument("--no-check", action="store_true", help="skip the bit comparison")
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    a = ap.parse_args()

    import numpy as np
    import torch
    import lights_ref as LR
    import materials_ref as MR
    import reflect_ref as RR
    from sdf3d_amd import Renderer, abi, scenes
    if not torch.cuda.is_available():
        raise SystemExit("reflect_probe: no HIP device (there is nothing to measure without one)")
    rd = Renderer("cuda:0")
    s = torch.cuda.current_stream()

    def other(path):
        r = Renderer("cuda:0")
        r.lib = abi.load_library(path, any_version=True)
        return r
    parent = other(a.parent_lib) if a.parent_lib else None
    variants = {v.split("=", 1)[0]: other(v.split("=", 1)[1]) for v in a.variant}

    def ids(lib):
        return {p: lib.sdf_kernel_id(abi.PRECISION_EXACT if p == "exact"
                                     else abi.PRECISION_FAST).decode() for p in a.precisions}
    rec = {"config": a.config, "width": a.width, "height": a.height, "window_s": a.window,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "kernel_id": ids(rd.lib), "results": []}
    if parent:
        rec["parent_kernel_id"] = ids(parent.lib)

    for prec in a.precisions:
        p = abi.PRECISION_EXACT if prec == "exact" else abi.PRECISION_FAST
        for L in a.lights:
            f = scenes.config(a.config, a.width, a.height, precision=p)
            mats = MR.palette_for(f)
            lights = LR.rig(L)
            out = rd.alloc(f)[0]
            kw = dict(out=out, stream=s, lights=lights)
            legs = {"lights": lambda: rd.render(f, **kw),
                    "materials": lambda: rd.render(f, materials=mats, **kw)}
            for b in (0, 1, 2):
                legs[f"reflect{b}"] = (lambda b=b: rd.render(f, materials=mats,
                                                             reflect=(b, 1.0), **kw))
            if parent:
                legs["parent_lights"] = lambda: parent.render(f, **kw)
                legs["parent_materials"] = lambda: parent.render(f, materials=mats, **kw)
            for name, r in variants.items():
                legs[name] = (lambda r=r: r.render(f, materials=mats, reflect=(2, 1.0), **kw))
            r = {"precision": prec, "lights": L}
            r.update(ratios(measure(torch, legs, s, a.window, a.repeats)))
            Cj, Wj, Sj, alive = kernel_layers(rd, f, 2, mats, lights)
            share = tile_shares(np, alive)
            r["live_tile_share"] = share
            r["live_pixel_share"] = [round(float(alive[..., j].mean()), 5) for j in range(3)]
            r["model"] = {"reflect1": round(1 + share[1], 5),
                          "reflect2": round(1 + share[1] + share[2], 5)}
            if not a.no_check:
                legs["reflect2"]()
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                want = RR.composite(Cj, Wj, alive, p)
                r["bit_exact"] = bool((want.view("uint32") == got.view("uint32")).all())
                del want, got
            del Cj, Wj, Sj, alive
            rec["results"].append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()

    # fast precision's composite against the reference, at the tests' shape
    dev = {}
    for name, pose in (("C4", 0), ("C3", 2), ("REF", 0)):
        f = MR.frame_of(name, pose, abi.PRECISION_FAST)
        mats = RR.materials_for(f) if name == "REF" else MR.palette_for(f)
        lights = LR.rig(1)
        for b in (1, 2):
            _, _, Sj, alive = kernel_layers(rd, f, b, mats, lights)
            got = rd.render(f, lights=lights, materials=mats,
                            reflect=(b, 1.0))[0].cpu().numpy()
            force = np.zeros(alive.shape + (RR.FORCE,), dtype=np.int32)
            force[..., 0:2] = Sj
            want, _, w = RR.render(MR.frame_of(name, pose), mats, b, 1.0, lights, 0, force=force)
            dev[f"{name}_bounces{b}"] = {
                "max_abs_deviation": float(np.abs(got.astype(np.float64) - want).max()),
                "layers_traced_differ": int((alive != w["alive"]).sum()),
                "pixels": int(alive[..., 0].size)}
    rec["fast_deviation"] = {"shape": list(MR.SHAPE), "frames": dev}
    print(json.dumps(rec["fast_deviation"]), flush=True)

    text = json.dumps(rec, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({"reflect_probe": "done", "kernel_id": rec["kernel_id"]}), flush=True)


if __name__ == "__main__":
    main()
