#!/usr/bin/env python3
"""Per-primitive materials against the multi-light render they extend
(DESIGN.md "Materials").

For one frame (default C4 at 1920 x 1080) and L in {1, 4} lights of the test
rig (tests/lights_ref.py RIG[:L]), these paths are timed with device events on
one stream, alternated window by window in one process:

  lights     one sdf_render_lights call (the frame's one material)
  materials  one sdf_render_materials call with scenes.palette: the same
             frame plus the material fold at P, one more unculled evaluation
             of the primitive list per pixel
  parent     sdf_render_lights of another build of the library (--parent-lib,
             e.g. the parent commit's): are the existing kernels untouched?
  NAME       sdf_render_materials of a variant build (--variant NAME=PATH,
             e.g. another SDF_MATERIALS_WAVES_PER_EU)

Each window renders back to back for at least --window seconds (after a
warm-up of every leg) and gives one ms-per-frame figure; --repeats windows per
leg.  The spread is that of the `lights` leg's own repeats, (max - min) /
median.  With L = 1 the lights leg is the plain kernel (one plain light is
sdf_render), so the pair is also timed with SDF_LIGHTS_COLOR, which keeps both
on the lights kernels.  Recorded beside the timings: whether the timed
materials frame equals tests/materials_ref.py compose_px of the build's own
terms and probed fold, bit for bit, and -- at the tests' 37 x 23 shape -- the
largest deviation of the fast kernel's blended components from the reference
fold replayed at the kernel's step counts (the bound of
tests/test_gpu_materials.py).

    python tools/materials_probe.py --out profiles/materials_C4.json
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

from lights_probe import measure  # noqa: E402  (the same windows and alternation)


def ratios(ms, base="lights"):
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = (max(ms[base]) - min(ms[base])) / med[base]
    out = {"ms": {k: round(v, 4) for k, v in med.items()},
           "windows_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "lights_spread": round(spread, 5)}
    for k in med:
        if k != base:
            out[f"{k}_over_lights"] = round(med[k] / med[base], 5)
    return out


def probe_fold(np, rd, abi, MR, f, light):
    """The kernel's own blended (amb, dif, ref) of `f` with its palette and the
    probe render's steps (tests/test_gpu_materials.py probe)."""
    g = f.copy()
    g.params.flags &= ~abi.FLAG_AO
    l = type(light).from_buffer_copy(light)
    l.ambient = 1.0
    out, st = [], None
    for field in ("amb", "dif", "ref"):
        mats = []
        for m in MR.palette_for(f):
            q = abi.sdf_material()
            q.shininess = m.shininess
            for c in range(3):
                q.amb[c] = getattr(m, field)[c]
            mats.append(q)
        rgba, st = rd.render(g, steps=True, lights=[l], materials=mats)
        out.append(rgba.cpu().numpy()[..., :3].copy())
    return out, st.cpu().numpy()


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
                    help="a variant build whose sdf_render_materials is timed too")
    ap.add_argument("--no-check", action="store_true", help="skip the bit comparison")
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    a = ap.parse_args()

    import numpy as np
    import torch
    import lights_ref as LR
    import materials_ref as MR
    from sdf3d_amd import Renderer, abi, scenes
    if not torch.cuda.is_available():
        raise SystemExit("materials_probe: no HIP device (there is nothing to measure without one)")
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

    def legs_of(f, lights, flags, mats):
        out = rd.alloc(f)[0]
        legs = {"lights": lambda: rd.render(f, out=out, stream=s, lights=lights,
                                            light_flags=flags),
                "materials": lambda: rd.render(f, out=out, stream=s, lights=lights,
                                               light_flags=flags, materials=mats)}
        if parent:
            legs["parent"] = lambda: parent.render(f, out=out, stream=s, lights=lights,
                                                   light_flags=flags)
        for name, r in variants.items():
            legs[name] = (lambda r=r: r.render(f, out=out, stream=s, lights=lights,
                                               light_flags=flags, materials=mats))
        return legs, out

    for prec in a.precisions:
        p = abi.PRECISION_EXACT if prec == "exact" else abi.PRECISION_FAST
        for L in a.lights:
            f = scenes.config(a.config, a.width, a.height, precision=p)
            mats = MR.palette_for(f)
            lights = LR.rig(L)
            legs, out = legs_of(f, lights, 0, mats)
            r = {"precision": prec, "lights": L}
            r.update(ratios(measure(torch, legs, s, a.window, a.repeats)))
            if L == 1:
                legs1, _ = legs_of(f, lights, abi.LIGHTS_COLOR, mats)
                r["one_coloured_light"] = ratios(measure(torch, legs1, s, a.window, a.repeats))
            if not a.no_check:
                terms, specs = [], []
                for l in lights:
                    g = LR.with_light(f, l)
                    g.params.output_format = abi.FORMAT_SHADE32F
                    terms.append(rd.render(g)[0].cpu().numpy())
                    h = LR.with_light(f, l)
                    for c in range(3):
                        h.material.amb[c], h.material.dif[c], h.material.ref[c] = 0.0, 0.0, 1.0
                    specs.append(rd.render(h)[0].cpu().numpy()[..., 0].copy())
                (amb, dif, ref), _ = probe_fold(np, rd, abi, MR, f, lights[0])
                want = MR.compose_px(f, terms, lights, amb, dif, ref, 0, p, specs=specs)
                legs["materials"]()
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                r["bit_exact"] = bool((want.view("uint32") == got.view("uint32")).all())
                del terms, specs, want, got
            rec["results"].append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()

    # fast precision's fold against the reference fold, at the tests' shape
    dev = {}
    for name, pose in (("C4", 0), ("SIX", 2), ("SIXH", 2)):
        f = MR.frame_of(name, pose, abi.PRECISION_FAST)
        if name != "C4":
            f.params.dispatch = abi.DISPATCH_GENERIC
        (amb, dif, ref), st = probe_fold(np, rd, abi, MR, f, LR.rig(1)[0])
        ref_f = MR.fold(MR.frame_of(name, pose), MR.palette_for(f), steps=st)
        keep = ref_f["min_gap"] >= MR.GAP
        worst = max(float(np.abs(got[keep].astype(np.float64) - ref_f[k][keep]).max())
                    for got, k in zip((amb, dif, ref), ("amb", "dif", "ref")))
        dev[name] = {"max_abs_deviation": worst, "pixels_compared": int(keep.sum()),
                     "pixels": int(keep.size)}
    rec["fast_fold_deviation"] = {"shape": list(MR.SHAPE), "min_gap": MR.GAP, "frames": dev}
    print(json.dumps(rec["fast_fold_deviation"]), flush=True)

    text = json.dumps(rec, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({"materials_probe": "done", "kernel_id": rec["kernel_id"]}), flush=True)


if __name__ == "__main__":
    main()
