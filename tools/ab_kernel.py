#!/usr/bin/env python3
"""In-process A/B timing of render-kernel builds (libsdf3d.so variants).

Each library is loaded side by side (tools/build_variant.sh builds one from a
git revision); the C4 frame (or --config) is rendered by each in turn,
rounds interleaved so clock drift hits all alike, and the median per-launch
kernel time (HIP events around 5 serialised launches) is printed per
library, with a bit-exactness check of each against the first.

    python tools/ab_kernel.py base=tools/_variants/libsdf3d_base.so new=sdf3d_amd/lib/libsdf3d.so

--rig: the lights and materials kernels instead, with the test rig's lights
(tests/lights_ref.py rig), palette (scenes.palette) and, with --reflect /
--sky, its bounces and sky passed to Renderer.render.  Two parts:

  bits    frames and step counts of every library against the first's, bit
          for bit, over C4 (a built-in variant), the tests' SIX (run-time
          specialised), SIX under DISPATCH_GENERIC and DISPATCH_UNCULLED, and
          C5; 1 and 3 lights; the colour flag off and on; samples 1 and 2;
          steps asked for and not; 37 x 23 and 64 x 36; both precisions
  timing  C4 at 1920 x 1080 with 1 and 4 lights in both precisions, the legs
          alternated window by window (tools/lights_probe.py measure); the
          margin is the first library's own spread, (max - min) / median, and
          a later library whose median lies beyond it on the slow side fails

    python tools/ab_kernel.py --rig parent=tools/_variants/libsdf3d_parent.so \
        new=sdf3d_amd/lib/libsdf3d.so --out profiles/shading_refactor_ab.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def rig_main(a):
    sys.path.insert(0, str(ROOT / "tests"))
    sys.path.insert(0, str(ROOT / "tools"))
    import torch
    import lights_ref as LR
    import materials_ref as MR
    import reflect_ref as RR
    from lights_probe import measure
    from sdf3d_amd import Renderer, abi, scenes
    rds = {}
    for spec in a.libs:
        name, path = spec.split("=", 1)
        rds[name] = Renderer("cuda:0")
        rds[name].lib = abi.load_library(path, any_version=True)
    first = next(iter(rds))
    precs = {"exact": abi.PRECISION_EXACT, "fast": abi.PRECISION_FAST}
    extra = {}
    if a.reflect:
        extra["reflect"] = RR.reflect(a.reflect, 0.5)
    if a.sky:
        extra["env"] = scenes.sky()
    rec = {"device": torch.cuda.get_device_name(0), "libs": list(rds), "extra": sorted(extra),
           "kernel_id": {n: {p: rd.lib.sdf_kernel_id(v).decode() for p, v in precs.items()}
                         for n, rd in rds.items()}}

    def frames(p, wh):
        yield "C4", scenes.config("C4", *wh, precision=p)
        for name, d in (("SIX", abi.DISPATCH_AUTO), ("SIX generic", abi.DISPATCH_GENERIC),
                        ("SIX unculled", abi.DISPATCH_UNCULLED)):
            f = MR.six(p, wh=wh)
            f.params.dispatch = d
            yield name, f
        yield "C5", scenes.config("C5", *wh, precision=p, pose=3)

    # ---- bits ----
    cases, differ = 0, []
    for pn, p in precs.items():
        for wh in ((37, 23), (64, 36)):
            for name, f in frames(p, wh):
                prims = f.scene.kind == abi.SCENE_PRIMITIVES
                for L in (1, 3):
                    for flags in (0, abi.LIGHTS_COLOR):
                        for samples in (1, 2):
                            for steps in (False, True):
                                for fam in ("lights", "materials") if prims else ("lights",):
                                    g = f.copy()
                                    g.params.samples = samples
                                    kw = dict(lights=LR.rig(L), light_flags=flags, steps=steps,
                                              **extra)
                                    if fam == "materials":
                                        kw["materials"] = MR.palette_for(g)
                                    got = {n: rd.render(g, **kw) for n, rd in rds.items()}
                                    torch.cuda.synchronize()
                                    cases += 1
                                    for n, (rgba, st) in got.items():
                                        same = torch.equal(rgba.view(torch.int32),
                                                           got[first][0].view(torch.int32))
                                        if steps:
                                            same = same and torch.equal(st, got[first][1])
                                        if not same:
                                            differ.append([n, pn, list(wh), name, L, flags,
                                                           samples, steps, fam])
    rec["bits"] = {"cases": cases, "differ": differ}
    print(json.dumps(rec["bits"]), flush=True)

    # ---- timing ----
    s = torch.cuda.current_stream()
    rec["timing"] = []
    ok = not differ
    for pn, p in precs.items():
        f = scenes.config("C4", 1920, 1080, precision=p)
        mats = MR.palette_for(f)
        for L in (1, 4):
            for fam in ("lights", "materials"):
                # one plain light is sdf_render's own path: the colour flag
                # keeps the leg on the lights kernels
                flags = abi.LIGHTS_COLOR if (fam == "lights" and L == 1) else 0
                kw = dict(lights=LR.rig(L), light_flags=flags, stream=s, **extra)
                if fam == "materials":
                    kw["materials"] = mats
                outs = {n: rd.alloc(f)[0] for n, rd in rds.items()}
                legs = {n: (lambda rd=rd, n=n: rd.render(f, out=outs[n], **kw))
                        for n, rd in rds.items()}
                ms = measure(torch, legs, s, a.window, a.repeats)
                med = {n: statistics.median(v) for n, v in ms.items()}
                spread = (max(ms[first]) - min(ms[first])) / med[first]
                r = {"precision": pn, "family": fam, "lights": L, "light_flags": flags,
                     "ms": {n: round(v, 4) for n, v in med.items()},
                     "windows_ms": {n: [round(x, 4) for x in v] for n, v in ms.items()},
                     f"{first}_spread": round(spread, 5),
                     "over_" + first: {n: round(med[n] / med[first], 5) for n in med if n != first}}
                r["not_slower"] = all(med[n] <= med[first] * (1.0 + spread) for n in med)
                ok = ok and r["not_slower"]
                rec["timing"].append(r)
                print(json.dumps(r), flush=True)
                del outs
                torch.cuda.empty_cache()
    rec["pass"] = ok
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({"ab_kernel_rig": "pass" if ok else "FAIL"}), flush=True)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+", help="name=path")
    ap.add_argument("--rig", action="store_true",
                    help="the lights / materials kernels with the test rig (see above)")
    ap.add_argument("--reflect", type=int, default=0, help="--rig: bounces (0: no reflect)")
    ap.add_argument("--sky", action="store_true", help="--rig: scenes.sky() as the environment")
    ap.add_argument("--window", type=float, default=0.5, help="--rig: seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="--rig: windows per leg")
    ap.add_argument("--config", default="C4")
    ap.add_argument("--precision", default="fast")
    ap.add_argument("--format", default="rgba32f")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--poses", default="0")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.rig:
        sys.exit(rig_main(a))
    import torch
    from sdf3d_amd import Renderer, abi, scenes
    rds = {}
    for spec in a.libs:
        name, path = spec.split("=", 1)
        rd = Renderer("cuda:0")
        rd.lib = abi.load_library(path, any_version=True)
        rds[name] = rd
    prec = abi.PRECISION_FAST if a.precision == "fast" else abi.PRECISION_EXACT
    res = {}
    for pose in [int(p) for p in a.poses.split(",")]:
        f = scenes.config(a.config, precision=prec, pose=pose)
        f.params.output_format = abi.FORMAT_NAMES[a.format]
        bufs = {n: rd.alloc(f)[0] for n, rd in rds.items()}
        first = None
        same = {}
        for n, rd in rds.items():
            rd.render(f, out=bufs[n])
            torch.cuda.synchronize()
            if first is None:
                first = bufs[n].clone()
            same[n] = bool(torch.equal(bufs[n].view(torch.uint8), first.view(torch.uint8)))
        t = {n: [] for n in rds}
        # warm the clocks
        for _ in range(100):
            for n, rd in rds.items():
                rd.render(f, out=bufs[n])
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for n, rd in rds.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                rd.render(f, out=bufs[n])
                e0.record()
                for _ in range(5):
                    rd.render(f, out=bufs[n])
                e1.record()
                torch.cuda.synchronize()
                t[n].append(e0.elapsed_time(e1) / 5)
        res[f"pose{pose}"] = {n: {"kernel_ms": round(statistics.median(v), 4),
                                  "bit_exact_vs_first": same[n]} for n, v in t.items()}
        print(json.dumps({f"{a.config} pose {pose}": res[f"pose{pose}"]}), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
