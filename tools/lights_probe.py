#!/usr/bin/env python3
"""Multi-light rendering against what it replaces (DESIGN.md "Lights").

For one frame (default C4 at 1920 x 1080) and L in {1, 2, 4, 8} lights of the
test rig (tests/lights_ref.py RIG[:L]), two paths are timed with device events
on one stream, alternated window by window in one process:

  baseline  L plain sdf_render calls, one per light, as RGBA32F: what a user
            runs today before a combination pass of their own -- that pass is
            NOT charged to the baseline
  lights    one sdf_render_lights call with the L lights

Each window renders back to back for at least --window seconds (after a
warm-up of every shape) and gives one ms-per-frame figure; --repeats windows
per path.  The spread is that of the baseline's own repeats, (max - min) /
median.  Recorded beside them: the same pair with SDF_FLAG_SHADOW cleared
(the per-light work without its march), L = 1 with SDF_LIGHTS_COLOR (the
lights kernel at one light) against plain sdf_render, and whether the timed
frame equals tests/lights_ref.py compose of the build's own single-light
terms, bit for bit.

    python tools/lights_probe.py --out profiles/lights_C4.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def window(torch, fn, stream, seconds, est_ms):
    """ms per frame over one window of back-to-back calls lasting >= seconds."""
    n = max(3, int(seconds * 1e3 / est_ms) + 1)
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= seconds * 1e3:
            return ms / n, n
        n = int(n * seconds * 1e3 / max(ms, 1e-3) * 1.1) + 1


def measure(torch, legs, stream, seconds, repeats):
    """Warm every leg up, then `repeats` windows per leg, alternated."""
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
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            ms[k].append(window(torch, fn, stream, seconds, est[k])[0])
    return ms


def summary(ms, base="baseline", new="lights"):
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = (max(ms[base]) - min(ms[base])) / med[base]
    return {"baseline_ms": round(med[base], 4), "lights_ms": round(med[new], 4),
            "baseline_windows_ms": [round(x, 4) for x in ms[base]],
            "lights_windows_ms": [round(x, 4) for x in ms[new]],
            "baseline_spread": round(spread, 5),
            "lights_over_baseline": round(med[new] / med[base], 5),
            "faster_by_more_than_spread": bool(med[new] < med[base] * (1.0 - spread))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--lights", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--precisions", nargs="+", default=["exact", "fast"])
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per path, alternated")
    ap.add_argument("--no-shadowless", action="store_true", help="skip the SDF_FLAG_SHADOW-off pair")
    ap.add_argument("--no-check", action="store_true", help="skip the bit comparison")
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    a = ap.parse_args()

    import torch
    import lights_ref as LR
    from sdf3d_amd import Renderer, abi, scenes
    if not torch.cuda.is_available():
        raise SystemExit("lights_probe: no HIP device (there is nothing to measure without one)")
    rd = Renderer("cuda:0")
    s = torch.cuda.current_stream()
    rec = {"config": a.config, "width": a.width, "height": a.height, "window_s": a.window,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "kernel_id": {p: rd.lib.sdf_kernel_id(abi.PRECISION_EXACT if p == "exact"
                                                 else abi.PRECISION_FAST).decode()
                         for p in a.precisions},
           "results": []}

    def pair(f, lights, flags):
        singles = [LR.with_light(f, l) for l in lights]
        outs = [rd.alloc(f)[0] for _ in lights]
        out = rd.alloc(f)[0]

        def baseline():
            for g, o in zip(singles, outs):
                rd.render(g, out=o, stream=s)
        return {"baseline": baseline,
                "lights": lambda: rd.render(f, out=out, stream=s, lights=lights,
                                            light_flags=flags)}, out

    for prec in a.precisions:
        p = abi.PRECISION_EXACT if prec == "exact" else abi.PRECISION_FAST
        for L in a.lights:
            f = scenes.config(a.config, a.width, a.height, precision=p)
            lights = LR.rig(L)
            legs, out = pair(f, lights, 0)
            r = {"precision": prec, "lights": L}
            r.update(summary(measure(torch, legs, s, a.window, a.repeats)))
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
                want = LR.compose(f, terms, lights, 0, p, specs=specs)
                legs["lights"]()
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                r["bit_exact"] = bool((want.view("uint32") == got.view("uint32")).all())
                del terms, specs, want, got
            if not a.no_shadowless:
                g = f.copy()
                g.params.flags &= ~abi.FLAG_SHADOW
                legs2, _ = pair(g, lights, 0)
                r["no_shadow"] = summary(measure(torch, legs2, s, a.window, max(a.repeats // 2, 3)))
            if L == 1:
                # the lights kernel itself at one light (the colour flag keeps
                # it off sdf_render's own path) against plain sdf_render
                legs3, _ = pair(f, lights, abi.LIGHTS_COLOR)
                r["one_coloured_light"] = summary(measure(torch, legs3, s, a.window, a.repeats))
            rec["results"].append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({"lights_probe": "done", "kernel_id": rec["kernel_id"]}), flush=True)


if __name__ == "__main__":
    main()
