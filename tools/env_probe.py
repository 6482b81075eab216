#!/usr/bin/env python3
"""The environment against the reflect render it extends (DESIGN.md
"Environment").

For each frame (default C4 and C3 at 1920 x 1080, scenes.palette, one light of
the test rig), each precision and 0, 1 and 2 bounces, these paths are timed
with device events on one stream, alternated window by window in one process:

  reflect   one sdf_render_reflect call (0 bounces: the materials call): the
            parent's path, which sdf_render_env with nothing switched on is
  sky       sdf_render_env with SDF_ENV_SKY | SDF_ENV_SUN (scenes.sky())
  fog       sdf_render_env with SDF_ENV_FOG, start 1, end 4
  all       all three flags

Each window renders back to back for at least --window seconds (after a
warm-up of every leg) and gives one ms-per-frame figure; --repeats windows per
leg; the spread is that of the reflect leg's repeats, (max - min) / median.
Beside the ratios stand, per layer, the share of the frame's pixels whose path
reaches the layer, the share that misses there (a layer rendered with SKY and
step counts took primary steps and no shadow step), and the share of the 8 x 8
tiles (waves) that reach the layer whose lanes all miss: the waves that skip
the surface work.  Recorded too -- at the tests' 37 x 23 shape -- the largest
deviation of the fast composite from the reference replayed at the kernel's
step counts, away from the miss boundary (the bound of tests/test_gpu_env.py).

    python tools/env_probe.py --out profiles/env_C4.json
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


def ratios(ms, base="reflect"):
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = (max(ms[base]) - min(ms[base])) / med[base]
    out = {"ms": {k: round(v, 4) for k, v in med.items()},
           "windows_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "reflect_spread": round(spread, 5)}
    for k in med:
        if k != base:
            out[f"{k}_over_reflect"] = round(med[k] / med[base], 5)
    return out


def miss_shares(np, rd, f, bounces, mats, lights, env):
    """Per layer: pixels reached, pixels that miss there, and the share of the
    reached 8 x 8 tiles whose reached lanes all miss (from layer = j renders
    with SKY and step counts: a sky layer counts no shadow step)."""
    out = []
    _, _, Sj, _ = G.own_layers(lambda r: G.both(rd, f, lights=lights, materials=mats, reflect=r,
                                                env=env), bounces, 1.0)
    for j in range(bounces + 1):
        st = Sj[:, :, j]
        alive, miss = st[..., 0] > 0, (st[..., 0] > 0) & (st[..., 1] == 0)
        H, W = alive.shape
        th, tw = (H + 7) // 8, (W + 7) // 8
        pa, pm = (np.zeros((th * 8, tw * 8), dtype=bool) for _ in range(2))
        pa[:H, :W], pm[:H, :W] = alive, miss
        ta = pa.reshape(th, 8, tw, 8).sum(axis=(1, 3))
        tm = pm.reshape(th, 8, tw, 8).sum(axis=(1, 3))
        reached = ta > 0
        out.append({"layer": j, "reached": round(float(alive.mean()), 5),
                    "missed": round(float(miss.mean()), 5),
                    "missed_of_reached": round(float(miss.sum() / max(alive.sum(), 1)), 5),
                    "tiles_all_missed_of_reached": round(
                        float(((tm == ta) & reached).sum() / max(reached.sum(), 1)), 5)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["C4", "C3"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--precisions", nargs="+", default=["exact", "fast"])
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per leg, alternated")
    ap.add_argument("--no-deviation", action="store_true", help="skip the fast deviation")
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    a = ap.parse_args()

    import numpy as np
    import torch
    import env_ref as ER
    import lights_ref as LR
    import materials_ref as MR
    import reflect_ref as RR
    from sdf3d_amd import Renderer, abi, scenes
    if not torch.cuda.is_available():
        raise SystemExit("env_probe: no HIP device (there is nothing to measure without one)")
    rd = Renderer("cuda:0")
    s = torch.cuda.current_stream()
    SKY, SUN, FOG = abi.ENV_SKY, abi.ENV_SUN, abi.ENV_FOG
    envs = {"sky": ER.environment(SKY | SUN), "fog": ER.environment(FOG),
            "all": ER.environment(SKY | SUN | FOG)}
    rec = {"configs": a.configs, "width": a.width, "height": a.height, "window_s": a.window,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "fog": list(ER.FOG_RANGE),
           "kernel_id": {p: rd.lib.sdf_kernel_id(abi.PRECISION_EXACT if p == "exact"
                                                 else abi.PRECISION_FAST).decode()
                         for p in a.precisions}, "results": []}

    for config in a.configs:
        for prec in a.precisions:
            p = abi.PRECISION_EXACT if prec == "exact" else abi.PRECISION_FAST
            f = scenes.config(config, a.width, a.height, precision=p)
            mats = MR.palette_for(f)
            lights = LR.rig(1)
            out = rd.alloc(f)[0]
            kw = dict(out=out, stream=s, lights=lights, materials=mats)
            for b in a.bounces:
                legs = {"reflect": lambda b=b: rd.render(f, reflect=(b, 1.0), **kw)}
                for name, env in envs.items():
                    legs[name] = (lambda b=b, env=env: rd.render(f, reflect=(b, 1.0), env=env,
                                                                  **kw))
                r = {"config": config, "precision": prec, "bounces": b}
                r.update(ratios(measure(torch, legs, s, a.window, a.repeats)))
                r["layers"] = miss_shares(np, rd, f, b, mats, lights, envs["sky"])
                rec["results"].append(r)
                print(json.dumps(r), flush=True)
            del out
            torch.cuda.empty_cache()

    if not a.no_deviation:
        # fast precision's composite against the reference, at the tests' shape
        dev = {}
        env = envs["all"]
        for name, pose in (("C4", 0), ("C3", 2), ("REF", 0)):
            f = MR.frame_of(name, pose, abi.PRECISION_FAST)
            mats = RR.materials_for(f) if name == "REF" else MR.palette_for(f)
            lights = LR.rig(1)
            for b in (1, 2):
                _, _, Sj, _ = G.own_layers(lambda r: G.both(rd, f, lights=lights, materials=mats,
                                                            reflect=r, env=env), b, 1.0)
                got = rd.render(f, lights=lights, materials=mats, reflect=(b, 1.0),
                                env=env)[0].cpu().numpy()
                d, left_out, pixels = ER.fast_deviation(f, mats, lights, env, b, got, Sj,
                                                        Sj[..., 0] > 0)
                dev[f"{name}_bounces{b}"] = {"max_abs_deviation": d, "pixels_left_out": left_out,
                                             "pixels": pixels}
        rec["fast_deviation"] = {"shape": list(ER.SHAPE), "flags": "SKY|SUN|FOG",
                                 "boundary": ER.BOUNDARY, "frames": dev,
                                 "largest": max(v["max_abs_deviation"] for v in dev.values())}
        print(json.dumps(rec["fast_deviation"]), flush=True)

    text = json.dumps(rec, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({"env_probe": "done", "kernel_id": rec["kernel_id"]}), flush=True)


if __name__ == "__main__":
    main()
