#!/usr/bin/env python3
"""sdf_sample_grad measured (DESIGN.md "grad").

Accuracy: for every test scene of tests/grad_ref.py (REF, C1, C4, three random
scenes, the 42 two-primitive coverage scenes) and each precision, the kernel's
error by the metric of tests/test_gpu_grad.py over E32, the float32 reference's
error by the same metric (the tests bound the ratio by 4 in exact and 8 in fast
precision).  Recorded per scene and precision, with the largest ratios.

Time: sdf_sample_grad with every output (dist, grad_points, grad_prims) on 2^20
points of the C4 scene beside sdf_sample on the same points, with device events
on one stream, alternated window by window (tools/lights_probe.py measure); also
without grad_prims, which skips the reduction.  The figure kept is the median
of --repeats windows; the spread is (max - min) / median of the sample leg.

    python tools/grad_probe.py --out profiles/grad_C4.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--precisions", nargs="+", default=["exact", "fast"])
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per leg, alternated")
    ap.add_argument("--no-accuracy", action="store_true", help="skip the error ratios")
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    a = ap.parse_args()

    import torch
    import grad_ref
    from sdf3d_amd import Renderer, abi, scenes
    if not torch.cuda.is_available():
        raise SystemExit("grad_probe: no HIP device (there is nothing to measure without one)")
    rd = Renderer("cuda:0")
    lib, dev = rd.lib, rd.device
    s = torch.cuda.current_stream()
    sp = C.c_void_p(s.cuda_stream)
    p = lambda x: C.c_void_p(x.data_ptr())
    prec_of = {"exact": abi.PRECISION_EXACT, "fast": abi.PRECISION_FAST}
    rec = {"points": a.points, "window_s": a.window, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0),
           "kernel_id": {k: lib.sdf_kernel_id(prec_of[k]).decode() for k in a.precisions},
           "timing": [], "accuracy": []}

    n = a.points
    pts = torch.from_numpy(grad_ref.cube_points(n, seed=1)).to(dev)
    up = torch.ones(n, dtype=torch.float32, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    gp = torch.empty((n, 3), dtype=torch.float32, device=dev)
    gt = torch.empty((16, 16), dtype=torch.float32, device=dev)
    nbytes = int(lib.sdf_grad_workspace_bytes(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    every = abi.sdf_grad_out(p(dist), p(gp), p(gt))
    no_prims = abi.sdf_grad_out(p(dist), p(gp), None)
    for prec in a.precisions:
        f = scenes.config("C4", 64, 36, precision=prec_of[prec])
        sc, pa = C.byref(f.scene), C.byref(f.params)

        def grad(out=every):
            abi.check(lib.sdf_sample_grad(sc, pa, p(pts), n, p(up), C.byref(out), p(ws), nbytes, sp),
                      "sdf_sample_grad")

        def sample():
            abi.check(lib.sdf_sample(sc, pa, p(pts), n, p(dist), None, sp), "sdf_sample")
        legs = {"grad": grad, "grad_no_prims": lambda: grad(no_prims), "sample": sample}
        ms = measure(torch, legs, s, a.window, a.repeats)
        med = {k: statistics.median(v) for k, v in ms.items()}
        r = {"scene": "C4", "precision": prec, "workspace_bytes": nbytes,
             "ms": {k: round(v, 4) for k, v in med.items()},
             "windows_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
             "sample_spread": round((max(ms["sample"]) - min(ms["sample"])) / med["sample"], 5),
             "grad_over_sample": round(med["grad"] / med["sample"], 4),
             "grad_no_prims_over_sample": round(med["grad_no_prims"] / med["sample"], 4)}
        rec["timing"].append(r)
        print(json.dumps(r), flush=True)

    if not a.no_accuracy:
        points = grad_ref.cube_points(200)
        worst = {k: {"points": 0.0, "prims": 0.0} for k in a.precisions}
        for name, frame in grad_ref.all_frames().items():
            c = grad_ref.Case(frame, points)
            e_pts, e_prims = c.e32()
            P = torch.from_numpy(c.points).to(dev)
            U = torch.from_numpy(c.upstream).to(dev)
            for prec in a.precisions:
                f = frame.copy()
                f.params.precision = prec_of[prec]
                g = rd.sample_grad(f, P, U)
                torch.cuda.synchronize()
                k_pts = c.points_error(g.grad_points.cpu().numpy())
                k_prims = c.prims_error(g.grad_prims.cpu().numpy())
                r = {"scene": name, "precision": prec, "excluded": int((~c.keep).sum()),
                     "points_error": k_pts, "points_e32": e_pts,
                     "points_ratio": round(k_pts / e_pts, 3) if e_pts > 0 else None,
                     "prims_error": k_prims, "prims_e32": e_prims,
                     "prims_ratio": round(k_prims / e_prims, 3)}
                rec["accuracy"].append(r)
                worst[prec]["points"] = max(worst[prec]["points"], r["points_ratio"] or 0.0)
                worst[prec]["prims"] = max(worst[prec]["prims"], r["prims_ratio"])
        rec["largest_ratio"] = worst
        print(json.dumps({"largest_ratio": worst}), flush=True)

    text = json.dumps(rec, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({"grad_probe": "done", "kernel_id": rec["kernel_id"]}), flush=True)


if __name__ == "__main__":
    main()
