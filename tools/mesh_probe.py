#!/usr/bin/env python3
"""The mesh entry points against the route a caller had before them
(DESIGN.md "mesh").

For each scene (default C4 and C5) and each grid (default 128^3 and 256^3 cells
over the scene's box) these legs are timed with device events on one stream,
alternated window by window in one process, every one into buffers allocated
once:

  count          sdf_mesh_count (classification and the offset scan)
  emit           sdf_mesh_emit of that count: vertices and triangles
  emit_all       the same with a normal and an owning primitive per vertex
  count_dense    sdf_mesh_count with SDF_MESH_DENSE: every brick evaluated
  sample         sdf_sample of the same (n + 1)^3 lattice: what a caller had to
                 run (before copying the lattice out and meshing it themselves)

Each window runs back to back for at least --window seconds (after a warm-up
of every leg) and gives one ms-per-call figure; --repeats windows per leg; the
figure kept is the median, the spread that of the sample leg, (max - min) /
median.  Recorded too: the counts, and on the tests' two fast-precision grids
the deviation of the fast kernels from the reference (the bounds of
tests/test_gpu_mesh.py).

    python tools/mesh_probe.py --out profiles/mesh_C4.json
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

# the box meshed per scene: the CSG scene with its floor, the Mandelbulb's hull
BOXES = {"C4": ((-1.3, -0.1, -1.1), (1.3, 0.9, 1.1)), "C5": ((-0.6, -0.3, -0.6), (0.6, 0.9, 0.6))}
FAST_GRIDS = {"C1": ("C1", (-0.31, 0.13, -0.29), (0.05, 0.06, 0.055), (12, 10, 11)),
              "C4": ("C4", (-1.13, -0.11, -1.02), (0.12, 0.08, 0.11), (19, 11, 17))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["C4", "C5"])
    ap.add_argument("--cells", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--precisions", nargs="+", default=["exact", "fast"])
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per leg, alternated")
    ap.add_argument("--no-deviation", action="store_true", help="skip the fast deviation")
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    a = ap.parse_args()

    import numpy as np
    import torch
    import mesh_ref as M
    from sdf3d_amd import Renderer, abi, scenes
    from sdf3d_amd import renderer as R
    if not torch.cuda.is_available():
        raise SystemExit("mesh_probe: no HIP device (there is nothing to measure without one)")
    rd = Renderer("cuda:0")
    lib, dev = rd.lib, rd.device
    s = torch.cuda.current_stream()
    sp = C.c_void_p(s.cuda_stream)
    p = lambda x: C.c_void_p(x.data_ptr())
    prec_of = {"exact": abi.PRECISION_EXACT, "fast": abi.PRECISION_FAST}
    rec = {"scenes": a.scenes, "cells": a.cells, "boxes": BOXES, "window_s": a.window,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "kernel_id": {k: lib.sdf_kernel_id(prec_of[k]).decode() for k in a.precisions},
           "results": []}

    for name in a.scenes:
        lo, hi = BOXES[name]
        for n in a.cells:
            cell = tuple((hi[c] - lo[c]) / n for c in range(3))
            g = R.grid(lo, cell, n)
            gd = R.grid(lo, cell, n, dense=True)
            nbytes = int(lib.sdf_mesh_workspace_bytes(C.byref(g)))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            wsd = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            counts = torch.zeros(4, dtype=torch.int64, device=dev)
            countsd = torch.zeros(4, dtype=torch.int64, device=dev)
            ax = [torch.arange(n + 1, dtype=torch.float32, device=dev) * np.float32(cell[c])
                  + np.float32(lo[c]) for c in range(3)]
            Z, Y, X = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
            pts = torch.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], dim=1).contiguous()
            dist = torch.empty(pts.shape[0], dtype=torch.float32, device=dev)
            del X, Y, Z
            for prec in a.precisions:
                f = scenes.config(name, 64, 36, precision=prec_of[prec])
                sc, pa = C.byref(f.scene), C.byref(f.params)

                def count(g=g, ws=ws, counts=counts):
                    abi.check(lib.sdf_mesh_count(sc, pa, C.byref(g), p(ws), nbytes, p(counts), sp),
                              "sdf_mesh_count")
                count()
                torch.cuda.synchronize()
                nv, nt, ev, nb = (int(x) for x in counts.cpu().tolist())
                verts = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev)
                tris = torch.empty((max(nt, 1), 3), dtype=torch.int32, device=dev)
                nrm = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev)
                own = torch.empty(max(nv, 1), dtype=torch.int32, device=dev)
                plain = abi.sdf_mesh_out(p(verts), nv, p(tris), nt, None, None)
                every = abi.sdf_mesh_out(p(verts), nv, p(tris), nt, p(nrm), p(own))

                def emit(out=plain):
                    abi.check(lib.sdf_mesh_emit(sc, pa, C.byref(g), p(ws), nbytes, C.byref(out), sp),
                              "sdf_mesh_emit")

                def sample():
                    abi.check(lib.sdf_sample(sc, pa, p(pts), pts.shape[0], p(dist), None, sp),
                              "sdf_sample")
                legs = {"count": count, "emit": emit, "emit_all": lambda: emit(every),
                        "count_dense": lambda: count(gd, wsd, countsd), "sample": sample}
                ms = measure(torch, legs, s, a.window, a.repeats)
                med = {k: statistics.median(v) for k, v in ms.items()}
                r = {"scene": name, "cells": n, "precision": prec, "vertices": nv, "triangles": nt,
                     "bricks_evaluated": ev, "bricks": nb, "workspace_bytes": nbytes,
                     "lattice_bytes": 4 * pts.shape[0],
                     "ms": {k: round(v, 4) for k, v in med.items()},
                     "windows_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                     "sample_spread": round((max(ms["sample"]) - min(ms["sample"])) / med["sample"], 5),
                     "count_plus_emit_over_sample": round((med["count"] + med["emit"]) / med["sample"], 5),
                     "count_plus_emit_all_over_sample": round((med["count"] + med["emit_all"])
                                                              / med["sample"], 5),
                     "count_over_count_dense": round(med["count"] / med["count_dense"], 5)}
                rec["results"].append(r)
                print(json.dumps(r), flush=True)
                del verts, tris, nrm, own
            del pts, dist, ws, wsd
            torch.cuda.empty_cache()

    if "fast" in a.precisions and not a.no_deviation:
        devs = {}
        for case, (name, origin, cell, n) in FAST_GRIDS.items():
            ref = M.mesh(scenes.config(name, 64, 36), origin, cell, n)
            m = rd.mesh(scenes.config(name, 64, 36, precision=abi.PRECISION_FAST), origin, cell, n,
                        normal=True, prim=True)
            torch.cuda.synchronize()
            got = {"counts": m.counts, "verts": m.verts.cpu().numpy(), "tris": m.tris.cpu().numpy(),
                   "normal": m.normal.cpu().numpy(), "prim": m.prim.cpu().numpy()}
            devs[case] = M.fast_deviation(ref, got, cell)
        rec["fast_deviation"] = {"grids": devs,
                                 "largest_vertex_over_cell": max(v["vertex_over_cell"] for v in devs.values()),
                                 "largest_normal": max(v["normal"] for v in devs.values())}
        print(json.dumps(rec["fast_deviation"]), flush=True)

    text = json.dumps(rec, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({"mesh_probe": "done", "kernel_id": rec["kernel_id"]}), flush=True)


if __name__ == "__main__":
    main()
