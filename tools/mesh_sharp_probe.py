#!/usr/bin/env python3
"""sdf_mesh_emit_sharp against sdf_mesh_emit (DESIGN.md "mesh_sharp").

C4 on a grid of --cells^3 cells over the scene's box (tools/mesh_probe.py's),
in each precision; these legs are timed with device events on one stream,
alternated window by window in one process, into buffers allocated once,
after one sdf_mesh_count:

  emit           sdf_mesh_emit: vertices and triangles
  emit_sharp     sdf_mesh_emit_sharp with --sharp R,K (default 4,16), the same
  emit_parent    sdf_mesh_emit of another build of the library (--parent-lib: the
                 commit before this entry point), on its own count of the grid

Each window runs back to back for at least --window seconds (after a warm-up
of every leg) and gives one ms-per-call figure; --repeats windows per leg; the
figure kept is the median, the spread that of the emit leg, (max - min) /
median.  Recorded too: the lattice's crossing edges (sign changes between
neighbours of sdf_sample's lattice; a brick refines the edges on its border
again, and the plane between its two slabs twice), what the kernel runs per
crossing, and on the tests' grids the deviation of the fast sharp mesh from the
exact one (the bound of tests/test_gpu_mesh_sharp.py).

    python tools/mesh_sharp_probe.py --out profiles/mesh_sharp_C4.json
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
from mesh_probe import BOXES  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--sharp", default="4,16")
    ap.add_argument("--precisions", nargs="+", default=["exact", "fast"])
    ap.add_argument("--parent-lib", default=None, help="libsdf3d.so of the commit before")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per leg, alternated")
    ap.add_argument("--no-deviation", action="store_true", help="skip the fast deviation")
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    a = ap.parse_args()
    refine, iterations = (int(x) for x in a.sharp.split(","))

    import numpy as np
    import torch
    from sdf3d_amd import Renderer, abi, scenes
    from sdf3d_amd import renderer as R
    if not torch.cuda.is_available():
        raise SystemExit("mesh_sharp_probe: no HIP device (there is nothing to measure without one)")
    rd = Renderer("cuda:0")
    lib, dev = rd.lib, rd.device
    parent = abi.load_library(a.parent_lib, any_version=True) if a.parent_lib else None
    s = torch.cuda.current_stream()
    sp = C.c_void_p(s.cuda_stream)
    p = lambda x: C.c_void_p(x.data_ptr())
    prec_of = {"exact": abi.PRECISION_EXACT, "fast": abi.PRECISION_FAST}
    name, n = "C4", a.cells
    lo, hi = BOXES[name]
    cell = tuple((hi[c] - lo[c]) / n for c in range(3))
    g = R.grid(lo, cell, n)
    nbytes = int(lib.sdf_mesh_workspace_bytes(C.byref(g)))
    sharp = abi.sdf_mesh_sharp(refine, iterations, 0, 0)
    rec = {"scene": name, "cells": n, "box": BOXES[name], "sharp": [refine, iterations],
           "window_s": a.window, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "kernel_id": {k: lib.sdf_kernel_id(prec_of[k]).decode() for k in a.precisions},
           "parent_kernel_id": {k: parent.sdf_kernel_id(prec_of[k]).decode() for k in a.precisions}
           if parent else None,
           "per_crossing": {"evaluations": refine, "gradient_forward_folds": 1,
                            "gradient_backward_sweeps": 1,
                            "scene_evaluations_implied": refine + 1},
           "results": []}

    for prec in a.precisions:
        f = scenes.config(name, 64, 36, precision=prec_of[prec])
        sc, pa = C.byref(f.scene), C.byref(f.params)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        wsp = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
        abi.check(lib.sdf_mesh_count(sc, pa, C.byref(g), p(ws), nbytes, p(counts), sp), "sdf_mesh_count")
        if parent:
            abi.check(parent.sdf_mesh_count(sc, pa, C.byref(g), p(wsp), nbytes, p(counts), sp),
                      "sdf_mesh_count (parent)")
        torch.cuda.synchronize()
        nv, nt, ev, nb = (int(x) for x in counts.cpu().tolist())
        # the crossing edges, from sdf_sample's lattice in slabs of planes
        crossings = 0
        ax = [torch.arange(n + 1, dtype=torch.float32, device=dev) * np.float32(cell[c]) + np.float32(lo[c])
              for c in range(3)]
        for k0 in range(0, n + 1, 32):
            k1 = min(k0 + 33, n + 1)                      # one plane of overlap with the next slab
            Z, Y, X = torch.meshgrid(ax[2][k0:k1], ax[1], ax[0], indexing="ij")
            pts = torch.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], dim=1).contiguous()
            d = torch.empty(pts.shape[0], dtype=torch.float32, device=dev)
            abi.check(lib.sdf_sample(sc, pa, p(pts), pts.shape[0], p(d), None, sp), "sdf_sample")
            torch.cuda.synchronize()
            ins = d.reshape(k1 - k0, n + 1, n + 1) < 0
            own = ins if k1 == n + 1 else ins[:-1]        # the planes whose own edges are counted here
            crossings += int((own[:, :, 1:] != own[:, :, :-1]).sum()) + int((own[:, 1:] != own[:, :-1]).sum())
            crossings += int((ins[1:] != ins[:-1]).sum())
            del pts, d, X, Y, Z
            if k1 == n + 1:
                break
        verts = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev)
        tris = torch.empty((max(nt, 1), 3), dtype=torch.int32, device=dev)
        out = abi.sdf_mesh_out(p(verts), nv, p(tris), nt, None, None)

        def emit():
            abi.check(lib.sdf_mesh_emit(sc, pa, C.byref(g), p(ws), nbytes, C.byref(out), sp), "sdf_mesh_emit")

        def emit_sharp():
            abi.check(lib.sdf_mesh_emit_sharp(sc, pa, C.byref(g), C.byref(sharp), p(ws), nbytes,
                                              C.byref(out), sp), "sdf_mesh_emit_sharp")

        def emit_parent():
            abi.check(parent.sdf_mesh_emit(sc, pa, C.byref(g), p(wsp), nbytes, C.byref(out), sp),
                      "sdf_mesh_emit (parent)")
        legs = {"emit": emit, "emit_sharp": emit_sharp}
        if parent:
            legs["emit_parent"] = emit_parent
        ms = measure(torch, legs, s, a.window, a.repeats)
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = (max(ms["emit"]) - min(ms["emit"])) / med["emit"]
        r = {"precision": prec, "vertices": nv, "triangles": nt, "bricks_evaluated": ev, "bricks": nb,
             "crossing_edges": crossings,
             "ms": {k: round(v, 4) for k, v in med.items()},
             "windows_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
             "emit_spread": round(spread, 5),
             "emit_sharp_over_emit": round(med["emit_sharp"] / med["emit"], 4),
             "ns_per_crossing_edge": round((med["emit_sharp"] - med["emit"]) * 1e6 / max(crossings, 1), 3)}
        if parent:
            r["emit_over_emit_parent"] = round(med["emit"] / med["emit_parent"], 5)
            r["emit_differs_from_parent_by_more_than_spread"] = bool(
                abs(med["emit"] - med["emit_parent"]) > spread * med["emit_parent"])
        rec["results"].append(r)
        print(json.dumps(r), flush=True)
        del verts, tris, ws, wsp
        torch.cuda.empty_cache()

    if "fast" in a.precisions and not a.no_deviation:
        import mesh_sharp_ref as T
        devs = {}
        for case in ("C4", "C4-generic", "C4-carved", "BOX-cubic"):
            scene, spec = T.CASES[case]
            m = {}
            for prec in (abi.PRECISION_EXACT, abi.PRECISION_FAST):
                m[prec] = rd.mesh(T.frame_of(scene, prec), *spec, sharp=(refine, iterations))
            torch.cuda.synchronize()
            e, q = m[abi.PRECISION_EXACT], m[abi.PRECISION_FAST]
            same = e.counts[:2] == q.counts[:2] and bool(torch.equal(e.tris, q.tris))
            dv = float(((q.verts.double() - e.verts.double()).abs()
                        / torch.tensor(spec[1], dtype=torch.float64, device=dev)).max()) if same else None
            devs[case] = {"same_connectivity": same, "vertex_over_cell": dv}
        rec["fast_deviation"] = {"grids": devs, "C4_vertex_over_cell": devs["C4"]["vertex_over_cell"]}
        print(json.dumps(rec["fast_deviation"]), flush=True)

    text = json.dumps(rec, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({"mesh_sharp_probe": "done", "kernel_id": rec["kernel_id"]}), flush=True)


if __name__ == "__main__":
    main()
