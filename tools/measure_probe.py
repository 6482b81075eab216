#!/usr/bin/env python3
"""sdf_measure against the route a caller had before it (DESIGN.md "measure").

For each scene box (default C4 over the mesh profile's box, C4-deep over the
same box reaching 1 below the plane, so that bricks proven inside exist, and C5)
and each grid (default 128^3, 256^3 and 512^3 cells) these legs are timed with
device events on one stream, alternated window by window in one process, every
one into buffers allocated once:

  measure          sdf_measure (bricks skipped or taken in closed form)
  measure_dense    sdf_measure with SDF_MESH_DENSE: every brick evaluated
  measure_owners   sdf_measure with SDF_MEASURE_OWNERS
  baseline         what a caller had: sdf_sample at the same cell centres, then
                   torch reductions to the ten sums (inside = dist < iso summed
                   along each axis to three planes, the sums from the planes)

Each window runs back to back for at least --window seconds (after a warm-up
of every leg) and gives one ms-per-call figure; --repeats windows per leg; the
figure kept is the median, a leg's spread (max - min) / median.  Recorded too:
row 0 and the counts, and that the baseline's ten sums equal row 0's.

    python tools/measure_probe.py --out profiles/measure_C4.json
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
sys.path.insert(0, str(ROOT / "tools"))

from lights_probe import measure as timed  # noqa: E402  (the same windows and alternation)

# name -> (scene, box): the mesh profile's boxes, and C4's reaching 1 below the plane
BOXES = {"C4": ("C4", (-1.3, -0.1, -1.1), (1.3, 0.9, 1.1)),
         "C4-deep": ("C4", (-1.3, -1.0, -1.1), (1.3, 0.9, 1.1)),
         "C5": ("C5", (-0.6, -0.3, -0.6), (0.6, 0.9, 0.6))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", nargs="+", default=list(BOXES))
    ap.add_argument("--cells", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--precisions", nargs="+", default=["exact", "fast"])
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per leg, alternated")
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    a = ap.parse_args()

    import numpy as np
    import torch
    from sdf3d_amd import Renderer, abi, scenes
    from sdf3d_amd import renderer as R
    if not torch.cuda.is_available():
        raise SystemExit("measure_probe: no HIP device (there is nothing to measure without one)")
    rd = Renderer("cuda:0")
    lib, dev = rd.lib, rd.device
    s = torch.cuda.current_stream()
    sp = C.c_void_p(s.cuda_stream)
    p = lambda x: C.c_void_p(x.data_ptr())
    prec_of = {"exact": abi.PRECISION_EXACT, "fast": abi.PRECISION_FAST}
    OWN = abi.MEASURE_OWNERS
    rec = {"boxes": {k: BOXES[k] for k in a.boxes}, "cells": a.cells, "window_s": a.window,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "kernel_id": {k: lib.sdf_kernel_id(prec_of[k]).decode() for k in a.precisions},
           "results": []}

    for box in a.boxes:
        name, lo, hi = BOXES[box]
        for n in a.cells:
            cell = tuple((hi[c] - lo[c]) / n for c in range(3))
            g = R.grid(lo, cell, n)
            gd = R.grid(lo, cell, n, dense=True)
            nb = {fl: int(lib.sdf_measure_workspace_bytes(C.byref(g), fl)) for fl in (0, OWN)}
            ws = torch.empty(nb[OWN], dtype=torch.uint8, device=dev)
            rows = torch.zeros((abi.MEASURE_ROWS, abi.MEASURE_SLOTS), dtype=torch.int64, device=dev)
            counts = torch.zeros(4, dtype=torch.int64, device=dev)
            # the cell centres as sdf_measure forms them: origin + (i + 0.5) cell in fp32
            ax = [(torch.arange(n, dtype=torch.float32, device=dev) + 0.5) * np.float32(cell[c])
                  + np.float32(lo[c]) for c in range(3)]
            Z, Y, X = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
            pts = torch.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], dim=1).contiguous()
            dist = torch.empty(pts.shape[0], dtype=torch.float32, device=dev)
            del X, Y, Z
            idx = torch.arange(n, dtype=torch.int64, device=dev)
            sums = torch.zeros(10, dtype=torch.int64, device=dev)
            for prec in a.precisions:
                f = scenes.config(name, 64, 36, precision=prec_of[prec])
                sc, pa = C.byref(f.scene), C.byref(f.params)

                def run(grid=g, flags=0):
                    abi.check(lib.sdf_measure(sc, pa, C.byref(grid), flags, p(ws), nb[flags], p(rows),
                                              p(counts), sp), "sdf_measure")

                def baseline():
                    abi.check(lib.sdf_sample(sc, pa, p(pts), pts.shape[0], p(dist), None, sp),
                              "sdf_sample")
                    inside = (dist < 0.0).view(n, n, n)            # [i2, i1, i0]
                    xy = inside.sum(dim=0, dtype=torch.int64)      # [i1, i0]
                    xz = inside.sum(dim=1, dtype=torch.int64)      # [i2, i0]
                    yz = inside.sum(dim=2, dtype=torch.int64)      # [i2, i1]
                    c0, c1, c2 = xy.sum(dim=0), xy.sum(dim=1), xz.sum(dim=1)
                    sums[0] = c0.sum()
                    sums[1], sums[2], sums[3] = (c0 * idx).sum(), (c1 * idx).sum(), (c2 * idx).sum()
                    sums[4], sums[5] = (c0 * idx * idx).sum(), (c1 * idx * idx).sum()
                    sums[6] = (c2 * idx * idx).sum()
                    sums[7] = (xy * idx[:, None] * idx[None, :]).sum()
                    sums[8] = (xz * idx[:, None] * idx[None, :]).sum()
                    sums[9] = (yz * idx[:, None] * idx[None, :]).sum()

                run()
                baseline()
                torch.cuda.synchronize()
                row0, cn = rows[0].cpu().tolist(), counts.cpu().tolist()
                same = sums.cpu().tolist() == row0[:10]
                legs = {"measure": run, "measure_dense": lambda: run(gd),
                        "measure_owners": lambda: run(g, OWN), "baseline": baseline}
                ms = timed(torch, legs, s, a.window, a.repeats)
                med = {k: statistics.median(v) for k, v in ms.items()}
                spread = {k: round((max(v) - min(v)) / med[k], 5) for k, v in ms.items()}
                r = {"box": box, "scene": name, "cells": n, "precision": prec, "row0": row0,
                     "bricks_evaluated": cn[0], "bricks_closed_form": cn[1], "bricks": cn[2],
                     "baseline_sums_equal_row0": same,
                     "workspace_bytes": nb, "baseline_bytes": 16 * pts.shape[0],
                     "ms": {k: round(v, 4) for k, v in med.items()},
                     "windows_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                     "spread": spread,
                     "measure_over_dense": round(med["measure"] / med["measure_dense"], 5),
                     "dense_over_baseline": round(med["measure_dense"] / med["baseline"], 5),
                     # a leg is faster than another when its slowest window beats the other's fastest
                     "measure_beats_dense": max(ms["measure"]) < min(ms["measure_dense"]),
                     "dense_no_slower_than_baseline": min(ms["measure_dense"]) <= max(ms["baseline"])}
                rec["results"].append(r)
                print(json.dumps(r), flush=True)
            del pts, dist, ws
            torch.cuda.empty_cache()

    text = json.dumps(rec, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({"measure_probe": "done", "kernel_id": rec["kernel_id"]}), flush=True)


if __name__ == "__main__":
    main()
