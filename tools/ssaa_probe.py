#!/usr/bin/env python3
"""Fused supersampling against what it replaces (DESIGN.md "Supersampling").

For a W x H output (default C4 at 1920 x 1080) and S in {2, 4}, two paths
are timed with device events on one stream, alternated window by window in
one process:

  baseline  sdf_render of the S W x S H frame as RGBA32F (samples = 0): the
            render a user makes today before a resolve pass of their own --
            the resolve itself and its buffer are NOT charged to the baseline
  ssaa      sdf_render of the W x H frame with samples = S

Each window renders back to back for at least --window seconds (after a
warm-up of both shapes) and gives one ms-per-frame figure; --repeats windows
per path.  The spread is that of the baseline's own repeats, (max - min) /
median: the fused path may be slower than the baseline by no more than that.
The two outputs are compared once: ssaa == resolve(baseline) in the
contract's tree order (tests/ssaa_ref.py), bit for bit.

The write traffic is computed from the shapes, not measured: the baseline
stores 16 S^2 bytes per output pixel (and a resolve pass reads them again and
writes the output), the fused path the output format's bytes per pixel.

    python tools/ssaa_probe.py --out profiles/ssaa_C4.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--precisions", nargs="+", default=["exact", "fast"])
    ap.add_argument("--format", default="rgba32f", choices=["rgba32f", "rgba16f", "rgba8", "rgb32f"],
                    help="output format of the fused path (the baseline is RGBA32F)")
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per path, alternated")
    ap.add_argument("--no-check", action="store_true", help="skip the bit comparison")
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    a = ap.parse_args()

    import torch
    from sdf3d_amd import Renderer, abi, scenes
    if not torch.cuda.is_available():
        raise SystemExit("ssaa_probe: no HIP device (there is nothing to measure without one)")
    rd = Renderer("cuda:0")
    s = torch.cuda.current_stream()
    fmt = abi.FORMAT_NAMES[a.format]
    bpp = rd.lib.sdf_format_bytes(fmt)
    rec = {"config": a.config, "width": a.width, "height": a.height, "format": a.format,
           "window_s": a.window, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "kernel_id": {p: rd.lib.sdf_kernel_id(abi.PRECISION_EXACT if p == "exact"
                                                 else abi.PRECISION_FAST).decode()
                         for p in a.precisions},
           "results": []}
    for prec in a.precisions:
        for S in a.samples:
            lo = scenes.config(a.config, a.width, a.height,
                               precision=abi.PRECISION_EXACT if prec == "exact"
                               else abi.PRECISION_FAST)
            hi = lo.copy()
            hi.params.width, hi.params.height = S * a.width, S * a.height
            lo.params.samples = S
            lo.params.output_format = fmt
            out_hi = rd.alloc(hi)[0]
            out_lo = rd.alloc(lo)[0]
            legs = {"baseline": lambda: rd.render(hi, out=out_hi, stream=s),
                    "ssaa": lambda: rd.render(lo, out=out_lo, stream=s)}
            est = {}
            for k, fn in legs.items():          # warm-up of both shapes, and a first estimate
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                est[k] = (time.perf_counter() - t0) * 1e3 / 3
            ms = {k: [] for k in legs}
            calls = {k: 0 for k in legs}
            for _ in range(a.repeats):
                for k, fn in legs.items():
                    m, n = window(torch, fn, s, a.window, est[k])
                    ms[k].append(m)
                    calls[k] += n
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = (max(ms["baseline"]) - min(ms["baseline"])) / med["baseline"]
            r = {"precision": prec, "samples": S,
                 "baseline_shape": [S * a.width, S * a.height],
                 "baseline_ms": round(med["baseline"], 4), "ssaa_ms": round(med["ssaa"], 4),
                 "baseline_windows_ms": [round(x, 4) for x in ms["baseline"]],
                 "ssaa_windows_ms": [round(x, 4) for x in ms["ssaa"]],
                 "calls": calls,
                 "baseline_spread": round(spread, 5),
                 "ssaa_over_baseline": round(med["ssaa"] / med["baseline"], 5),
                 "within_spread": bool(med["ssaa"] <= med["baseline"] * (1.0 + spread)),
                 # from shapes, not measured
                 "baseline_write_bytes": 16 * S * S * a.width * a.height,
                 "ssaa_write_bytes": bpp * a.width * a.height,
                 "user_resolve_bytes_avoided": (16 * S * S + 16) * a.width * a.height}
            if not a.no_check and fmt == abi.FORMAT_RGBA32F:
                import ssaa_ref
                want = ssaa_ref.resolve(out_hi.cpu().numpy(), S)
                got = out_lo.cpu().numpy()
                r["bit_exact"] = bool((want.view("uint32") == got.view("uint32")).all())
            rec["results"].append(r)
            print(json.dumps(r), flush=True)
            del out_hi, out_lo
            torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({"ssaa_probe": "done", "kernel_id": rec["kernel_id"]}), flush=True)


if __name__ == "__main__":
    main()
