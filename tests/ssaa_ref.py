"""NumPy statement of the supersampling resolve (include/sdf_abi.h
"Supersampling", sdf_params.samples = S).

A supersampled W x H frame is the S W x S H frame box-filtered: sub-sample
(i, j) of output pixel (x, y) is pixel (S x + i, S y + j) of the high
resolution frame, and per channel R, G, B the S x S colours c[i][j] (i along
x, j along y) are summed in fp32, round to nearest, no fused multiply-add, by
a balanced pairwise tree -- first along x, then along y, left / lower operand
first -- and scaled by 1 / S^2 (a power of two):

  S = 2   h_j = c[0][j] + c[1][j];                    out = (h_0 + h_1) * 0.25
  S = 4   a_j = (c[0][j] + c[1][j]) + (c[2][j] + c[3][j]);
          out = ((a_0 + a_1) + (a_2 + a_3)) * 0.0625

Alpha is 1.  Denormals are kept (NumPy's fp32 arithmetic is IEEE with gradual
underflow).  The render kernel's epilogue (render_kernel.inc ssaa_sum) must
equal this bit for bit.
"""
from __future__ import annotations

import numpy as np


def _pairs(a, axis):
    """Adjacent pairs along `axis` added, even (left / lower) operand first."""
    ev = [slice(None)] * a.ndim
    od = [slice(None)] * a.ndim
    ev[axis] = slice(0, None, 2)
    od[axis] = slice(1, None, 2)
    return (a[tuple(ev)] + a[tuple(od)]).astype(np.float32)


def resolve(hi, samples: int):
    """[S rows, S W, 4] float32 -> [rows, W, 4] float32 in the contract's tree
    order.  samples 0 or 1: the frame itself."""
    a = np.ascontiguousarray(hi, dtype=np.float32)
    s = int(samples)
    if s in (0, 1):
        return a.copy()
    if s not in (2, 4):
        raise ValueError(f"samples must be 0, 1, 2 or 4, got {samples}")
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] % s or a.shape[1] % s:
        raise ValueError(f"a [{s} rows, {s} W, 4] frame is needed, got {a.shape}")
    c = a[..., :3]
    with np.errstate(all="ignore"):
        for _ in range(1 if s == 2 else 2):     # along x: columns 2k, 2k + 1
            c = _pairs(c, 1)
        for _ in range(1 if s == 2 else 2):     # then along y
            c = _pairs(c, 0)
        c = (c * np.float32(1.0 / (s * s))).astype(np.float32)
    out = np.empty((a.shape[0] // s, a.shape[1] // s, 4), dtype=np.float32)
    out[..., :3] = c
    out[..., 3] = np.float32(1.0)
    return out


def resolve_sequential(hi, samples: int):
    """The same box filter summed row-major, one sub-sample after another (NOT
    the contract: the tests use it to show that the order is pinned)."""
    a = np.ascontiguousarray(hi, dtype=np.float32)
    s = int(samples)
    rows, w = a.shape[0] // s, a.shape[1] // s
    acc = np.zeros((rows, w, 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(s):
            for i in range(s):
                acc = (acc + a[j::s, i::s, :3]).astype(np.float32)
        acc = (acc * np.float32(1.0 / (s * s))).astype(np.float32)
    out = np.empty((rows, w, 4), dtype=np.float32)
    out[..., :3] = acc
    out[..., 3] = np.float32(1.0)
    return out
