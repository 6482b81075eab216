"""NumPy statement of the multi-light colour (include/sdf_abi.h "Lights",
sdf_render_lights) and the test rig its tests share.

A pixel's geometry -- the primary march, P, N and the ambient-occlusion term
ao -- does not depend on the light.  Light i contributes (dif_i, x_i): channels
1 and 2 of the SDF_FORMAT_SHADE32F render with that light alone, and spec_i =
x_i ^ shininess as the precision forms it.  Per channel c, in fp32 round to
nearest, lights in index order, never reassociated:

    la     = sum of lights[i].ambient, fp32, index order
    acc    = RN(RN(la * amb[c]) * ao)
    d, s   = RN(dif_i * color_i[c]), RN(spec_i * color_i[c])   with LIGHTS_COLOR
           = dif_i, spec_i                                       otherwise
    exact    acc = RN(RN(acc + RN(d * dif[c])) + RN(s * ref[c]))
    fast     acc = fma(s, ref[c], fma(d, dif[c], acc))           each fma rounded once

Alpha is 1.  Exact precision takes spec_i = RN32(pow64(x_i, shininess)), the
oracle's own form (oracle.colour_from_terms); fast precision's spec_i is the
hardware's exp2 / log2, so its callers pass the kernel's own values (`specs`).
"""
from __future__ import annotations

import numpy as np

from sdf3d_amd import abi

f32 = np.float32

RIG = [(-4, 3, 3), (-2, 0.6, 1), (5, 5, 0), (0.5, 6, -4), (0, -3, 0.5), (3, 2, 4), (-5, 4, -2),
       (0.2, 8, 0.3)]
AMBIENTS = [0.1, 0.05, 0.02, 0.01, 0.0, 0.0, 0.0, 0.0]
COLOURS = [(1, 0.5, 0.25), (0.25, 0.5, 1), (0.7, 0.7, 0.7), (2, 0, 0.5)]
SHAPE = (37, 23)    # partial 8 x 8 tiles in x and y, a last block of 7 rows
FRAMES = [("REF", 0), ("C2", 1), ("C3", 2), ("C4", 0), ("C5", 3), ("C1", 0)]


def rig(n: int):
    """The first n lights of the rig (the fifth is below the ground plane)."""
    out = []
    for i in range(n):
        l = abi.sdf_light()
        for c in range(3):
            l.pos[c] = RIG[i][c]
            l.color[c] = COLOURS[i % len(COLOURS)][c]
        l.ambient = AMBIENTS[i]
        out.append(l)
    return out


def with_light(frame, light):
    """A copy of `frame` lit by `light` alone."""
    g = frame.copy()
    g.light = type(light).from_buffer_copy(light)
    return g


def fma32(a, b, c):
    """fma(a, b, c) of float32 arrays rounded ONCE to float32.

    The product of two floats is exact in fp64 (48 bits).  s = p + c in fp64 is
    rounded once already; TwoSum gives its error e, and where e != 0 and s's
    last mantissa bit is even, s moves one fp64 ulp towards the exact sum
    (round to odd).  A value rounded to odd at 53 bits then rounds to 24 bits
    (or to a float32 subnormal) exactly as the unrounded sum would -- midpoints
    of float32 included, which a plain fp64 multiply-add would round twice."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        cc = c.astype(np.float64)
        s = p + cc
        bb = s - p
        e = (p - (s - bb)) + (cc - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        towards = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, towards), s)
        return s.astype(f32)


def spec_exact(x, shininess):
    """Exact precision's x ^ shininess: fp64 pow rounded to fp32 once."""
    with np.errstate(all="ignore"):
        return np.power(np.asarray(x, f32).astype(np.float64),
                        np.float64(f32(shininess))).astype(f32)


def compose(frame, terms_list, lights, flags=0, precision=abi.PRECISION_EXACT, specs=None):
    """The L-light frame from the lights' single-light terms.

    terms_list[i]: [rows, W, 4] float32 (ao, dif_i, x_i, 1) of light i (ao is
    read from light 0's: it is the same for all).  specs[i]: spec_i, needed in
    fast precision; None: exact precision's pow.  Returns [rows, W, 4]."""
    assert len(terms_list) == len(lights) >= 1
    exact = precision == abi.PRECISION_EXACT
    if specs is None:
        assert exact, "fast precision's spec is the kernel's own: pass `specs`"
        specs = [spec_exact(t[..., 2], frame.material.shininess) for t in terms_list]
    m = frame.material
    ao = np.asarray(terms_list[0][..., 0], f32)
    la = f32(lights[0].ambient)
    for l in lights[1:]:
        la = f32(la + f32(l.ambient))
    out = np.empty(terms_list[0].shape, dtype=f32)
    with np.errstate(all="ignore"):
        for c in range(3):
            lam = f32(la * f32(m.amb[c]))
            md, mr = f32(m.dif[c]), f32(m.ref[c])
            acc = (lam * ao).astype(f32)
            for l, t, sp in zip(lights, terms_list, specs):
                d, s = np.asarray(t[..., 1], f32), np.asarray(sp, f32)
                if flags & abi.LIGHTS_COLOR:
                    col = f32(l.color[c])
                    d, s = (d * col).astype(f32), (s * col).astype(f32)
                if exact:
                    acc = (acc + (d * md).astype(f32)).astype(f32)
                    acc = (acc + (s * mr).astype(f32)).astype(f32)
                else:
                    acc = fma32(s, mr, fma32(d, md, acc))
            out[..., c] = acc
    out[..., 3] = f32(1.0)
    return out
