"""The return code of every shading entry point for faulty requests, held
against a recording (tests/golden/request_codes.json).  No GPU.

A request is refused for the first rule it breaks, so the code of a request with
two faults tells the order the rules run in wherever SDF_E_UNSUPPORTED competes
with SDF_E_INVALID_ARG (include/sdf_abi.h: differing shininess beside a NaN
``ref`` at one bounce stays UNSUPPORTED).  FAULTS is a fixed, ordered list of
single mutations of one valid C3 request; the test applies every one of them
and every ordered pair of distinct ones to

  sdf_validate_lights, _materials, _reflect, _env, _rays, _points

and to the matching sdf_render_* / sdf_shade_points, which are handed null
buffers (sdf_shade_points: no points) and a stream handle that must never be
touched, and asserts the recorded codes; a render entry point must also return
its validator's code wherever that is not SDF_OK.  A fault that means nothing
to an entry point (an environment to sdf_render_lights, a frame's width to a
list of rays) is skipped for it.

The recording is of the commit before the request validator became one
function, made with ``python tests/test_request_codes.py --record`` in a build
of that commit.  It is never regenerated from the code under test."""
import ctypes as C
import json
import math
import sys
from pathlib import Path

if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import env_ref as ER
import lights_ref as LR
import reflect_ref as RR
from sdf3d_amd import abi, scenes

GOLDEN = Path(__file__).resolve().parent / "golden" / "request_codes.json"
BOGUS_STREAM = C.c_void_p(0xDEAD0000BEEF0)     # never dereferenced: no call here reaches a device
PTR = 0x1000                                   # a non-null "device pointer", likewise
LETTER = {abi.SDF_OK: "K", abi.SDF_E_INVALID_ARG: "I", abi.SDF_E_UNSUPPORTED: "U"}
SKIPPED, SELF = ".", "-"
NAN = math.nan

# entry point -> (validator, render); FRAMES render a frame through a camera
ENTRIES = {"lights": ("sdf_validate_lights", "sdf_render_lights"),
           "materials": ("sdf_validate_materials", "sdf_render_materials"),
           "reflect": ("sdf_validate_reflect", "sdf_render_reflect"),
           "env": ("sdf_validate_env", "sdf_render_env"),
           "rays": ("sdf_validate_rays", "sdf_render_rays"),
           "points": ("sdf_validate_points", "sdf_shade_points")}
FRAMES = ("lights", "materials", "reflect", "env")
ALL = tuple(ENTRIES)
MATERIALS = ("materials", "reflect", "env", "rays", "points")   # take a material table
REFLECT = ("reflect", "env", "rays")                            # take an sdf_reflect
ENV = ("env", "rays")                                           # take an sdf_environment


class Request:
    """A valid C3 request at the ABI tests' shape that collapses to sdf_render:
    one plain light, eight copies of the frame's material, no bounce, no
    environment flag."""

    def __init__(self):
        self.f = f = scenes.config("C3", *LR.SHAPE)
        self.lights = [f.light]
        self.nlights = None            # None: len(lights)
        self.light_flags = 0
        self.materials = [type(f.material).from_buffer_copy(f.material) for _ in range(8)]
        self.nmaterials = None
        self.reflect = RR.reflect(0, 1.0)
        self.env = ER.environment(0)
        self.null = set()              # the pointers passed as NULL


def null(name):
    return lambda q: q.null.add(name)


def set_(path, value):
    """q.<path> = value; a trailing integer indexes an array."""
    def apply(q):
        *head, last = path.split(".")
        o = q
        for name in head:
            o = o[int(name)] if name.isdigit() else getattr(o, name)
        if last.isdigit():
            o[int(last)] = value
        else:
            setattr(o, last, value)
    return apply


def both(*fs):
    return lambda q: [f(q) for f in fs]


def palette(q):
    q.materials = scenes.palette(8)


def two_lights(q):
    q.lights = LR.rig(2)


def nan_ref(q):
    """A NaN ``ref`` where it is looked at: at one bounce or more."""
    q.materials[2].ref[1] = NAN
    q.reflect.bounces = max(q.reflect.bounces, 1)


def singular_view(q):
    for i in range(4):
        q.f.camera.view[4 + i] = 0.0


def zero_capsule(q):
    p = q.f.scene.prims[4]
    assert p.kind == abi.PRIM_CAPSULE
    for i in range(3):
        p.p[3 + i] = p.p[i]


def stream(fmt):
    return set_("f.params.output_format", fmt)


def streams(name, fault, applies):
    return [(f"{name}+{n}", both(fault, stream(fmt)), tuple(e for e in applies if e != "points"))
            for n, fmt in (("TILES", abi.FORMAT_TILES), ("SHADE32F", abi.FORMAT_SHADE32F))]


# (name, mutation, the entry points it means something to).  A list of rays or
# points has no camera and no frame size; sdf_shade_points has neither samples
# nor an output format, and sdf_render_rays takes a null reflect.
FAULTS = [
    ("null lights", null("lights"), ALL),
    ("null materials", null("materials"), ALL),
    ("null reflect", null("reflect"), ("reflect", "env")),
    ("null params", null("params"), ALL),
    ("null scene", null("scene"), ALL),
    ("nlights 0", set_("nlights", 0), ALL),
    ("nlights 9", set_("nlights", 9), ALL),
    ("unknown light flag", set_("light_flags", 0x2), ALL),
    ("NaN light position", set_("lights.0.pos.1", NAN), ALL),
    ("NaN colour with LIGHTS_COLOR",
     both(set_("light_flags", abi.LIGHTS_COLOR), set_("lights.0.color.2", NAN)), ALL),
    ("wrong nmaterials", set_("nmaterials", 7), MATERIALS),
    ("differing shininess", set_("materials.5.shininess", 13.0), MATERIALS),
    ("NaN ref", nan_ref, REFLECT),
    ("bounces 5", set_("reflect.bounces", 5), REFLECT),
    ("layer above bounces", set_("reflect.layer", abi.MAX_BOUNCES + 1), REFLECT),
    ("REFLECT_WEIGHT with layer -1",
     both(set_("reflect.flags", abi.REFLECT_WEIGHT), set_("reflect.layer", -1)), REFLECT),
    ("NaN strength", set_("reflect.strength", NAN), REFLECT),
    ("ENV_SUN without ENV_SKY", set_("env.flags", abi.ENV_SUN), ENV),
    ("empty fog range", both(set_("env.flags", abi.ENV_FOG), set_("env.fog_start", 4.0),
                             set_("env.fog_end", 1.0)), ENV),
    *streams("palette", palette, MATERIALS),
    *streams("two lights", two_lights, ALL),
    *streams("one bounce", set_("reflect.bounces", 1), REFLECT),
    *streams("sky", set_("env.flags", abi.ENV_SKY), ENV),
    ("samples 2 with TILES", both(set_("f.params.samples", 2), stream(abi.FORMAT_TILES)),
     FRAMES + ("rays",)),
    ("samples 3", set_("f.params.samples", 3), FRAMES + ("rays",)),
    ("width 0", set_("f.params.width", 0), FRAMES),
    ("singular view matrix", singular_view, FRAMES),
    ("primitive kind out of range", set_("f.scene.prims.3.kind", 7), ALL),
    ("capsule of zero length", zero_capsule, ALL),
    ("smooth k of 0", set_("f.scene.prims.2.k", 0.0), ALL),
]
NAMES = [name for name, _, _ in FAULTS]
SHININESS, NAN_REF, NMATERIALS = (NAMES.index(n) for n in
                                  ("differing shininess", "NaN ref", "wrong nmaterials"))


def call(lib, entry, q, render):
    """The entry point's validator, or its render with null buffers."""
    f, n = q.f, q.null
    scene = None if "scene" in n else C.byref(f.scene)
    params = None if "params" in n else C.byref(f.params)
    larr = None if "lights" in n else (abi.sdf_light * len(q.lights))(*q.lights)
    nl = len(q.lights) if q.nlights is None else q.nlights
    marr = None if "materials" in n else (abi.sdf_material * len(q.materials))(*q.materials)
    nm = len(q.materials) if q.nmaterials is None else q.nmaterials
    reflect = None if "reflect" in n else C.byref(q.reflect)
    fn = getattr(lib, ENTRIES[entry][render])
    if entry == "rays":
        rays = abi.sdf_rays(PTR, PTR, 1, 0, 0)
        return fn(scene, larr, nl, q.light_flags, marr, nm, reflect, C.byref(q.env), params,
                  C.byref(rays), *((None, None, BOGUS_STREAM) if render else ()))
    if entry == "points":
        pts = abi.sdf_points()   # no points: a valid call has nothing to launch
        out = abi.sdf_point_shade()
        out.rgba = PTR
        return fn(scene, larr, nl, q.light_flags, marr, nm, params, C.byref(pts),
                  *((C.byref(out), BOGUS_STREAM) if render else ()))
    head = [scene, C.byref(f.camera), larr, nl, q.light_flags]
    head += [marr] if entry == "lights" else [marr, nm]   # sdf_render_lights: the one material
    if entry in REFLECT:
        head.append(reflect)
    if entry == "env":
        head.append(C.byref(q.env))
    return fn(*head, params, None, *((None, None, None, BOGUS_STREAM) if render else ()))


def codes(lib, entry, faults):
    """(validator's, render's) letter for the base request with `faults`
    (indices into FAULTS) applied in order; SKIPPED where one does not apply."""
    if any(entry not in FAULTS[i][2] for i in faults):
        return SKIPPED, SKIPPED
    out = []
    for render in (0, 1):
        q = Request()
        for i in faults:
            FAULTS[i][1](q)
        out.append(LETTER[call(lib, entry, q, render)])
    return tuple(out)


def table(lib):
    """{entry: {"validate": {...}, "render": {...}}}, each {"single": one letter
    per fault, "pairs": {first fault: one letter per second fault}}."""
    n = range(len(FAULTS))
    t = {}
    for entry in ENTRIES:
        single = [codes(lib, entry, (i,)) for i in n]
        pairs = [[(SELF, SELF) if i == j else codes(lib, entry, (i, j)) for j in n] for i in n]
        t[entry] = {kind: {"single": "".join(c[k] for c in single),
                           "pairs": {NAMES[i]: "".join(c[k] for c in pairs[i]) for i in n}}
                    for k, kind in enumerate(("validate", "render"))}
    return t


def pair(t, entry, kind, first, second):
    return t[entry][kind]["pairs"][NAMES[first]][second]


def both_orders_are_held(t):
    """The one INVALID_ARG behind UNSUPPORTED checks, and its mirror."""
    for entry in REFLECT:
        for kind in ("validate", "render"):
            for a, b in ((SHININESS, NAN_REF), (NAN_REF, SHININESS)):
                assert pair(t, entry, kind, a, b) == "U", (entry, kind)
            for a, b in ((NAN_REF, NMATERIALS), (NMATERIALS, NAN_REF)):
                assert pair(t, entry, kind, a, b) == "I", (entry, kind)


def golden():
    return json.loads(GOLDEN.read_text())


def test_the_recording_is_of_this_fault_list():
    g = golden()
    assert g["faults"] == NAMES and list(g["codes"]) == list(ENTRIES)
    assert g["applies"] == {name: list(applies) for name, _, applies in FAULTS}
    both_orders_are_held(g["codes"])
    # every fault is refused on its own by every entry point it applies to
    for entry in ENTRIES:
        for kind in ("validate", "render"):
            assert set(g["codes"][entry][kind]["single"]) <= set("IU" + SKIPPED), (entry, kind)


def test_the_base_request_is_valid():
    lib = abi.load_library()
    for entry in ENTRIES:
        v, r = codes(lib, entry, ())
        # null buffers: a valid request is refused for them, and for nothing else
        assert (v, r) == ("K", "K" if entry == "points" else "I"), entry


def test_codes_are_the_recorded_ones():
    lib = abi.load_library()
    now, then = table(lib), golden()["codes"]
    for entry in ENTRIES:
        for kind in ("validate", "render"):
            a, b = now[entry][kind], then[entry][kind]
            assert a["single"] == b["single"], (entry, kind)
            for name in NAMES:
                assert a["pairs"][name] == b["pairs"][name], (entry, kind, name)
        # the render entry point gives its validator's code wherever that is not SDF_OK
        v, r = now[entry]["validate"], now[entry]["render"]
        assert all(x == y for x, y in zip(v["single"], r["single"]) if x != "K"), entry
        for name in NAMES:
            assert all(x == y for x, y in zip(v["pairs"][name], r["pairs"][name]) if x != "K"), \
                (entry, name)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_request_codes.py --record   (in a build of the commit to record)")
    t = table(abi.load_library())
    both_orders_are_held(t)
    GOLDEN.write_text(json.dumps(
        {"faults": NAMES, "applies": {name: list(applies) for name, _, applies in FAULTS},
         "letters": {"K": "SDF_OK", "I": "SDF_E_INVALID_ARG", "U": "SDF_E_UNSUPPORTED",
                     SKIPPED: "a fault does not apply", SELF: "the same fault twice"},
         "codes": t}, indent=1) + "\n")
    print("recorded", GOLDEN)
