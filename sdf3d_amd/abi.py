"""ctypes mirror of ``include/sdf_abi.h`` and the loader for ``libsdf3d.so``.

The struct layouts here must match the C header byte for byte;
``tests/test_abi.py`` checks every size against the C library's own view.
The loader raises if the in-tree HIP library is missing: there is no CPU
fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

SDF_ABI_VERSION = 12
MAX_DECODE_PARTS = 64   # SDF_MAX_DECODE_PARTS
SDF_MAX_PRIMS = 16
MAX_LIGHTS = 8        # SDF_MAX_LIGHTS (sdf_render_lights)
LIGHTS_COLOR = 0x1    # SDF_LIGHTS_COLOR: light i's diffuse and specular scaled by its colour
MAX_BOUNCES = 4       # SDF_MAX_BOUNCES (sdf_render_reflect)
REFLECT_WEIGHT = 0x1  # SDF_REFLECT_WEIGHT: with layer >= 0, W_layer instead of C_layer
ENV_SKY = 0x1         # SDF_ENV_SKY: a missed layer's colour is the sky along its ray
ENV_SUN = 0x2         # SDF_ENV_SUN: with ENV_SKY, a glow around sun_dir
ENV_FOG = 0x4         # SDF_ENV_FOG: linear distance fog on every layer that is not sky
RAYS_UNIT = 0x1       # SDF_RAYS_UNIT: sdf_render_rays uses dirs as given (unit vectors)
POINTS_EYE = 0x1      # SDF_POINTS_EYE: sdf_shade_points evaluates the specular term from `eye`
MESH_DENSE = 0x1      # SDF_MESH_DENSE: sdf_mesh_count evaluates every brick (no skipping)
MEASURE_OWNERS = 0x1  # SDF_MEASURE_OWNERS: sdf_measure also writes a row per owning primitive
MEASURE_SLOTS = 16    # SDF_MEASURE_SLOTS: int64 per row of sdf_measure
MEASURE_ROWS = 17     # SDF_MEASURE_ROWS: row 0 and a row per primitive
MEASURE_MAX_BLOCKS = 4096   # the workgroups of an sdf_measure launch at most (its workspace formula)

# status codes
SDF_OK = 0
SDF_E_INVALID_ARG = -1
SDF_E_UNSUPPORTED = -2
SDF_E_HIP = -3
SDF_E_NO_DEVICE = -4
SDF_E_COMM = -5
SDF_E_TIMEOUT = -6
COMM_ID_BYTES = 128
DRIVER_ROOT_AS_PEER = 0x1

# primitive kinds
PRIM_SPHERE, PRIM_PLANE, PRIM_BOX, PRIM_ROUND_BOX, PRIM_TORUS, PRIM_CAPSULE, PRIM_CYLINDER = range(7)
PRIM_NAMES = ["sphere", "plane", "box", "round_box", "torus", "capsule", "cylinder"]
# CSG ops
OP_UNION, OP_SMOOTH_UNION, OP_SUBTRACT, OP_INTERSECT, OP_SMOOTH_SUBTRACT, OP_SMOOTH_INTERSECT = range(6)
OP_COUNT = 6
OP_NAMES = ["union", "smooth_union", "subtract", "intersect", "smooth_subtract", "smooth_intersect"]
# scene kinds
SCENE_PRIMITIVES, SCENE_MANDELBULB = 0, 1
# flags / modes
FLAG_SHADOW, FLAG_AO = 0x1, 0x2
NORMAL_CENTRAL, NORMAL_TETRA = 0, 1
PRECISION_EXACT, PRECISION_FAST = 0, 1
DISPATCH_AUTO, DISPATCH_GENERIC, DISPATCH_UNCULLED = 0, 1, 2
FORMAT_RGBA32F, FORMAT_RGBA16F, FORMAT_RGBA8, FORMAT_RGB32F, FORMAT_TILES = 0, 1, 2, 3, 4
FORMAT_SHADE32F = 5   # the pixels' shading terms (ao, dif, x, 1): what TILES carries
TILING_FRAME_ROWS = 1
FORMAT_NAMES = {"rgba32f": FORMAT_RGBA32F, "rgba16f": FORMAT_RGBA16F, "rgba8": FORMAT_RGBA8,
                "rgb32f": FORMAT_RGB32F, "shade32f": FORMAT_SHADE32F}
# TILES (the frame losslessly compressed, the multi-device wire) is a byte
# stream of per-frame length, not a pixel format: see Renderer.alloc
FORMAT_CHANNELS = {FORMAT_RGBA32F: 4, FORMAT_RGBA16F: 4, FORMAT_RGBA8: 4, FORMAT_RGB32F: 3,
                   FORMAT_SHADE32F: 4}
TILES_HEADER_BYTES = 64   # used, ntiles, shade mode, 0, shading constants (sdf_abi.h)
# sdf_tiles_decode_checked status bits (sdf_abi.h SDF_TILES_BAD_*)
TILES_BAD_HEADER, TILES_BAD_TILE, TILES_BAD_FIELD = 0x1, 0x100, 0x10000


class sdf_primitive(C.Structure):
    _fields_ = [("kind", C.c_int32), ("op", C.c_int32), ("k", C.c_float),
                ("reserved", C.c_float), ("p", C.c_float * 12)]


class sdf_scene(C.Structure):
    _fields_ = [("kind", C.c_int32), ("count", C.c_int32),
                ("prims", sdf_primitive * SDF_MAX_PRIMS),
                ("bulb_center", C.c_float * 3), ("bulb_scale", C.c_float),
                ("bulb_iterations", C.c_int32), ("bulb_bailout", C.c_float),
                ("reserved", C.c_int32 * 2)]


class sdf_camera(C.Structure):
    _fields_ = [("view", C.c_float * 16), ("eye", C.c_float * 3), ("fov_deg", C.c_float),
                ("aspect", C.c_float), ("pi", C.c_float)]


class sdf_light(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("ambient", C.c_float), ("color", C.c_float * 3),
                ("reserved", C.c_float)]


class sdf_material(C.Structure):
    _fields_ = [("amb", C.c_float * 3), ("dif", C.c_float * 3), ("ref", C.c_float * 3),
                ("shininess", C.c_float)]


class sdf_reflect(C.Structure):
    _fields_ = [("bounces", C.c_int32), ("strength", C.c_float), ("layer", C.c_int32),
                ("flags", C.c_int32)]


class sdf_environment(C.Structure):
    _fields_ = [("flags", C.c_int32), ("horizon", C.c_float * 3), ("zenith", C.c_float * 3),
                ("ground", C.c_float * 3), ("sun_dir", C.c_float * 3),
                ("sun_color", C.c_float * 3), ("sun_exponent", C.c_float),
                ("fog_color", C.c_float * 3), ("fog_start", C.c_float), ("fog_end", C.c_float),
                ("reserved", C.c_int32 * 2)]


class sdf_hits(C.Structure):
    """Outputs of sdf_trace / sdf_trace_camera: device pointers, any may be NULL."""
    _fields_ = [("t", C.c_void_p), ("steps", C.c_void_p), ("normal", C.c_void_p),
                ("prim", C.c_void_p)]


class sdf_rays(C.Structure):
    """The rays of sdf_render_rays: device pointers to n x 3 packed fp32."""
    _fields_ = [("origins", C.c_void_p), ("dirs", C.c_void_p), ("n", C.c_int64),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class sdf_points(C.Structure):
    """The points of sdf_shade_points: device pointers to n x 3 packed fp32
    (normals may be NULL: the normal is evaluated at the point)."""
    _fields_ = [("points", C.c_void_p), ("normals", C.c_void_p), ("n", C.c_int64),
                ("eye", C.c_float * 3), ("lift", C.c_float), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class sdf_point_shade(C.Structure):
    """Outputs of sdf_shade_points: device pointers, any may be NULL (not all)."""
    _fields_ = [("rgba", C.c_void_p), ("ao", C.c_void_p), ("shadow", C.c_void_p),
                ("material", C.c_void_p), ("steps", C.c_void_p)]


class sdf_grid(C.Structure):
    """The lattice of sdf_mesh_count / sdf_mesh_emit: n cells of `cell` from `origin`."""
    _fields_ = [("origin", C.c_float * 3), ("cell", C.c_float * 3), ("n", C.c_int32 * 3),
                ("iso", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


class sdf_mesh_out(C.Structure):
    """Outputs of sdf_mesh_emit: device pointers with capacities; normal and prim may be NULL."""
    _fields_ = [("verts", C.c_void_p), ("max_verts", C.c_int64), ("tris", C.c_void_p),
                ("max_tris", C.c_int64), ("normal", C.c_void_p), ("prim", C.c_void_p)]


class sdf_mesh_sharp(C.Structure):
    """Sharp-feature vertices of sdf_mesh_emit_sharp: regula-falsi steps per crossing
    edge (0 .. 8) and descent steps of the vertex fit (0 .. 64); (0, 0) is sdf_mesh_emit."""
    _fields_ = [("refine", C.c_int32), ("iterations", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class sdf_grad_out(C.Structure):
    """Outputs of sdf_sample_grad: device pointers, any may be NULL (not all);
    grad_prims holds SDF_MAX_PRIMS x 16 floats, the slots of sdf_primitive."""
    _fields_ = [("dist", C.c_void_p), ("grad_points", C.c_void_p), ("grad_prims", C.c_void_p)]


class sdf_params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("max_steps", C.c_int32),
                ("max_dist", C.c_float), ("eps", C.c_float), ("shadow_k", C.c_float),
                ("normal_eps", C.c_float), ("shadow_offset", C.c_float),
                ("flags", C.c_int32), ("normal_mode", C.c_int32), ("ao_taps", C.c_int32),
                ("ao_step", C.c_float), ("ao_base", C.c_float), ("ao_falloff", C.c_float),
                ("ao_strength", C.c_float), ("precision", C.c_int32),
                ("dispatch", C.c_int32), ("output_format", C.c_int32),
                # sub-samples per axis: 0 / 1 one sample per pixel, 2 / 4 supersampling
                ("samples", C.c_int32), ("reserved", C.c_int32 * 1)]


class sdf_tiling(C.Structure):
    _fields_ = [("block_rows", C.c_int32), ("first_block", C.c_int32),
                ("block_stride", C.c_int32), ("flags", C.c_int32),
                ("block_run", C.c_int32), ("run_step", C.c_int32)]


class sdf_driver_config(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("share_root", C.c_int32),
                ("share_peer", C.c_int32), ("nbuf", C.c_int32), ("lag", C.c_int32),
                ("flags", C.c_int32), ("timeout_ms", C.c_int32), ("batch", C.c_int32)]


STRUCT_SIZES = {
    "sdf_primitive": 64, "sdf_scene": 8 + 64 * SDF_MAX_PRIMS + 32, "sdf_camera": 88,
    "sdf_light": 32, "sdf_material": 40, "sdf_params": 80, "sdf_tiling": 24,
    "sdf_driver_config": 36, "sdf_reflect": 16, "sdf_environment": 96, "sdf_hits": 32,
    "sdf_rays": 32, "sdf_grid": 48, "sdf_mesh_out": 48, "sdf_grad_out": 24,
    "sdf_points": 48, "sdf_point_shade": 40, "sdf_mesh_sharp": 16,
}
MAX_QUERY = 1 << 30   # rays or points of one sdf_trace / sdf_sample call

# every entry point of include/sdf_abi.h: name -> (restype, argtypes)
_P = C.POINTER
SIGNATURES = {
    "sdf_abi_version": (C.c_int, []),
    "sdf_defaults": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light), _P(sdf_material),
                               _P(sdf_params), C.c_int32, C.c_int32]),
    "sdf_validate": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light), _P(sdf_material),
                               _P(sdf_params), _P(sdf_tiling)]),
    "sdf_owned_rows": (C.c_int, [C.c_int32, _P(sdf_tiling)]),
    "sdf_share_tiling": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(sdf_tiling)]),
    "sdf_render": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light), _P(sdf_material),
                             _P(sdf_params), _P(sdf_tiling), C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdf_deinterleave": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sdf_format_bytes": (C.c_int, [C.c_int32]),
    "sdf_tiles_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "sdf_jit_count": (C.c_int, []),
    "sdf_kernel_id": (C.c_char_p, [C.c_int32]),
    "sdf_scene_bounds": (C.c_int, [_P(sdf_scene), _P(C.c_float), _P(C.c_float), _P(C.c_int32)]),
    "sdf_tiles_decode": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_void_p, C.c_void_p]),
    "sdf_tiles_decode_tilings": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, _P(sdf_tiling),
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sdf_schedule_create": (C.c_int, [C.c_int32, C.c_int32, _P(C.c_void_p)]),
    "sdf_schedule_destroy": (C.c_int, [C.c_void_p]),
    "sdf_schedule_order": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int32]),
    "sdf_render_scheduled": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light),
                                       _P(sdf_material), _P(sdf_params), _P(sdf_tiling),
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdf_validate_lights": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light), C.c_int32,
                                      C.c_int32, _P(sdf_material), _P(sdf_params),
                                      _P(sdf_tiling)]),
    "sdf_render_lights": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light), C.c_int32,
                                    C.c_int32, _P(sdf_material), _P(sdf_params), _P(sdf_tiling),
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdf_validate_materials": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light), C.c_int32,
                                         C.c_int32, _P(sdf_material), C.c_int32, _P(sdf_params),
                                         _P(sdf_tiling)]),
    "sdf_render_materials": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light), C.c_int32,
                                       C.c_int32, _P(sdf_material), C.c_int32, _P(sdf_params),
                                       _P(sdf_tiling), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "sdf_validate_reflect": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light), C.c_int32,
                                       C.c_int32, _P(sdf_material), C.c_int32, _P(sdf_reflect),
                                       _P(sdf_params), _P(sdf_tiling)]),
    "sdf_render_reflect": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light), C.c_int32,
                                     C.c_int32, _P(sdf_material), C.c_int32, _P(sdf_reflect),
                                     _P(sdf_params), _P(sdf_tiling), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "sdf_validate_env": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light), C.c_int32,
                                   C.c_int32, _P(sdf_material), C.c_int32, _P(sdf_reflect),
                                   _P(sdf_environment), _P(sdf_params), _P(sdf_tiling)]),
    "sdf_render_env": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light), C.c_int32,
                                 C.c_int32, _P(sdf_material), C.c_int32, _P(sdf_reflect),
                                 _P(sdf_environment), _P(sdf_params), _P(sdf_tiling), C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdf_validate_query": (C.c_int, [_P(sdf_scene), _P(sdf_params)]),
    "sdf_trace": (C.c_int, [_P(sdf_scene), _P(sdf_params), C.c_void_p, C.c_void_p, C.c_int64,
                            _P(sdf_hits), C.c_void_p]),
    "sdf_trace_camera": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_params), _P(sdf_hits),
                                   C.c_void_p]),
    "sdf_sample": (C.c_int, [_P(sdf_scene), _P(sdf_params), C.c_void_p, C.c_int64, C.c_void_p,
                             C.c_void_p, C.c_void_p]),
    "sdf_validate_mesh": (C.c_int, [_P(sdf_scene), _P(sdf_params), _P(sdf_grid)]),
    "sdf_mesh_workspace_bytes": (C.c_int64, [_P(sdf_grid)]),
    "sdf_mesh_count": (C.c_int, [_P(sdf_scene), _P(sdf_params), _P(sdf_grid), C.c_void_p,
                                 C.c_int64, C.c_void_p, C.c_void_p]),
    "sdf_mesh_emit": (C.c_int, [_P(sdf_scene), _P(sdf_params), _P(sdf_grid), C.c_void_p,
                                C.c_int64, _P(sdf_mesh_out), C.c_void_p]),
    "sdf_validate_mesh_sharp": (C.c_int, [_P(sdf_scene), _P(sdf_params), _P(sdf_grid),
                                          _P(sdf_mesh_sharp)]),
    "sdf_mesh_emit_sharp": (C.c_int, [_P(sdf_scene), _P(sdf_params), _P(sdf_grid),
                                      _P(sdf_mesh_sharp), C.c_void_p, C.c_int64, _P(sdf_mesh_out),
                                      C.c_void_p]),
    "sdf_validate_measure": (C.c_int, [_P(sdf_scene), _P(sdf_params), _P(sdf_grid), C.c_int32]),
    "sdf_measure_workspace_bytes": (C.c_int64, [_P(sdf_grid), C.c_int32]),
    "sdf_measure": (C.c_int, [_P(sdf_scene), _P(sdf_params), _P(sdf_grid), C.c_int32, C.c_void_p,
                              C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdf_validate_grad": (C.c_int, [_P(sdf_scene), _P(sdf_params)]),
    "sdf_grad_workspace_bytes": (C.c_int64, [C.c_int64]),
    "sdf_sample_grad": (C.c_int, [_P(sdf_scene), _P(sdf_params), C.c_void_p, C.c_int64,
                                  C.c_void_p, _P(sdf_grad_out), C.c_void_p, C.c_int64,
                                  C.c_void_p]),
    "sdf_validate_rays": (C.c_int, [_P(sdf_scene), _P(sdf_light), C.c_int32, C.c_int32,
                                    _P(sdf_material), C.c_int32, _P(sdf_reflect),
                                    _P(sdf_environment), _P(sdf_params), _P(sdf_rays)]),
    "sdf_render_rays": (C.c_int, [_P(sdf_scene), _P(sdf_light), C.c_int32, C.c_int32,
                                  _P(sdf_material), C.c_int32, _P(sdf_reflect),
                                  _P(sdf_environment), _P(sdf_params), _P(sdf_rays), C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "sdf_validate_points": (C.c_int, [_P(sdf_scene), _P(sdf_light), C.c_int32, C.c_int32,
                                      _P(sdf_material), C.c_int32, _P(sdf_params),
                                      _P(sdf_points)]),
    "sdf_shade_points": (C.c_int, [_P(sdf_scene), _P(sdf_light), C.c_int32, C.c_int32,
                                   _P(sdf_material), C.c_int32, _P(sdf_params), _P(sdf_points),
                                   _P(sdf_point_shade), C.c_void_p]),
    "sdf_camera_rays": (C.c_int, [_P(sdf_camera), _P(sdf_params), C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "sdf_tiles_decode_checked": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, _P(sdf_tiling),
                                           _P(C.c_int64), C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "sdf_heatmap": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                              C.c_void_p, C.c_void_p]),
    "sdf_render_multi": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light),
                                   _P(sdf_material), _P(sdf_params), C.c_int32, C.c_void_p,
                                   C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sdf_render_multi_release": (C.c_int, []),
    "sdf_render_frames": (C.c_int, [_P(sdf_scene), _P(sdf_camera), C.c_int32, _P(sdf_light),
                                    _P(sdf_material), _P(sdf_params), C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "sdf_comm_unique_id": (C.c_int, [C.c_char_p, C.c_void_p]),
    "sdf_comm_create": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                  _P(C.c_void_p)]),
    "sdf_comm_destroy": (C.c_int, [C.c_void_p]),
    "sdf_driver_create": (C.c_int, [_P(sdf_scene), _P(sdf_camera), _P(sdf_light),
                                    _P(sdf_material), _P(sdf_params), _P(sdf_driver_config),
                                    C.c_void_p, C.c_void_p, _P(C.c_void_p)]),
    "sdf_driver_set_camera": (C.c_int, [C.c_void_p, _P(sdf_camera)]),
    "sdf_driver_step": (C.c_int, [C.c_void_p, _P(C.c_int64)]),
    "sdf_driver_drain": (C.c_int, [C.c_void_p]),
    "sdf_driver_frame": (C.c_int, [C.c_void_p, C.c_int64, _P(C.c_void_p)]),
    "sdf_driver_read_frame": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                        C.c_void_p]),
    "sdf_driver_stats": (C.c_int, [C.c_void_p, _P(C.c_double), C.c_int32]),
    "sdf_driver_destroy": (C.c_int, [C.c_void_p]),
    "sdf_strerror": (C.c_char_p, [C.c_int]),
}

LIB_PATH = Path(__file__).resolve().parent / "lib" / "libsdf3d.so"
_lib = None


class SdfError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = _strerror(code)
        super().__init__(f"{what}: {msg} ({code})" if what else f"{msg} ({code})")


def _strerror(code: int) -> str:
    try:
        return load_library().sdf_strerror(code).decode()
    except Exception:  # pragma: no cover - library missing
        return f"error {code}"


def load_library(path: Path | str | None = None, any_version: bool = False) -> C.CDLL:
    """Load the in-tree HIP library; raise if it has not been built.
    any_version: accept another ABI version (measurement tools timing an
    older build of the same entry points side by side)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise RuntimeError(
            f"{p} is missing: build the HIP library first (python -m sdf3d_amd.build). "
            "There is no CPU fallback on the product path.")
    lib = C.CDLL(str(p))
    # the version first: a stale library lacks later entry points, and the
    # mismatch is the message to give, not a missing symbol
    lib.sdf_abi_version.restype = C.c_int
    lib.sdf_abi_version.argtypes = []
    v = lib.sdf_abi_version()
    if v != SDF_ABI_VERSION and not any_version:
        raise RuntimeError(f"libsdf3d ABI version {v} != {SDF_ABI_VERSION}: rebuild it "
                           "(python -m sdf3d_amd.build)")
    for name, (res, args) in SIGNATURES.items():
        if any_version and not hasattr(lib, name):
            continue   # an older build without a later entry point
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def check(code: int, what: str = "") -> None:
    if code != SDF_OK:
        raise SdfError(code, what)
